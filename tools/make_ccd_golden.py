"""Golden runs of the reference's CCDR1 solver (-s 0) for tests/test_ccd.py.

Runs the reference binary built by oracle/Makefile (oracle/_ref/omp-pmf-train, -n 1) on the golden data sets (edge5, mid5, real),
two small seeded synthetic sets, a set whose test file is not user-sorted and a set with users and items of more than 4096
ratings (the data sets are built by tests/ccd_data.py), and writes per data set
    tests/golden/ccd_<set>.json   {"cases": {tag: {"args": [...], "stdout": "..."}}}
    tests/golden/ccd_<set>.npz    pred_<tag>: omp-pmf-predict on the test file, as the integers of its %lf text (micro-units);
                                  U_<tag>, V_<tag>: the model, for the cases in MODELS (the tests compare every other case's model
                                  against the reference run live)

    python tools/make_ccd_golden.py
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from primalcr_amd import synth  # noqa: E402
from ccd_data import ratings  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")
OUT = os.path.join(ROOT, "tests", "golden")

# data set -> {tag: reference arguments}; every case runs with -s 0 -n 1
CASES = {
    "edge5": {"base": ["-k", "5", "-t", "3", "-l", "0.05"]},
    "real": {"base": ["-k", "6", "-t", "4", "-l", "0.1"]},
    "mid5": {
        "base": ["-k", "8", "-t", "3", "-l", "0.05"],
        "t0": ["-k", "8", "-t", "0", "-l", "0.05"],
        "k1": ["-k", "1", "-t", "3", "-l", "0.05"],
        "T1": ["-k", "8", "-t", "3", "-l", "0.05", "-T", "1"],
        "T0": ["-k", "8", "-t", "2", "-l", "0.05", "-T", "0"],
        "e05": ["-k", "8", "-t", "3", "-l", "0.05", "-e", "0.5"],
        "N1": ["-k", "8", "-t", "3", "-l", "0.05", "-N", "1"],
        "p0": ["-k", "8", "-t", "3", "-l", "0.05", "-p", "0"],
        "p0q1": ["-k", "8", "-t", "3", "-l", "0.05", "-p", "0", "-q", "1"],
    },
    "synth3": {"base": ["-k", "10", "-t", "5", "-l", "0.05"]},
    "synth4": {"base": ["-k", "7", "-t", "3", "-l", "0.08"]},
    "unsorted": {"base": ["-k", "5", "-t", "3", "-l", "0.05"]},
    "long": {"base": ["-k", "4", "-t", "2", "-l", "0.05"]},
}
MODELS = {("edge5", "base"), ("real", "base"), ("mid5", "base"), ("mid5", "t0"), ("synth3", "base"), ("synth4", "base"),
          ("unsorted", "base")}


def read_model(path):
    """The model file: long d1, long k, d1*k doubles, long d2, long k, d2*k doubles."""
    raw = open(path, "rb").read()
    d1, k = np.frombuffer(raw, np.int64, 2, 0)
    o = 16
    U = np.frombuffer(raw, np.float64, d1 * k, o).reshape(d1, k); o += 8 * d1 * k
    d2, k2 = np.frombuffer(raw, np.int64, 2, o); o += 16
    V = np.frombuffer(raw, np.float64, d2 * k2, o).reshape(d2, k2)
    return U, V


def main():
    exe, pred_exe = os.path.join(REF, "omp-pmf-train"), os.path.join(REF, "omp-pmf-predict")
    if not os.path.exists(exe):
        sys.exit("build the reference first: make -C oracle ref")
    for name, cases in CASES.items():
        with tempfile.TemporaryDirectory() as tmp:
            d = synth.write_dir(ratings(name), os.path.join(tmp, "data"))
            meta, arrays = {"cases": {}}, {}
            for tag, args in cases.items():
                model = os.path.join(tmp, tag + ".model")
                argv = ["-s", "0", "-n", "1"] + args
                r = subprocess.run([exe] + argv + [d, model], capture_output=True, text=True, check=True, cwd=tmp)
                U, V = read_model(model)
                pred = os.path.join(tmp, tag + ".pred")
                subprocess.run([pred_exe, os.path.join(d, "test.ratings"), model, pred], capture_output=True, check=True, cwd=tmp)
                meta["cases"][tag] = {"args": argv, "stdout": r.stdout}
                if (name, tag) in MODELS:
                    arrays["U_" + tag], arrays["V_" + tag] = U, V
                arrays["pred_" + tag] = np.rint(np.loadtxt(pred, ndmin=1) * 1e6).astype(np.int64)
            with open(os.path.join(OUT, "ccd_" + name + ".json"), "w") as f:
                json.dump(meta, f, indent=1)
            np.savez_compressed(os.path.join(OUT, "ccd_" + name + ".npz"), **arrays)
            print(name, len(cases), "cases")


if __name__ == "__main__":
    main()
