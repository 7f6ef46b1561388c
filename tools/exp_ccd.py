"""CCDR1 (solver type 0) on the device: ms per outer iteration on the ml1m shape and a Netflix-shaped set, against the reference.

Generates both shapes from seeds, runs pcr_iterate for CCDR1 (k = 100, lambda = 0.05, -T 5) after a warm-up outer iteration with
device-event timing, and prints one JSON line: ms per outer iteration, launches per outer iteration and per rank, the bytes the
executed work moves (from the shapes and the inner iterations and ranks that ran), and -- where oracle/_ref exists -- the reference binary's `-s 0 -p 0 -n 16` wall time per
outer iteration on the same data and host.

    python tools/exp_ccd.py [--steps 3] [--netflix-nnz 20000000] [--f32]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import primalcr_amd as pcr  # noqa: E402
from primalcr_amd import synth  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "omp-pmf-train")
SLOTS = ("ccd/begin", "ccd/vsweep", "ccd/usweep", "ccd/decide", "ccd/resid", "ccd/final")


def moved_bytes(nnz, inner, ranks, rb):
    """Bytes the executed work moves at the algorithm's level: per sweep every rating reads its residual (rb), its index (4) and
    the other side's fp64 value (8); the add-back in a rank's first sweeps also writes the residual (rb per copy); the end of a
    rank reads and writes both residual copies with both indices.  Vectors (d1 + d2) are noise at these shapes."""
    sweep = nnz * (rb + 4 + 8)
    return 2 * inner * sweep + ranks * (2 * nnz * rb + 2 * nnz * (2 * rb + 8))


def measure(R, k, T, steps, f64):
    ds = pcr.Dataset.from_ratings(R)
    s = pcr.Solver(ds, pcr.Parameter(solver_type=pcr.PCR_SOLVER_CCDR1, k=k, do_predict=0, verbose=0,
                                     precision=pcr.PCR_F64 if f64 else pcr.PCR_F32, **{"lambda": 0.05}))
    s.set_ccd_params(maxinneriter=T)
    s.set_factors(pcr.initial_col(R.d1, k), None)
    base = s.iterate(1)[0]                                         # warm-up (outer iteration 1: no add-back)
    recs = s.iterate(steps)
    ms = (recs[-1]["seconds"]) * 1e3 / steps
    s.profile(True)
    s.profile_reset()
    s.iterate(1)
    prof = s.profile_all()
    launches = sum(prof.get(n, (0, 0))[1] for n in SLOTS)
    kernel_ms = {n: round(prof[n][0], 3) for n in SLOTS if n in prof}
    inner = recs[-1]["cg_v"] - base["cg_v"]
    ranks = recs[-1]["cg_u"] - base["cg_u"]
    s.close()
    return ms, launches, kernel_ms, inner, ranks


def ref_time(R, k, T, steps):
    if not os.path.exists(REF):
        return None
    with tempfile.TemporaryDirectory() as tmp:
        d = synth.write_dir(R, os.path.join(tmp, "data"))
        out = []
        for t in (1, 1 + steps):                                   # the difference removes loading and set-up
            t0 = time.perf_counter()
            subprocess.run([REF, "-s", "0", "-k", str(k), "-t", str(t), "-l", "0.05", "-T", str(T), "-p", "0", "-n", "16", d,
                            os.path.join(tmp, "m")], check=True, capture_output=True, timeout=3600)
            out.append(time.perf_counter() - t0)
        return (out[1] - out[0]) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--netflix-nnz", type=int, default=20_000_000)
    ap.add_argument("--f32", action="store_true")
    ap.add_argument("--no-ref", action="store_true")
    a = ap.parse_args()
    k, T, f64 = 100, 5, not a.f32
    res = {"k": k, "T": T, "precision": "f64" if f64 else "f32", "shapes": {}}
    for name, R in (("ml1m", synth.generate("ml1m", seed=7)),
                    ("netflix_slice", synth.generate_fast("netflix", seed=11, d1=int(480189 * a.netflix_nnz / 1e8), nnz=a.netflix_nnz))):
        d1, d2, nnz, _ = pcr.Dataset.from_ratings(R).dims()
        ms, launches, kms, inner, ranks = measure(R, k, T, a.steps, f64)
        gb = moved_bytes(nnz, inner / a.steps, ranks / a.steps, 8 if f64 else 4) / 1e9
        res["shapes"][name] = {
            "d1": d1, "d2": d2, "nnz": nnz, "ms_per_outer": round(ms, 3), "launches_per_outer": launches,
            "launches_per_rank": launches / k, "inner_iters_per_outer": inner / a.steps, "ranks_run_per_outer": ranks / a.steps,
            "kernel_ms_one_outer": kms, "algorithm_GB_per_outer": round(gb, 2), "algorithm_GBps": round(gb / (ms / 1e3), 1),
            "ref_ms_per_outer_n16": None if a.no_ref else ref_time(R, k, T, a.steps)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
