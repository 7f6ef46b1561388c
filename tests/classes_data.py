"""The rating set and knob sets of the U-step length-class tests (tests/test_classes.py, the GPU cell in tests/test_gpu_parity.py)
and of tools/record_ustep_classes.py, which recorded tests/golden/ustep_classes.json from them.

One rating set designed by user length: a user on each side of every class bound, enough short users for a many-user class,
and more mid-length users (1025..4096 ratings) than a quarter of the CUs, so that the 2048 class and the throughput forms
appear.  Ratings are 1..5, so every user has at most five levels."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

D2, K = 5003, 8
EDGE_LENGTHS = [1, 16, 32, 33, 64, 65, 128, 129, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 5000]
KNOB_SETS = [
    {},
    {"ustep_mode": 1},
    {"ustep_mode": 2},
    {"cluster_k": 1},
    {"cluster_users": 64},
    {"ubins": "16:64:1,48:64:1,200:256:0,700:256:0"},
    {"ustep_gram": 64},
    {"window_cache": 0},
]
PRECISIONS = ["f64", "f32"]


def case_id(precision, knobs):
    return precision + "".join(f",{k}={v}" for k, v in knobs.items())


def lengths():
    """Ratings per user, in user order (a fixed shuffle: ties in length are broken by user order in the class layout)."""
    lens = np.array(EDGE_LENGTHS + [8] * 300 + list(range(1100, 1170)), np.int64)
    return lens[np.random.default_rng(5).permutation(len(lens))]


def rating_set():
    """(d1, d2, user, item, val) as triplets, items ascending per user."""
    rng = np.random.default_rng(6)
    lens = lengths()
    user = np.repeat(np.arange(len(lens)), lens)
    item = np.concatenate([np.sort(rng.choice(D2, int(n), replace=False)) for n in lens])
    val = rng.integers(1, 6, user.shape[0]).astype(np.float64)
    return len(lens), D2, user, item, val


def levels_per_user(user, val, d1):
    """Distinct rating values of every user (the level count the class layout reads)."""
    pairs = np.unique(np.stack([user, val.astype(np.int64)]), axis=1)
    return np.bincount(pairs[0], minlength=d1)


def harness_case(precision, knobs, ncu):
    """The plain-text case csrc/check/classes_dump reads: a header line of key=value pairs, then `length levels` per user."""
    d1, _, user, _, val = rating_set()
    lens, lev = lengths(), levels_per_user(user, val, d1)
    ld = (K + 3) & ~3
    head = [f"precision={precision}", f"ld={ld}", f"ncu={ncu}", f"users={d1}"] + [f"{k}={v}" for k, v in knobs.items()]
    return " ".join(head) + "\n" + "".join(f"{int(n)} {int(t)}\n" for n, t in zip(lens, lev))


def build_dump():
    """Compiles csrc/check/classes_dump (a no-op of make when it is current) and returns its path."""
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "primalcr_amd", "csrc"), "classes_dump"], check=True)
    return os.path.join(ROOT, "primalcr_amd", "bin", "classes_dump")


def run_dump(exe, tmp, precision, knobs, ncu):
    """classes_dump on harness_case(...): (exit code, one dict per `class` line, the scalar outputs, the raw output)."""
    path = os.path.join(str(tmp), "case.txt")
    with open(path, "w") as f:
        f.write(harness_case(precision, knobs, ncu))
    p = subprocess.run([exe, path], capture_output=True, text=True)
    classes, scalars = [], {}
    for line in p.stdout.splitlines():
        if line.startswith("class "):
            _, name, *kv = line.split()
            classes.append(dict({"name": name}, **{k: int(v) for k, v in (x.split("=") for x in kv)}))
        elif not line.startswith("error"):
            scalars.update({k: int(v) for k, v in (x.split("=") for x in line.split())})
    return p.returncode, classes, scalars, p.stdout
