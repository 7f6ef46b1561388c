#!/usr/bin/env python3
"""Ridge fold-in (pcr_fold_in_ridge): the direct forms against the forced-CG arm of the same build.

Per cell (users x ratings per user over 17 770 items at rank k, lambda = 0.05 weighted, fp32 and fp64 storage) two arms,
interleaved round by round in one process, on a solver that holds V:
  default   the form rule (dual for the 20-rating cells, primal for the 200- and 2000-rating cells)
  cg        pcr_tune ridge_form=cg: every user by matrix-free CG, the only other route this tree offers
For each arm the foldin/ridge slot (device time of the launches) and the call's wall time.  One warm-up round, then --rounds
timed ones; median, min and max.  Prints one JSON line per cell.
Usage: python tools/exp_foldin_ridge.py [--rounds 5] [--out file.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import primalcr_amd as pcr  # noqa: E402

D2, LAM = 17770, 0.05
CELLS = ((100000, 20, 100), (100000, 20, 200), (10000, 200, 100), (1000, 2000, 100))


def new_users(n, per, seed):
    rng = np.random.default_rng(seed)
    edges = np.linspace(0, D2, per + 1).astype(np.int64)           # one item per stratum: distinct and ascending inside a user
    item = (edges[:-1] + (rng.random((n, per)) * np.diff(edges)).astype(np.int64)).astype(np.int32)
    index = np.arange(n + 1, dtype=np.int64) * per
    return index, item.reshape(-1), rng.integers(1, 6, size=n * per).astype(np.float64)


def stat(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    results = []
    hidx, hitem, hval = new_users(64, 20, 1)
    for prec, pname in ((pcr.PCR_F32, "fp32"), (pcr.PCR_F64, "fp64")):
        hosts = {}
        for n, per, k in CELLS:
            if k not in hosts:                                     # the solver that serves: any data set over the same items, V set
                V = np.random.default_rng(5).normal(size=(D2, k)) / np.sqrt(k)
                hosts[k] = pcr.Solver(pcr.Dataset.from_csr(64, D2, hidx, hitem, hval), pcr.Parameter(k=k, precision=prec, **{"lambda": LAM}))
                hosts[k].set_factors(np.zeros((64, k)), V)
                hosts[k].profile(True)
            host = hosts[k]
            ratings = new_users(n, per, 7)
            t = {f"{arm}_{w}": [] for arm in ("default", "cg") for w in ("wall", "slot")}
            stats = {}
            for rnd in range(a.rounds + 1):
                for arm in ("default", "cg"):
                    with pcr.tuned(ridge_form="cg" if arm == "cg" else "auto"):
                        host.profile_reset()
                        t0 = time.perf_counter()
                        _, stats[arm] = host.fold_in_ridge(ratings)
                        w = time.perf_counter() - t0
                        ms, _ = host.profile_get("foldin/ridge")
                    if rnd > 0:
                        t[f"{arm}_wall"].append(w * 1e3); t[f"{arm}_slot"].append(ms)
            res = {"storage": pname, "users": n, "ratings_per_user": per, "k": k, "lambda": LAM, "rounds": a.rounds, "stats": stats,
                   "ms": {key: stat(v) for key, v in t.items()}}
            print(json.dumps(res), flush=True)
            results.append(res)
        for h in hosts.values():
            h.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
