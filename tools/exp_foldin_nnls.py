#!/usr/bin/env python3
"""Non-negative fold-in (pcr_fold_in_nnls) against the ridge fold-in of the same build on the same users
-- the unconstrained solve, which is the first pivot and so a lower bound -- and against its own forced-CG arm.

Per cell (tools/exp_foldin_ridge.py's four shapes: users x ratings per user over 17 770 items at rank k, lambda = 0.05 weighted,
fp32 and fp64 storage), on Gaussian F ~ N(0, 1) / sqrt(k) and on its absolute value, three arms interleaved round by round in
one process, on a solver that holds V:
  ridge     Solver.fold_in_ridge: the foldin/ridge slot
  nnls      Solver.fold_in_nnls by the form rule (direct at k = 100, CG at k = 200): the foldin/nnls slot
  nnls_cg   pcr_tune nnls_form=cg: every pivot's solve by the masked matrix-free CG
For each arm the slot (device time of the launches) and the call's wall time; for the nnls arms pivots per user and the share of
coordinates at 0.  One warm-up round, then --rounds timed ones; median, min and max.  Prints one JSON line per cell.
Usage: python tools/exp_foldin_nnls.py [--rounds 5] [--out file.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import primalcr_amd as pcr  # noqa: E402
from exp_foldin_ridge import CELLS, D2, LAM, new_users, stat  # noqa: E402

ARMS = ("ridge", "nnls", "nnls_cg")
SLOT = {"ridge": "foldin/ridge", "nnls": "foldin/nnls", "nnls_cg": "foldin/nnls"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    results = []
    hidx, hitem, hval = new_users(64, 20, 1)
    for prec, pname in ((pcr.PCR_F32, "fp32"), (pcr.PCR_F64, "fp64")):
        for kind in ("gauss", "abs"):
            hosts = {}
            for n, per, k in CELLS:
                if k not in hosts:                                 # the solver that serves: any data set over the same items, V set
                    V = np.random.default_rng(5).normal(size=(D2, k)) / np.sqrt(k)
                    hosts[k] = pcr.Solver(pcr.Dataset.from_csr(64, D2, hidx, hitem, hval), pcr.Parameter(k=k, precision=prec, **{"lambda": LAM}))
                    hosts[k].set_factors(np.zeros((64, k)), np.abs(V) if kind == "abs" else V)
                    hosts[k].profile(True)
                host = hosts[k]
                ratings = new_users(n, per, 7)
                t = {f"{arm}_{w}": [] for arm in ARMS for w in ("wall", "slot")}
                stats = {}
                for rnd in range(a.rounds + 1):
                    for arm in ARMS:
                        with pcr.tuned(nnls_form="cg" if arm == "nnls_cg" else "auto"):
                            host.profile_reset()
                            t0 = time.perf_counter()
                            _, stats[arm] = host.fold_in_ridge(ratings) if arm == "ridge" else host.fold_in_nnls(ratings)
                            w = time.perf_counter() - t0
                            ms, _ = host.profile_get(SLOT[arm])
                        if rnd > 0:
                            t[f"{arm}_wall"].append(w * 1e3); t[f"{arm}_slot"].append(ms)
                res = {"storage": pname, "F": kind, "users": n, "ratings_per_user": per, "k": k, "lambda": LAM, "rounds": a.rounds, "stats": stats,
                       "pivots_per_user": {arm: stats[arm]["pivots"] / n for arm in ARMS[1:]},
                       "zero_share": {arm: stats[arm]["zeros"] / (n * k) for arm in ARMS[1:]},
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
