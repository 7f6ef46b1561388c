#!/usr/bin/env python3
"""Confidence-weighted / implicit fold-in (pcr_fold_in_conf) against the ridge fold-in of the same users
and against its own forced-CG arm; tools/exp_foldin_ridge.py's shapes and method.

Per cell (users x ratings per user over 17 770 items at rank k, lambda = 0.05 weighted, fp32 and fp64 storage) five arms,
interleaved round by round in one process, on a solver that holds V:
  ridge          pcr_fold_in_ridge: the unweighted problem (slot foldin/ridge; its kernels are the parent commit's, unchanged)
  weights        pcr_fold_in_conf with one weight of {0.25, 0.5, 1, 2, 4} per rating, alpha = 0: the ridge rule's forms
  weights_cg     the same under pcr_tune ridge_form=cg
  implicit       the same weights and alpha = 0.5: primal at every length (k = 100: a 112-side system where the ridge entry's
                 dual form solves a 32-side one for 20 ratings), CG at k = 200
  implicit_cg    the same under pcr_tune ridge_form=cg
For each arm the slot (device time of the launches; the conf arms: foldin/conf, and foldin/conf.gram for the catalogue Gram) and
the call's wall time.  One warm-up round, then --rounds timed ones; median, min and max.  Prints one JSON line per cell.
Usage: python tools/exp_foldin_conf.py [--rounds 5] [--out file.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import primalcr_amd as pcr  # noqa: E402
from exp_foldin_ridge import CELLS, D2, LAM, new_users, stat  # noqa: E402

ALPHA = 0.5
ARMS = (("ridge", None, False), ("weights", 0.0, False), ("weights_cg", 0.0, True), ("implicit", ALPHA, False), ("implicit_cg", ALPHA, True))


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
            if k not in hosts:
                V = np.random.default_rng(5).normal(size=(D2, k)) / np.sqrt(k)
                hosts[k] = pcr.Solver(pcr.Dataset.from_csr(64, D2, hidx, hitem, hval), pcr.Parameter(k=k, precision=prec, **{"lambda": LAM}))
                hosts[k].set_factors(np.zeros((64, k)), V)
                hosts[k].profile(True)
            host = hosts[k]
            ratings = new_users(n, per, 7)
            w = np.random.default_rng(9).choice(np.array([0.25, 0.5, 1.0, 2.0, 4.0]), size=len(ratings[1]))
            t = {f"{arm}_{x}": [] for arm, _, _ in ARMS for x in ("wall", "slot")}
            t["gram_slot"] = []
            stats = {}
            for rnd in range(a.rounds + 1):
                for arm, alpha, cg in ARMS:
                    with pcr.tuned(ridge_form="cg" if cg else "auto"):
                        host.profile_reset()
                        t0 = time.perf_counter()
                        if alpha is None:
                            _, stats[arm] = host.fold_in_ridge(ratings)
                        else:
                            _, stats[arm] = host.fold_in_conf(ratings, weights=w, alpha=alpha)
                        wall = time.perf_counter() - t0
                        ms, _ = host.profile_get("foldin/ridge" if alpha is None else "foldin/conf")
                        gram = host.profile_get("foldin/conf.gram")[0] if arm == "implicit" else None
                    if rnd > 0:
                        t[f"{arm}_wall"].append(wall * 1e3); t[f"{arm}_slot"].append(ms)
                        if gram is not None:
                            t["gram_slot"].append(gram)
            res = {"storage": pname, "users": n, "ratings_per_user": per, "k": k, "lambda": LAM, "alpha": ALPHA, "rounds": a.rounds, "stats": stats,
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
