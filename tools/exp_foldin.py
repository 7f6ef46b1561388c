#!/usr/bin/env python3
"""Fold-in (pcr_fold_in) against the route the library offered before it, on cold-start workloads.

Per workload (users x ratings per user over 17 770 items, k = 100, lambda = 5000, fp32, steps = 10) two arms, interleaved
round by round in one process:
  foldin       Solver.fold_in on a solver that holds V: the foldin/newton slot (device time of the launches) and the call's wall
               time; pcr.fold_in (the model entry, which also uploads V) is timed beside it
  solver       a Solver over the new users: creation + set_factors + 10 x (comp_m, update_U) + get_factors
One warm-up round, then --rounds timed ones; median, min and max per arm, and the rows of V gathered per user for both routes.
Prints one JSON line per workload.  Usage: python tools/exp_foldin.py [--rounds 5] [--out file.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import primalcr_amd as pcr  # noqa: E402

D2, K, LAM, STEPS = 17770, 100, 5000.0, 10


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
    V = np.random.default_rng(5).normal(size=(D2, K)) / np.sqrt(K)
    # the solver that serves: any data set over the same items (a few users), V set
    hidx, hitem, hval = new_users(64, 20, 1)
    host = pcr.Solver(pcr.Dataset.from_csr(64, D2, hidx, hitem, hval), pcr.Parameter(k=K, precision=pcr.PCR_F32, **{"lambda": LAM}))
    host.set_factors(np.zeros((64, K)), V)
    host.profile(True)
    results = []
    for n, per in ((100000, 20), (10000, 200)):
        ratings = new_users(n, per, 7)
        t = {"foldin_wall": [], "foldin_slot": [], "foldin_model_wall": [], "solver_wall": []}
        rows = {}
        for rnd in range(a.rounds + 1):
            rec = rnd > 0
            host.profile_reset()
            t0 = time.perf_counter()
            U, fold_stats, pu = host.fold_in(ratings, steps=STEPS, per_user=True)
            w = time.perf_counter() - t0
            ms, _ = host.profile_get("foldin/newton")
            if rec:
                t["foldin_wall"].append(w * 1e3); t["foldin_slot"].append(ms)
            # passes over the user's rows: the state at the start and one per line-search try, one per gradient, two per CG iteration
            rows["foldin"] = float((1 + pu[:, 2] + pu[:, 0] + (pu[:, 5] != pcr.PCR_FOLDIN_STEP_CAP) + 2 * pu[:, 1]).mean())
            t0 = time.perf_counter()
            pcr.fold_in(V, ratings, LAM, steps=STEPS, dtype=pcr.PCR_F32)
            if rec:
                t["foldin_model_wall"].append((time.perf_counter() - t0) * 1e3)
            with pcr.tuned(count_rows=1 if rnd == 0 else 0):
                t0 = time.perf_counter()
                s = pcr.Solver(pcr.Dataset.from_csr(n, D2, *ratings), pcr.Parameter(k=K, precision=pcr.PCR_F32, **{"lambda": LAM}))
                s.set_factors(np.zeros((n, K)), V)
                for _ in range(STEPS):
                    s.comp_m(want=False)
                    s.update_U()
                s.get_factors()
                w = time.perf_counter() - t0
                if rnd == 0:
                    rows["solver"] = s.counter("ustep_row_gathers") / (n * per) + STEPS      # + comp_m's pass per step
                s.close()
            if rec:
                t["solver_wall"].append(w * 1e3)
        res = {"users": n, "ratings_per_user": per, "k": K, "lambda": LAM, "steps": STEPS, "rounds": a.rounds, "foldin_stats": fold_stats,
               "rows_of_V_per_rating": rows, "ms": {k: stat(v) for k, v in t.items()}}
        print(json.dumps(res), flush=True)
        results.append(res)
    host.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
