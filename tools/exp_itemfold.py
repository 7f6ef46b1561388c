#!/usr/bin/env python3
"""Item fold-in (pcr_fold_in_items) against the only route the library offered before it, on the
ml1m-shaped synthetic set (6040 x 3952, 939 809 ratings), k = 100, lambda = 5000, fp32, steps = 10.

Per workload (new items x raters per item, the raters drawn uniformly among the users, ratings 1..5) two arms, interleaved round
by round in one process:
  itemfold     Solver.fold_in_items on a solver that holds the trained factors: the itemfold/scores slot (the rater table) and the
               itemfold/newton slot (device time of the launches), and the call's wall time
  update_V     one update_V of a Solver over the data with the new items appended (its creation is not timed): the retraining
               step a caller had to take before -- it moves every row of V, not the new ones alone
One warm-up round, then --rounds timed ones; median, min and max.  Prints one JSON line per workload.
Usage: python tools/exp_itemfold.py [--rounds 5] [--out file.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import primalcr_amd as pcr  # noqa: E402
from primalcr_amd import synth  # noqa: E402

K, LAM, STEPS = 100, 5000.0, 10


def new_items(d1, n, per, seed):
    rng = np.random.default_rng(seed)
    user = np.concatenate([np.sort(rng.choice(d1, size=per, replace=False)) for _ in range(n)]).astype(np.int32)
    return np.arange(n + 1, dtype=np.int64) * per, user, rng.integers(1, 6, size=n * per).astype(np.float64)


def appended(d1, d2, idx, it, val, new):
    """The training data with the new items as items d2 .. d2 + n - 1 (rows item-ascending)."""
    nidx, nuser, nval = new
    n = len(nidx) - 1
    user = np.concatenate([np.repeat(np.arange(d1), np.diff(idx)), nuser])
    item = np.concatenate([it, np.repeat(np.arange(d2, d2 + n), np.diff(nidx))])
    o = np.lexsort((item, user))
    index = np.concatenate([[0], np.cumsum(np.bincount(user, minlength=d1))]).astype(np.int64)
    return pcr.Dataset.from_csr(d1, d2 + n, index, item[o].astype(np.int32), np.concatenate([val, nval])[o])


def stat(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    R = synth.generate("ml1m")
    ds = pcr.Dataset.from_ratings(R)
    idx, it, val = ds.csr(0)
    prm = dict(k=K, precision=pcr.PCR_F32, **{"lambda": LAM})
    host = pcr.Solver(ds, pcr.Parameter(**prm))
    host.set_factors(pcr.initial(R.d1, K), pcr.initial(R.d2, K))
    host.iterate(2)
    U, V = host.get_factors()
    host.profile(True)
    results = []
    for n, per in ((1000, 20), (100, 2000)):
        new = new_items(R.d1, n, per, 7)
        big = pcr.Solver(appended(R.d1, R.d2, idx, it, val, new), pcr.Parameter(**prm))
        Vx = np.vstack([V, np.zeros((n, K))])
        t = {"itemfold_wall": [], "itemfold_scores": [], "itemfold_newton": [], "update_V_wall": []}
        for rnd in range(a.rounds + 1):
            host.profile_reset()
            t0 = time.perf_counter()
            rows, st = host.fold_in_items(new, steps=STEPS)
            w = time.perf_counter() - t0
            sc, nw = host.profile_get("itemfold/scores")[0], host.profile_get("itemfold/newton")[0]
            big.set_factors(U, Vx)
            big.comp_m(want=False)
            big.sync()
            t0 = time.perf_counter()
            big.update_V()
            big.sync()
            wv = time.perf_counter() - t0
            if rnd > 0:
                t["itemfold_wall"].append(w * 1e3); t["itemfold_scores"].append(sc); t["itemfold_newton"].append(nw); t["update_V_wall"].append(wv * 1e3)
        big.close()
        unique = int(len(np.unique(new[1])))
        table = int(np.diff(idx)[np.unique(new[1])].sum())
        res = {"items": n, "raters_per_item": per, "k": K, "lambda": LAM, "steps": STEPS, "rounds": a.rounds, "itemfold_stats": st,
               "unique_raters": unique, "table_ratings": table, "ms": {k: stat(v) for k, v in t.items()}}
        print(json.dumps(res), flush=True)
        results.append(res)
    host.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
