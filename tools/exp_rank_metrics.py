"""Exact rank metrics (pcr_evaluate_ranks): what the counting tail costs next to the selecting one.

For each shape (ml1m 6 040 x 3 706, k = 100; Netflix 480 189 x 17 770, k = 100), fp32 and fp64: a solver over a generated set of
20 training and 10 held-out ratings per user on average, factors from initial(); after one warm-up call of each, --steps calls of
evaluate_ranks() and of evaluate_topn(cutoffs=(10,)) on the same factors in the same process, each timed by the solver's device
events.  Both sweeps run the same GEMM over the same users and items: ranks/count against recommend/score is the price of counting
over selecting.  Prints one JSON line per case with the medians over the calls (ms) and the ratio.

    python tools/exp_rank_metrics.py [--steps 5] [--shapes ml1m,netflix]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import primalcr_amd as pcr  # noqa: E402
from primalcr_amd import synth  # noqa: E402

SHAPES = {"ml1m": (6040, 3706, 100), "netflix": (480189, 17770, 100)}
RANK_SLOTS = ("ranks/relscore", "ranks/count", "ranks/finish")
TOPN_SLOTS = ("recommend/score", "recommend/metrics")


def timed(s, call, slots, steps):
    """Median over `steps` calls of each slot's device time per call (ms)."""
    call()                                           # warm-up (code object, tables, allocation)
    s.profile(True)
    per = {n: [] for n in slots}
    for _ in range(steps):
        s.profile_reset()
        call()
        for n in slots:
            per[n].append(s.profile_get(n)[0])
    s.profile(False)
    return {n: float(np.median(v)) for n, v in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--shapes", default="ml1m,netflix")
    a = ap.parse_args()
    for name in a.shapes.split(","):
        d1, d2, k = SHAPES[name]
        R = synth.generate_fast("netflix", d1=d1, d2=d2, nnz=20 * d1)
        ds = pcr.Dataset.from_ratings(R)
        for prec in (pcr.PCR_F32, pcr.PCR_F64):
            s = pcr.Solver(ds, pcr.Parameter(k=k, precision=prec, do_predict=0, verbose=0))
            s.set_factors(pcr.initial(d1, k), pcr.initial(d2, k))
            rk = timed(s, lambda: s.evaluate_ranks(), RANK_SLOTS, a.steps)
            tn = timed(s, lambda: s.evaluate_topn((10,)), TOPN_SLOTS, a.steps)
            st = s.evaluate_ranks()
            rec = dict(shape=name, d1=d1, d2=d2, k=k, dtype="f32" if prec == pcr.PCR_F32 else "f64", users=st["users"],
                       relevant=st["relevant"], relscore_ms=round(rk["ranks/relscore"], 3), count_ms=round(rk["ranks/count"], 3),
                       finish_ms=round(rk["ranks/finish"], 3), topn_score_ms=round(tn["recommend/score"], 3),
                       topn_metrics_ms=round(tn["recommend/metrics"], 3),
                       count_over_score=round(rk["ranks/count"] / tn["recommend/score"], 3) if tn["recommend/score"] > 0 else None,
                       tflops_count=round(2.0 * st["users"] * d2 * k / (rk["ranks/count"] * 1e-3) / 1e12, 2) if rk["ranks/count"] > 0 else None)
            print(json.dumps(rec), flush=True)
            s.close()


if __name__ == "__main__":
    main()
