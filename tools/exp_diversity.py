"""Beyond-accuracy metrics (pcr_evaluate_diversity): what the diversity tail costs next to the score sweep.

For each shape (ml1m 6 040 x 3 706, k = 100; Netflix 480 189 x 17 770, k = 100), fp32 and fp64: a solver over a generated set of
20 training ratings per user on average, factors from initial(); after one warm-up call of each, --steps calls of
evaluate_diversity(cutoffs=(10, 100)) and of evaluate_topn(cutoffs=(10, 100)) on the same factors in the same process, each timed by
the solver's device events.  recommend/diversity (row norms, merge + exposure + novelty + ILD, reductions) stands next to
recommend/score of the same call; recommend/metrics of the top-N evaluation is the reference point for a fused merge tail.
Prints one JSON line per case with the medians over the calls (ms) and the ratio.

    python tools/exp_diversity.py [--steps 5] [--shapes ml1m,netflix]
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
CUTOFFS = (10, 100)
DIV_SLOTS = ("recommend/score", "recommend/diversity")
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
            dv = timed(s, lambda: s.evaluate_diversity(CUTOFFS), DIV_SLOTS, a.steps)
            tn = timed(s, lambda: s.evaluate_topn(CUTOFFS), TOPN_SLOTS, a.steps)
            st = s.evaluate_diversity(CUTOFFS)[-1]
            esz = 4 if prec == pcr.PCR_F32 else 8
            gathered = st["recs"] * ((k + 3) // 4 * 4) * esz
            rec = dict(shape=name, d1=d1, d2=d2, k=k, dtype="f32" if prec == pcr.PCR_F32 else "f64", users=st["users"], recs=st["recs"],
                       coverage=round(st["coverage"], 4), gini=round(st["gini"], 4), ild=round(st["ild"], 4),
                       score_ms=round(dv["recommend/score"], 3), diversity_ms=round(dv["recommend/diversity"], 3),
                       topn_score_ms=round(tn["recommend/score"], 3), topn_metrics_ms=round(tn["recommend/metrics"], 3),
                       diversity_over_score=round(dv["recommend/diversity"] / dv["recommend/score"], 3) if dv["recommend/score"] > 0 else None,
                       gather_gbs=round(gathered / (dv["recommend/diversity"] * 1e-3) / 1e9, 1) if dv["recommend/diversity"] > 0 else None)
            print(json.dumps(rec), flush=True)
            s.close()


if __name__ == "__main__":
    main()
