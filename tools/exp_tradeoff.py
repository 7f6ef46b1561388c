"""The theta sweep (pcr_evaluate_rerank): what scoring once buys next to one recommend_diverse() call per theta.

For each shape (ml1m 6 040 x 3 706, k = 100; Netflix 480 189 x 17 770, k = 100), fp32 and fp64, (topk, pool) = (10, 100) and nth = 1
and 4 thetas: a solver over a generated set of 20 training ratings per user on average, factors from initial(); after one warm-up
call, --steps calls of Solver.evaluate_rerank(thetas), each timed by the solver's device events: recommend/score (one launch per
user batch, whatever nth is), recommend/rerank (the selection, nth launches per batch) and recommend/listmetrics (the row norms,
the metrics of the lists, the reductions).  Next to it the path without the sweep: nth separate Solver.recommend_diverse() calls,
their recommend/score and recommend/rerank summed (the lists then still have to be copied out and evaluated on the host, which is
not timed here).  Prints one JSON line per case with the medians over the calls (ms).  Nothing here is a pass / fail threshold.

    python tools/exp_tradeoff.py [--steps 5] [--shapes ml1m,netflix] [--dtypes f32,f64] [--nth 1,4] [--case 10:100]
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
SWEEP_SLOTS = ("recommend/score", "recommend/rerank", "recommend/listmetrics")
PLAIN_SLOTS = ("recommend/score", "recommend/rerank")


def timed(s, call, steps, slots):
    """Median over `steps` calls of each slot's device time per call (ms)."""
    call()                                           # warm-up (code object, allocation)
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
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--nth", default="1,4")
    ap.add_argument("--case", default="10:100")
    a = ap.parse_args()
    topk, pool = (int(x) for x in a.case.split(":"))
    for name in a.shapes.split(","):
        d1, d2, k = SHAPES[name]
        R = synth.generate_fast("netflix", d1=d1, d2=d2, nnz=20 * d1)
        ds = pcr.Dataset.from_ratings(R)
        for dt in a.dtypes.split(","):
            prec = pcr.PCR_F32 if dt == "f32" else pcr.PCR_F64
            s = pcr.Solver(ds, pcr.Parameter(k=k, precision=prec, do_predict=0, verbose=0))
            s.set_factors(pcr.initial(d1, k), pcr.initial(d2, k))
            for nth in (int(x) for x in a.nth.split(",")):
                thetas = tuple(np.linspace(0.0, 1.0, nth)) if nth > 1 else (0.5,)
                sweep = timed(s, lambda: s.evaluate_rerank(thetas, pool=pool, cutoffs=(topk,)), a.steps, SWEEP_SLOTS)

                def separate():
                    for th in thetas:
                        s.recommend_diverse(topk, pool=pool, theta=float(th))
                plain = timed(s, separate, a.steps, PLAIN_SLOTS)
                total = sum(sweep.values())
                print(json.dumps(dict(shape=name, d1=d1, d2=d2, k=k, dtype=dt, topk=topk, pool=pool, nth=nth,
                                      sweep_score_ms=round(sweep["recommend/score"], 3), sweep_rerank_ms=round(sweep["recommend/rerank"], 3),
                                      sweep_listmetrics_ms=round(sweep["recommend/listmetrics"], 3), sweep_total_ms=round(total, 3),
                                      separate_score_ms=round(plain["recommend/score"], 3), separate_rerank_ms=round(plain["recommend/rerank"], 3),
                                      separate_total_ms=round(sum(plain.values()), 3))), flush=True)
            s.close()


if __name__ == "__main__":
    main()
