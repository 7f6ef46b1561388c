"""MMR re-ranking (pcr_recommend_diverse): what the greedy selection costs next to the scoring sweep of the same call.

For each shape (ml1m 6 040 x 3 706, k = 100; Netflix 480 189 x 17 770, k = 100), fp32 and fp64, (topk, pool) = (10, 100) and
(100, 1024): a solver over a generated set of 20 training ratings per user on average, factors from initial(); after one warm-up
call, --steps calls of recommend_diverse(theta = 0.5), each timed by the solver's device events: recommend/rerank (the row norms,
the merge and the selection) next to recommend/score of the same call.  Both kernel forms are timed where both apply
(pcr_tune "rerank_lds" 0 = streaming, 1 = the pool's rows staged in LDS).  Prints one JSON line per case with the medians over
the calls (ms), the ratio, and the rows of V the selection reads per second (topk x pool x users rows of ld values).

    python tools/exp_rerank.py [--steps 5] [--shapes ml1m,netflix] [--cases 10:100,100:1024] [--dtypes f32,f64]
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
SLOTS = ("recommend/score", "recommend/rerank")


def lds_form_fits(pool, k, size):
    """mmr_wave_lds(pool, ld, 1) of pcr_topk.h within a workgroup's 160 KiB: the LDS form exists for this case."""
    ld = (k + 3) & ~3
    per = 16 // size
    stride = ((ld // per) | 1) * per
    return ((pool * stride * size + pool * (8 + size + 4) + 15) & ~15) <= 160 * 1024


def timed(s, call, steps):
    """Median over `steps` calls of each slot's device time per call (ms)."""
    call()                                           # warm-up (code object, allocation)
    s.profile(True)
    per = {n: [] for n in SLOTS}
    for _ in range(steps):
        s.profile_reset()
        call()
        for n in SLOTS:
            per[n].append(s.profile_get(n)[0])
    s.profile(False)
    return {n: float(np.median(v)) for n, v in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--shapes", default="ml1m,netflix")
    ap.add_argument("--cases", default="10:100,100:1024")
    ap.add_argument("--dtypes", default="f32,f64")
    a = ap.parse_args()
    cases = [tuple(int(x) for x in c.split(":")) for c in a.cases.split(",")]
    for name in a.shapes.split(","):
        d1, d2, k = SHAPES[name]
        R = synth.generate_fast("netflix", d1=d1, d2=d2, nnz=20 * d1)
        ds = pcr.Dataset.from_ratings(R)
        for dt in a.dtypes.split(","):
            prec, size = (pcr.PCR_F32, 4) if dt == "f32" else (pcr.PCR_F64, 8)
            s = pcr.Solver(ds, pcr.Parameter(k=k, precision=prec, do_predict=0, verbose=0))
            s.set_factors(pcr.initial(d1, k), pcr.initial(d2, k))
            for topk, pool in cases:
                for form in (0, 1):
                    if form and not lds_form_fits(pool, k, size):
                        continue
                    with pcr.tuned(rerank_lds=form):
                        t = timed(s, lambda: s.recommend_diverse(topk, pool=pool, theta=0.5), a.steps)
                    rr, sc = t["recommend/rerank"], t["recommend/score"]
                    print(json.dumps(dict(shape=name, d1=d1, d2=d2, k=k, dtype=dt, topk=topk, pool=pool, form="lds" if form else "stream",
                                          score_ms=round(sc, 3), rerank_ms=round(rr, 3), rerank_over_score=round(rr / sc, 3) if sc > 0 else None,
                                          grows_per_s=round(d1 * topk * pool / (rr * 1e-3) / 1e9, 2) if rr > 0 else None)), flush=True)
            s.close()


if __name__ == "__main__":
    main()
