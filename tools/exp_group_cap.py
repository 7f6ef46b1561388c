"""Group-capped lists (pcr_recommend_capped): what the merge with the selection fused in costs next to the scoring sweep of the
same call, and next to the plain merge (k_rec_merge) of pcr_recommend with K = pool in the same process.

The ml1m-shaped set (6 040 x 3 706, k = 100; 20 training ratings per user on average, factors from initial()), fp32 and fp64,
topk = 10, pool = 100 and 1024.  Two group tables: "genres" (18 groups drawn uniformly, cap 2: the walk ends early for most
users) and "one" (a single group, cap 1: every user's walk covers the whole pool, the direct count's worst case).  After one
warm-up call of each entry, --steps rounds alternate recommend_capped() and recommend(K = pool); each call is timed by the
solver's device events.  Prints one JSON line per case with the medians (and the extremes) over the rounds, in ms.

    python tools/exp_group_cap.py [--steps 20] [--pools 100,1024] [--dtypes f32,f64]
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

D1, D2, K, TOPK = 6040, 3706, 100, 10


def slots(s, call, names):
    s.profile_reset()
    call()
    return [s.profile_get(n)[0] for n in names]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--pools", default="100,1024")
    ap.add_argument("--dtypes", default="f32,f64")
    a = ap.parse_args()
    R = synth.generate_fast("netflix", d1=D1, d2=D2, nnz=20 * D1)
    ds = pcr.Dataset.from_ratings(R)
    rng = np.random.default_rng(3)
    tables = {"genres": (rng.integers(0, 18, D2).astype(np.int32), 2), "one": (np.zeros(D2, np.int32), 1)}
    for dt in a.dtypes.split(","):
        prec = pcr.PCR_F32 if dt == "f32" else pcr.PCR_F64
        s = pcr.Solver(ds, pcr.Parameter(k=K, precision=prec, do_predict=0, verbose=0))
        s.set_factors(pcr.initial(D1, K), pcr.initial(D2, K))
        for pool in (int(x) for x in a.pools.split(",")):
            for name, (g, cap) in tables.items():
                capped = lambda: s.recommend_capped(TOPK, g, cap, pool=pool)
                plain = lambda: s.recommend(pool)
                st = capped()[3]
                plain()                                      # warm-up of both entries (code objects, allocation)
                s.profile(True)
                t = {"cap": [], "cap_score": [], "merge": [], "merge_score": []}
                for _ in range(a.steps):
                    c, cs = slots(s, capped, ("recommend/cap", "recommend/score"))
                    m, ms = slots(s, plain, ("recommend/merge", "recommend/score"))
                    t["cap"].append(c); t["cap_score"].append(cs); t["merge"].append(m); t["merge_score"].append(ms)
                s.profile(False)
                med = {n: float(np.median(v)) for n, v in t.items()}
                print(json.dumps(dict(d1=D1, d2=D2, k=K, dtype=dt, topk=TOPK, pool=pool, groups=name, cap=cap, steps=a.steps,
                                      cap_ms=round(med["cap"], 4), score_ms=round(med["cap_score"], 4),
                                      plain_merge_ms=round(med["merge"], 4), plain_score_ms=round(med["merge_score"], 4),
                                      cap_min_max=[round(min(t["cap"]), 4), round(max(t["cap"]), 4)],
                                      merge_min_max=[round(min(t["merge"]), 4), round(max(t["merge"]), 4)],
                                      cap_over_score=round(med["cap"] / med["cap_score"], 3) if med["cap_score"] > 0 else None,
                                      exhausted=st["exhausted"], kept=st["kept"])), flush=True)
        s.close()


if __name__ == "__main__":
    main()
