"""Explanations (pcr_explain): what `explain/contrib` costs next to `recommend/score + recommend/merge` for the same users, and
where its time goes.

The ml1m-shaped synthetic set (6 040 users, 939 809 ratings), PrimalCR++ k = 100 after five iterations, fp32 by default, every
user.  After one warm-up call of each entry, --rounds rounds of --reps alternating calls of Solver.recommend(topk = L) and
Solver.explain(lists, top = E); every launch is timed by the solver's device events (profile period 1).  Prints one JSON line per
case: the mean ms per call of each round (their spread is the run-to-run noise inside one process) and the median over the rounds.
Cases: the headline (L = 10, E = 5); the same with E = 1 and with L = 1 (what the top-E merge and the tile cost); and the headline
restricted to the users of each workgroup form (<= 64 ratings, 65 .. 2048, beyond), which are one launch each.

    python tools/exp_explain.py [--rounds 5] [--reps 40] [--dtype f32]
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

SLOTS = ("explain/contrib", "recommend/score", "recommend/merge")


def measure(s, users, L, E, rounds, reps):
    lists, _ = s.recommend(topk=L, users=users)
    s.explain(lists, users=users, top=E)                                  # warm-up of every form the case uses
    per_round = {n: [] for n in SLOTS}
    for _ in range(rounds):
        s.profile_reset()
        for _ in range(reps):
            s.recommend(topk=L, users=users)
            s.explain(lists, users=users, top=E)
        s.sync()
        for n in SLOTS:
            ms, cnt = s.profile_get(n)
            per_round[n].append(ms / max(cnt, 1) * (cnt / reps))          # ms per call (a call may be several timed launch groups)
    return per_round


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--dtype", default="f32")
    a = ap.parse_args()
    R = synth.generate("ml1m")
    ds = pcr.Dataset.from_ratings(R)
    k = 100
    s = pcr.Solver(ds, pcr.Parameter(k=k, precision=pcr.PCR_F32 if a.dtype == "f32" else pcr.PCR_F64, solver_type=2, **{"lambda": 25.0}))
    s.set_factors(pcr.initial(R.d1, k), pcr.initial(R.d2, k))
    s.iterate(5)
    s.profile(True)
    length = np.diff(ds.csr(0)[0])
    wave, lds = pcr.foldin_boundaries()
    everyone = np.arange(R.d1, dtype=np.int32)
    cases = [("all users, L=10 E=5", everyone, 10, 5), ("all users, L=10 E=1", everyone, 10, 1), ("all users, L=1 E=5", everyone, 1, 5),
             (f"users of <= {wave} ratings, L=10 E=5", everyone[length <= wave], 10, 5),
             (f"users of {wave + 1} .. {lds} ratings, L=10 E=5", everyone[(length > wave) & (length <= lds)], 10, 5),
             (f"users beyond {lds} ratings, L=10 E=5", everyone[length > lds], 10, 5)]
    for name, users, L, E in cases:
        if users.shape[0] == 0:
            continue
        r = measure(s, users, L, E, a.rounds, a.reps)
        print(json.dumps({"case": name, "dtype": a.dtype, "users": int(users.shape[0]), "ratings": int(length[users].sum()), "reps": a.reps,
                          "ms_per_call": {n: {"rounds": [round(x, 4) for x in v], "median": round(float(np.median(v)), 4)} for n, v in r.items()}}))


if __name__ == "__main__":
    main()
