"""Squared-loss explanations (pcr_explain_ridge): what `explain/ridge` costs for every user of an ml1m-shaped CCDR1 model, with
`explain/contrib` of pcr_explain at the same shape beside it as context.

The ml1m-shaped synthetic set (6 040 users, 939 809 ratings), k = 100, L = 10, E = 5, fp32 by default.  A CCDR1 solver after two
iterations runs Solver.explain_ridge on its own top-10 lists; a PrimalCR++ solver after two iterations runs Solver.explain on
its own.  After one warm-up call, --rounds rounds of --reps calls, every launch timed by the solver's device events (profile
period 1).  Prints one JSON line per entry: the mean ms per call of each round and the median over the rounds.

    python tools/exp_explain_ridge.py [--rounds 5] [--reps 20] [--dtype f32]
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


def measure(s, slot, call, rounds, reps):
    call()                                                                # warm-up
    per_round = []
    for _ in range(rounds):
        s.profile_reset()
        for _ in range(reps):
            call()
        s.sync()
        ms, cnt = s.profile_get(slot)
        per_round.append(ms / max(cnt, 1) * (cnt / reps))
    return per_round


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--dtype", default="f32")
    a = ap.parse_args()
    R = synth.generate("ml1m")
    ds = pcr.Dataset.from_ratings(R)
    k, L, E = 100, 10, 5
    prec = pcr.PCR_F32 if a.dtype == "f32" else pcr.PCR_F64
    nnz = int(ds.csr(0)[0][-1])
    cases = (("explain/ridge", pcr.PCR_SOLVER_CCDR1, 0.05, lambda s, lists: s.explain_ridge(lists, top=E)),
             ("explain/ridge", pcr.PCR_SOLVER_CCDR1, 0.05, lambda s, lists: s.explain_ridge(lists, top=E, nonneg=True)),
             ("explain/contrib", pcr.PCR_SOLVER_PCRPP, 25.0, lambda s, lists: s.explain(lists, top=E)))
    for n, (slot, solver, lam, fn) in enumerate(cases):
        s = pcr.Solver(ds, pcr.Parameter(k=k, precision=prec, solver_type=solver, **{"lambda": lam}))
        if solver == pcr.PCR_SOLVER_CCDR1:
            s.set_factors(pcr.initial_col(R.d1, k), None)
        else:
            s.set_factors(pcr.initial(R.d1, k), pcr.initial(R.d2, k))
        s.iterate(2)
        lists, _ = s.recommend(topk=L)
        s.profile(True)
        r = measure(s, slot, lambda: fn(s, lists), a.rounds, a.reps)
        print(json.dumps({"slot": slot, "nonneg": n == 1, "dtype": a.dtype, "users": int(R.d1), "ratings": nnz, "k": k, "L": L, "E": E, "reps": a.reps,
                          "ms_per_call": {"rounds": [round(x, 4) for x in r], "median": round(float(np.median(r)), 4)}}), flush=True)
        s.close()


if __name__ == "__main__":
    main()
