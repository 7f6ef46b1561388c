#!/usr/bin/env python3
"""What per-user loss weights (Solver.set_user_weights) cost per outer iteration on the bench shape.

The ml1m-shaped synthetic set of bench.py (6040 x 3952, 939 809 ratings, k = 100, lambda = 5000), from the reference's initial
factors: --warmup iterations, then --steps timed ones (pcr_iterate's device clock), for two arms interleaved round by round
  plain      no weights: the unweighted kernel symbols
  pairs      PCR_WEIGHT_PAIRS: the WT instantiations of the sweeps and of k_ustep, weighted sums in k_obj3
in fp32 and fp64.  The two arms solve DIFFERENT problems (the weighted one spreads the loss over all users), so their inner
iteration counts differ; the counts are printed beside the times.  One JSON line.
Usage: python tools/exp_user_weights.py [--rounds 3] [--steps 20] [--warmup 5]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import primalcr_amd as pcr  # noqa: E402
from primalcr_amd import synth  # noqa: E402

K, LAM = 100, 5000.0


def arm(ds, d1, d2, prec, w, warmup, steps):
    s = pcr.Solver(ds, pcr.Parameter(k=K, precision=prec, **{"lambda": LAM}))
    s.set_factors(pcr.initial(d1, K), pcr.initial(d2, K))
    if w is not None:
        s.set_user_weights(w)
    s.iterate(warmup)
    recs = s.iterate(steps)
    s.close()
    inner = {k: int(sum(r[k] for r in recs)) for k in ("cg_v", "ls_v", "cg_u", "ls_u")}
    return 1e3 * recs[-1]["seconds"] / steps, inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    R = synth.generate("ml1m")
    ds = pcr.Dataset.from_ratings(R)
    w = pcr.user_weights(ds, pcr.PCR_WEIGHT_PAIRS)
    out = {"shape": "ml1m", "k": K, "lambda": LAM, "steps": a.steps, "warmup": a.warmup, "weights": {"min": float(w.min()), "max": float(w.max())}}
    for pname, prec in (("f32", pcr.PCR_F32), ("f64", pcr.PCR_F64)):
        ms = {"plain": [], "pairs": []}
        inner = {}
        for _ in range(a.rounds):
            for name, ww in (("plain", None), ("pairs", w)):
                t, inner[name] = arm(ds, R.d1, R.d2, prec, ww, a.warmup, a.steps)
                ms[name].append(t)
        out[pname] = {n: {"ms_per_step": [round(x, 4) for x in ms[n]], "median": round(float(np.median(ms[n])), 4), "inner": inner[n]} for n in ms}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
