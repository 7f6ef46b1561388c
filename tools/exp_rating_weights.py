#!/usr/bin/env python3
"""What per-rating confidence weights (Solver.set_rating_weights) cost CCDR1 per outer iteration, and
whether the unweighted kernels are where an earlier build left them.

The ml1m-shaped synthetic set (6040 x 3952, 939 809 ratings), k = 10, lambda = 0.05, five inner iterations, from initial_col:
one warm-up training, then a timed one of --steps outer iterations (pcr_iter_stats' device clock), in fp32 and fp64, for the arms
  plain      no weights: k_ccd_sweep / k_ccd_resid / k_ccd_init
  weighted   rating_weights_popularity(0.5): the _w kernels (one more value of the residual's type per rating and sweep)
Every repeat is a fresh process (a library can be chosen only before it is loaded).  With --other-lib the repeats alternate
between that library (an earlier build: plain only) and this tree's, so that both see the same machine state.  --profile adds one
more process that reports the "ccd/..." profiler slots of both arms.  One JSON line.
Usage: python tools/exp_rating_weights.py [--repeats 5] [--steps 5] [--other-lib path/libprimalcr.so] [--profile]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K, LAM = 10, 0.05


def child(a):
    import primalcr_amd as pcr
    from primalcr_amd import synth
    if a.lib:
        pcr.use_library(a.lib)
    R = synth.generate("ml1m")
    ds = pcr.Dataset.from_ratings(R)
    can_weight = hasattr(pcr.lib(), "pcr_solver_set_rating_weights")
    w = pcr.rating_weights_popularity(ds, 0.5) if can_weight else None
    U0 = pcr.initial_col(R.d1, K)
    out = {"weighted_arm": can_weight}
    for pname, prec in (("f32", pcr.PCR_F32), ("f64", pcr.PCR_F64)):
        out[pname] = {}
        for arm in ("plain", "weighted") if can_weight else ("plain",):
            p = pcr.Parameter(solver_type=pcr.PCR_SOLVER_CCDR1, k=K, precision=prec, maxiter=a.steps, do_predict=0, verbose=0, **{"lambda": LAM})
            s = pcr.Solver(ds, p)
            if arm == "weighted":
                s.set_rating_weights(w)
            s.set_factors(U0, None)
            s.train()                                                 # warm-up
            s.set_factors(U0, None)
            if a.profile:
                s.profile(True)
            recs, _ = s.train()
            res = {"s_per_outer": recs[a.steps]["seconds"] / a.steps, "inner": int(recs[a.steps]["cg_v"]), "obj": recs[a.steps]["obj"]}
            if a.profile:
                res["slots_ms_launches"] = {n: [round(v[0], 4), v[1]] for n, v in s.profile_all().items() if n.startswith("ccd/")}
            s.close()
            out[pname][arm] = res
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)

    def run(lib, profile=False):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--steps", str(a.steps)] + (["--lib", lib] if lib else []) + (["--profile"] if profile else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
        if r.returncode != 0:                                         # nothing more is started after a failure
            sys.exit(f"{' '.join(cmd)} left with {r.returncode}:\n{r.stderr[-2000:]}")
        return json.loads(r.stdout.strip().splitlines()[-1])
    runs = {"other": [], "this": []}
    for _ in range(a.repeats):
        if a.other_lib:
            runs["other"].append(run(a.other_lib))
        runs["this"].append(run(None))
    out = {"shape": "ml1m", "k": K, "lambda": LAM, "steps": a.steps, "repeats": a.repeats}
    for prec, bytes_ratio in (("f32", (4 + 4 + 8 + 4) / (4 + 4 + 8)), ("f64", (4 + 8 + 8 + 8) / (4 + 8 + 8))):
        o = {}
        for who in ("other", "this"):
            for arm in ("plain", "weighted"):
                t = [r[prec][arm]["s_per_outer"] for r in runs[who] if arm in r[prec]]
                if t:
                    o[f"{who}/{arm}"] = {"ms_per_outer": [round(1e3 * x, 4) for x in t], "median": round(1e3 * float(np.median(t)), 4),
                                         "spread": round(1e3 * (max(t) - min(t)), 4), "inner": runs[who][0][prec][arm]["inner"]}
        if "other/plain" in o:
            o["plain_within_other_spread"] = abs(o["this/plain"]["median"] - o["other/plain"]["median"]) <= o["other/plain"]["spread"]
        if "this/weighted" in o:
            o["weighted_over_plain"] = round(o["this/weighted"]["median"] / o["this/plain"]["median"], 4)
            o["sweep_bytes_ratio"] = bytes_ratio                      # per rating: index + residual + gathered fp64 x, + the weight
        out[prec] = o
    if a.profile:
        p = run(None, profile=True)
        out["profile"] = {prec: {arm: p[prec][arm]["slots_ms_launches"] for arm in p[prec]} for prec in ("f32", "f64")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
