#!/usr/bin/env python3
"""What implicit feedback (Solver.set_implicit) costs CCDR1 per outer iteration, and whether the explicit
kernels are where an earlier build left them.

The ml1m-shaped synthetic set (6040 x 3952, 939 809 ratings), k = 100, lambda = 0.05, five inner iterations, from initial_col:
one warm-up training, then a timed one of --steps outer iterations (pcr_iter_stats' device clock), in fp32 and fp64, for the arms
  explicit   k_ccd_sweep / k_ccd_resid / k_ccd_init                                    (3 T + 3 launches per rank)
  implicit   set_implicit(0.3): k_ccd_gramcol / k_ccd_gramred / k_ccd_sweep_i / ...    (7 T + 5 launches per rank)
Every repeat is a fresh process (a library can be chosen only before it is loaded).  With --other-lib the repeats alternate
between that library (an earlier build: explicit only) and this tree's, so that both see the same machine state; the scatter of the
earlier build is its max - min over the repeats.  --profile adds one more process that reports the "ccd/..." profiler slots of both
arms.  One JSON line.
Usage: python tools/exp_implicit.py [--repeats 3] [--steps 3] [--other-lib path/libprimalcr.so] [--profile]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K, LAM, ALPHA = 100, 0.05, 0.3


def child(a):
    import primalcr_amd as pcr
    from primalcr_amd import synth
    if a.lib:
        pcr.use_library(a.lib)
    R = synth.generate("ml1m")
    ds = pcr.Dataset.from_ratings(R)
    can = hasattr(pcr.lib(), "pcr_solver_set_implicit")
    U0 = pcr.initial_col(R.d1, K)
    out = {"implicit_arm": can}
    for pname, prec in (("f32", pcr.PCR_F32), ("f64", pcr.PCR_F64)):
        out[pname] = {}
        for arm in ("explicit", "implicit") if can else ("explicit",):
            p = pcr.Parameter(solver_type=pcr.PCR_SOLVER_CCDR1, k=K, precision=prec, maxiter=a.steps, do_predict=0, verbose=0, **{"lambda": LAM})
            s = pcr.Solver(ds, p)
            if arm == "implicit":
                s.set_implicit(ALPHA)
            s.set_factors(U0, None)
            s.train()                                                 # warm-up
            s.set_factors(U0, None)
            if a.profile:
                s.profile(True)
            recs, _ = s.train()
            res = {"s_per_outer": recs[a.steps]["seconds"] / a.steps, "inner": int(recs[a.steps]["cg_v"]), "ranks": int(recs[a.steps]["cg_u"]),
                   "obj": recs[a.steps]["obj"]}
            if a.profile:
                res["slots_ms_launches"] = {n: [round(v[0], 4), v[1]] for n, v in s.profile_all().items() if n.startswith("ccd/")}
            s.close()
            out[pname][arm] = res
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
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
    out = {"shape": "ml1m", "k": K, "lambda": LAM, "alpha": ALPHA, "steps": a.steps, "repeats": a.repeats}
    for prec in ("f32", "f64"):
        o = {}
        for who in ("other", "this"):
            for arm in ("explicit", "implicit"):
                t = [r[prec][arm]["s_per_outer"] for r in runs[who] if arm in r[prec]]
                if t:
                    o[f"{who}/{arm}"] = {"ms_per_outer": [round(1e3 * x, 4) for x in t], "median": round(1e3 * float(np.median(t)), 4),
                                         "spread": round(1e3 * (max(t) - min(t)), 4), "inner": runs[who][0][prec][arm]["inner"],
                                         "ranks": runs[who][0][prec][arm]["ranks"]}
        if "other/explicit" in o:
            o["explicit_within_other_spread"] = abs(o["this/explicit"]["median"] - o["other/explicit"]["median"]) <= o["other/explicit"]["spread"]
        if "this/implicit" in o:
            o["implicit_over_explicit"] = round(o["this/implicit"]["median"] / o["this/explicit"]["median"], 4)
        out[prec] = o
    if a.profile:
        p = run(None, profile=True)
        out["profile"] = {prec: {arm: p[prec][arm]["slots_ms_launches"] for arm in p[prec]} for prec in ("f32", "f64")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
