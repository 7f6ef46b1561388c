"""Filtered evaluation (pcr_evaluate_topn_filtered, pcr_evaluate_ranks_filtered): what the sampled-candidate
protocol costs on the device, beside the route it replaces, and what the allow operand costs the unfiltered rank sweep.

Netflix-shaped catalogue (17 770 items, k = 100, fp32), --users users (default 100 000) with 20 training ratings on average and
one held-out rating each, factors from initial(), exclusion on; candidate rows from sample_negatives(n_neg = 99): 100 candidates
per user.  After one warm-up of every call the rounds are interleaved: each round runs every variant once, and the medians (and
the extremes) over the rounds are reported.

  candidates   Solver.evaluate_topn(cutoffs = (10,), candidates=) -- slots recommend/candidates_metrics, recommend/metrics -- and
               Solver.evaluate_ranks(candidates=) -- slots ranks/relscore, ranks/candidates, ranks/finish, each on its own -- with
               their wall times, beside the route they replace: Solver.recommend(10, candidates=) (slot recommend/candidates, wall) followed
               by evaluate_lists() on the returned lists (a model entry: wall time only, it has no profile slots).  list_bytes: what
               that route copies for the lists alone (items and scores device -> host, items host -> device); the new entries copy
               none.  The old route has no rank metrics at all.
  ranks_count  with --parent LIB (a libprimalcr.so built from the commit before the entries): ranks/count of that build's
               evaluate_ranks(), of this build's evaluate_ranks() (NULL allow pointer) and of this build's evaluate_ranks(allow =
               all ones), one solver per build in one process (api.use_library), alternating; results compared bitwise.
               "parent_spread_ms" is max - min of the parent build's rounds.

Prints one JSON line per case.

    python tools/exp_filtered_eval.py [--rounds 5] [--users 100000] [--parent path/to/libprimalcr.so]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import primalcr_amd as pcr  # noqa: E402
from primalcr_amd import synth  # noqa: E402

D2, RANK, K, NEG = 17770, 100, 10, 99


def stats(xs):
    xs = sorted(xs)
    return dict(median=round(xs[len(xs) // 2], 3), min=round(xs[0], 3), max=round(xs[-1], 3))


def timed(s, names, call):
    """({slot: ms} of the named slots, wall ms, result) of one call."""
    s.profile_reset()
    t0 = time.perf_counter()
    out = call()
    wall = (time.perf_counter() - t0) * 1e3
    have = s.profile_all()
    return {n: have[n][0] for n in names if n in have}, wall, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--users", type=int, default=100000)
    ap.add_argument("--parent", default=None)
    a = ap.parse_args()
    d1 = a.users
    R = synth.generate_fast("netflix", d1=d1, d2=D2, nnz=20 * d1, n_test=1)
    U0, V0 = pcr.initial(d1, RANK), pcr.initial(D2, RANK)

    def solver():
        ds = pcr.Dataset.from_ratings(R)
        s = pcr.Solver(ds, pcr.Parameter(k=RANK, precision=pcr.PCR_F32, do_predict=0, verbose=0))
        s.set_factors(U0, V0)
        s.profile(True)
        return s, ds

    here = pcr.lib_path()
    new, ds = solver()
    test = ds.csr(1)
    t0 = time.perf_counter()
    cand = pcr.sample_negatives(D2, ds, ds, n_neg=NEG, seed=1)
    sample_ms = (time.perf_counter() - t0) * 1e3

    # ---- the sampled-candidate protocol
    variants = {
        "topn": (("recommend/candidates_metrics", "recommend/metrics"), lambda: new.evaluate_topn((K,), candidates=cand)),
        "ranks": (("ranks/relscore", "ranks/candidates", "ranks/finish"), lambda: new.evaluate_ranks(candidates=cand)),
        "old_recommend": (("recommend/candidates",), lambda: new.recommend(K, candidates=cand)),
    }
    slot = {n: {x: [] for x in names} for n, (names, _) in variants.items()}
    wall = {n: [] for n in variants}
    lists_wall, out = [], {}
    for rnd in range(a.rounds + 1):                                   # (round 0 warms every variant up)
        for name, (names, call) in variants.items():
            x, y, out[name] = timed(new, names, call)
            if rnd:
                wall[name].append(y)
                for k_, v_ in x.items():
                    slot[name][k_].append(v_)
        t0 = time.perf_counter()
        old = pcr.evaluate_lists(out["old_recommend"][0], V0, d1=d1, test=test, cutoffs=(K,), dtype=pcr.PCR_F32)
        if rnd:
            lists_wall.append((time.perf_counter() - t0) * 1e3)
    for f in ("users", "hits"):
        assert old["topn"][0][f] == out["topn"][0][f], (f, old["topn"][0], out["topn"][0])
    rec = dict(case="candidates", users=d1, per_user=NEG + 1, K=K, candidate_items=int(cand[0][-1]), sample_negatives_wall_ms=round(sample_ms, 1),
               counted_users=out["topn"][0]["users"], hit_rate=out["topn"][0]["hit_rate"], auc=out["ranks"]["auc"],
               old_route_list_bytes=dict(device_to_host=d1 * K * 12, host_to_device=d1 * K * 4), new_route_list_bytes=0)
    for name in variants:
        rec[name + "_slots_ms"] = {k_: stats(v_) for k_, v_ in slot[name].items() if v_}; rec[name + "_wall_ms"] = stats(wall[name])
    rec["old_evaluate_lists_wall_ms"] = stats(lists_wall)
    print(json.dumps(rec), flush=True)

    # ---- the allow operand of the counting sweep against the parent build
    if a.parent:
        ones = np.ones(D2, bool)
        pcr.use_library(os.path.abspath(a.parent))
        oldb, _ = solver()
        full = dict(per_user=True, ranks=True)
        arms = {"parent": (a.parent, oldb, lambda: oldb.evaluate_ranks(**full)), "new_no_filter": (here, new, lambda: new.evaluate_ranks(**full)),
                "new_allow_ones": (here, new, lambda: new.evaluate_ranks(allow=ones, **full))}
        ms = {name: [] for name in arms}
        ref = None
        for rnd in range(a.rounds + 1):
            for name, (path, s, call) in arms.items():
                pcr.use_library(os.path.abspath(path))
                x, _, got = timed(s, ("ranks/count",), call)
                if rnd:
                    ms[name].append(x["ranks/count"])
                ref = got if ref is None else ref
                assert got[0] == ref[0] and np.array_equal(got[1].view(np.int64), ref[1].view(np.int64)) and np.array_equal(got[2], ref[2]), name
        rec = dict(case="ranks_count", users=d1, results_bitwise_equal=True, **{name + "_count_ms": stats(v) for name, v in ms.items()})
        rec["parent_spread_ms"] = round(max(ms["parent"]) - min(ms["parent"]), 3)
        rec["new_minus_parent_median_ms"] = round(stats(ms["new_no_filter"])["median"] - stats(ms["parent"])["median"], 3)
        print(json.dumps(rec), flush=True)
        pcr.use_library(os.path.abspath(a.parent))
        oldb.close()
    pcr.use_library(here)
    new.close()


if __name__ == "__main__":
    main()
