"""Filtered recommendation (pcr_recommend_filtered): what candidate lists and an allow set cost.

Netflix-shaped catalogue (17 770 items, k = 100, fp32), --users users (default 100 000) with 20 training ratings each on
average, factors from initial(), exclusion on, K = 10.  After one warm-up of every call the rounds are interleaved: each round
runs every variant once, and the medians (and the extremes) over the rounds are reported.

  candidates   recommend(candidates=) for 100 000 users x 100 candidates and 10 000 users x 1 000 candidates: the profile slot
               recommend/candidates (device events) and the wall time of the call, against the only route without the entry:
               recommend(topk=1024) for the same users (slots recommend/score + recommend/merge and the wall time) plus a numpy
               filter of its lists on the host (wall time), which cannot promise K results.
  allow        with --parent LIB (a libprimalcr.so built from the commit before the entry): recommend/score of that build's
               recommend(), of this build's recommend() and of this build's recommend(allow = all ones), one solver per build in
               one process (api.use_library), alternating.  "parent_spread_ms" is max - min of the parent build's rounds.

Prints one JSON line per case.

    python tools/exp_filter.py [--rounds 5] [--users 100000] [--parent path/to/libprimalcr.so] [--skip-host-route]
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

D2, RANK, K = 17770, 100, 10


def stats(xs):
    xs = sorted(xs)
    return dict(median=round(xs[len(xs) // 2], 3), min=round(xs[0], 3), max=round(xs[-1], 3))


def slot_ms(s, names):
    return sum(s.profile_get(n)[0] for n in names if n in s.profile_all())


def timed(s, names, call):
    """(slot ms, wall ms) of one call."""
    s.profile_reset()
    t0 = time.perf_counter()
    out = call()
    wall = (time.perf_counter() - t0) * 1e3
    return slot_ms(s, names), wall, out


def host_filter(items, cptr, citem, users_chunk=2048):
    """The first K eligible entries of each row of items [n, 1024]: what a caller without the entry does with recommend(topk=1024)."""
    n = items.shape[0]
    out = np.full((n, K), -1, np.int32)
    for b0 in range(0, n, users_chunk):
        b1 = min(n, b0 + users_chunk)
        E = np.zeros((b1 - b0, D2 + 1), bool)
        rows = np.repeat(np.arange(b1 - b0), np.diff(cptr[b0:b1 + 1]))
        E[rows, citem[cptr[b0]:cptr[b1]]] = True
        keep = E[np.arange(b1 - b0)[:, None], items[b0:b1]]          # (padding -1 indexes the extra, never eligible, column)
        order = np.argsort(~keep, axis=1, kind="stable")[:, :K]
        got = np.take_along_axis(items[b0:b1], order, axis=1)
        got[~np.take_along_axis(keep, order, axis=1)] = -1
        out[b0:b1] = got
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--users", type=int, default=100000)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--skip-host-route", action="store_true")
    a = ap.parse_args()
    d1 = a.users
    R = synth.generate_fast("netflix", d1=d1, d2=D2, nnz=20 * d1)
    U0, V0 = pcr.initial(d1, RANK), pcr.initial(D2, RANK)
    rng = np.random.default_rng(1)

    def solver():
        s = pcr.Solver(pcr.Dataset.from_ratings(R), pcr.Parameter(k=RANK, precision=pcr.PCR_F32, do_predict=0, verbose=0))
        s.set_factors(U0, V0)
        s.profile(True)
        return s

    here = pcr.lib_path()
    new = solver()

    # ---- candidate lists
    for n, per in ((d1, 100), (max(1, d1 // 10), 1000)):
        users = rng.choice(d1, n, replace=False).astype(np.int32)
        cptr = np.arange(n + 1, dtype=np.int64) * per
        # distinct ids per row without n shuffles of the catalogue: an arithmetic progression mod D2 with a step coprime to it
        steps = np.array([x for x in range(1, D2) if np.gcd(x, D2) == 1])
        citem = ((rng.integers(0, D2, (n, 1)) + rng.choice(steps, (n, 1)) * np.arange(per, dtype=np.int64)[None, :]) % D2).astype(np.int32).ravel()
        cand = lambda: new.recommend(K, users=users, candidates=(cptr, citem))
        full = lambda: new.recommend(1024, users=users)
        cand()
        if not a.skip_host_route:
            full()
        c_slot, c_wall, f_slot, f_wall, h_wall, short = [], [], [], [], [], 0
        for _ in range(a.rounds):
            x, y, got = timed(new, ("recommend/candidates",), cand)
            c_slot.append(x); c_wall.append(y)
            if a.skip_host_route:
                continue
            x, y, lists = timed(new, ("recommend/score", "recommend/merge"), full)
            f_slot.append(x); f_wall.append(y)
            t0 = time.perf_counter()
            flt = host_filter(lists[0], cptr, citem)
            h_wall.append((time.perf_counter() - t0) * 1e3)
            short = int(((flt >= 0).sum(axis=1) < (got[0] >= 0).sum(axis=1)).sum())
            same = int((flt == got[0]).all(axis=1).sum())
        rec = dict(case="candidates", users=n, per_user=per, K=K, candidates_slot_ms=stats(c_slot), candidates_wall_ms=stats(c_wall))
        if not a.skip_host_route:
            rec.update(top1024_slots_ms=stats(f_slot), top1024_wall_ms=stats(f_wall), host_filter_wall_ms=stats(h_wall),
                       host_route_rows_short_of_the_entry=short, host_route_rows_equal=same)
        print(json.dumps(rec), flush=True)

    # ---- allow set against the parent build's sweep
    if a.parent:
        ones = np.ones(D2, bool)
        pcr.use_library(os.path.abspath(a.parent))
        old = solver()
        variants = {"parent": (a.parent, old, lambda: old.recommend(K)), "new_no_filter": (here, new, lambda: new.recommend(K)),
                    "new_allow_ones": (here, new, lambda: new.recommend(K, allow=ones))}
        ms = {name: [] for name in variants}
        ref = None
        for rnd in range(a.rounds + 1):                               # (round 0 warms every variant up)
            for name, (path, s, call) in variants.items():
                pcr.use_library(os.path.abspath(path))
                x, _, out = timed(s, ("recommend/score",), call)
                if rnd:
                    ms[name].append(x)
                ref = out if ref is None else ref
                assert np.array_equal(out[0], ref[0]) and np.array_equal(out[1].view(np.int64), ref[1].view(np.int64)), name
        rec = dict(case="allow", users=d1, K=K, lists_bitwise_equal=True, **{name + "_score_ms": stats(v) for name, v in ms.items()})
        rec["parent_spread_ms"] = round(max(ms["parent"]) - min(ms["parent"]), 3)
        rec["allow_minus_parent_median_ms"] = round(stats(ms["new_allow_ones"])["median"] - stats(ms["parent"])["median"], 3)
        print(json.dumps(rec), flush=True)
        pcr.use_library(os.path.abspath(a.parent))
        old.close()
    pcr.use_library(here)
    new.close()


if __name__ == "__main__":
    main()
