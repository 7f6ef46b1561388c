"""Group-capped top-K lists (pcr_recommend_capped_model / pcr_recommend_capped, omp-pmf-recommend --groups --max-per-group,
Python recommend_capped()): the first topk entries of a user's `pool` best items that the rule "at most cap items of one group"
keeps, with one status byte per user.

group_cap_ref.py holds the reference: ref_capped() applies the contract of include/primalcr.h to the pool recommend() returns
with K = pool (that pool's exactness is held by test_recommend*.py), ref_capped_full() walks the whole eligible catalogue.
The selection is integer compares and copies, so everything is compared with == (items, status) and bitwise (scores).

Exact inputs: integer factors in [-2, 2] (scores are small integers, exact in f32 and fp64 in any summation order, and heavily
tied: every test below exercises the (score, id) order of the pool).  Every exact case carries three special exclusion rows:
user 0 keeps 30 eligible items (fewer than the pools of 63 and more), user 1 keeps 7 (fewer than topk = 10), user 2 keeps none.

CPU part: argument checks of both entries before any device is looked for, the PCR_ERR_UNSUPPORTED refusal of candidate rows, the
"no device" error, the wrappers' ValueErrors, the CLI's usage text and refusals, the header's [device] marks, a property test
of the reference itself (status-0 rows are the full-catalogue list, status-1 rows a prefix of it, counting kept entries only
gives the same lists) and the non-vacuity of every parametrised GPU case, asserted from the reference alone.
GPU part (-m gpu): pool and lane edges, group layouts and ranks, short and empty pools, the partial-list merge (four item splits;
rec_run has no split knob, the shape decides), two user batches, the contract's identities, the full-catalogue claim, an allow
set, independence of the other users, Gaussian factors, composition with evaluate_lists(), live solvers and the CLI.
"""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import BIN_DIR, ROOT
from group_cap_ref import CAP_EXACT, CAP_POOL_EXHAUSTED, ref_capped, ref_capped_full, stats_of, walk
from test_recommend import excl_mask, ref_topk
from test_recommend_grid import boundary_row, csr_of, int_factors, random_csr, rec_geometry, splits_of

RECOMMEND = os.path.join(BIN_DIR, "omp-pmf-recommend")
TRAIN = os.path.join(BIN_DIR, "omp-pmf-train")
ERR_ARG, ERR_DEVICE, ERR_UNSUPPORTED = -1, -4, -7
D1, D2 = 40, 300
KEEP = {0: 30, 1: 7, 2: 0}                    # eligible items of the three special users
CAPS = (1, 2, 5)
LAYOUTS = ("one", "three", "distinct", "negative", "mixed", "sparse")
POOLS = (1, 63, 64, 65, 128, 1024)


def run(cmd, cwd, timeout=600):
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=timeout)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def same_lists(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))


# ---------------------------------------------------------------------------------------------------------------- cases
@functools.lru_cache(maxsize=None)
def exact_case(seed, d1, d2, k):
    """(U, V, index, item): integer factors; users 0, 1, 2 keep KEEP[u] eligible items."""
    rng = np.random.default_rng(seed)
    U, V = int_factors(rng, d1, k), int_factors(rng, d2, k)
    special = {u: np.setdiff1d(np.arange(d2), rng.choice(d2, keep, replace=False)).astype(np.int32) for u, keep in KEEP.items()}
    index, item = random_csr(rng, d1, d2, special)
    return U, V, index, item


@functools.lru_cache(maxsize=None)
def layout(name, d2, seed=5):
    rng = np.random.default_rng(seed)
    if name == "one":
        g = np.zeros(d2, np.int64)
    elif name == "three":
        g = rng.integers(0, 3, d2)
    elif name == "distinct":
        g = rng.permutation(d2)
    elif name == "negative":
        g = -1 - rng.integers(0, 4, d2)
    elif name == "mixed":
        g = rng.choice([-1, -7, 0, 1, 2, 3, 4], d2)
    else:
        g = rng.choice([7, 2 ** 30, 123456789], d2)
    return g.astype(np.int32)


def is_identity(name, cap, pool):
    return name in ("distinct", "negative") or cap >= pool


def edge_case(pool):
    """test_pool_and_lane_edges' inputs and (topk, cap) sweep at one pool."""
    d2 = 1100 if pool == 1024 else D2
    return exact_case(20 + pool, D1, d2, 3), layout("three", d2), [(t, c) for t in sorted({1, min(10, pool), pool}) for c in CAPS]


def layout_case(name, k):
    """test_group_layouts_and_ranks' inputs and sweep: pool 64, topk 10, every cap."""
    return exact_case(40 + k, D1, D2, k), layout(name, D2), [(10, c) for c in CAPS]


@functools.lru_cache(maxsize=None)
def reference_pool(seed, d1, d2, k, pool):
    """ref_topk's pool of an exact case, from the scores alone (the device returns the same pool: test_recommend*.py)."""
    U, V, index, item = exact_case(seed, d1, d2, k)
    return ref_topk(U @ V.T, excl_mask(d1, d2, index, item), pool)


def vacuity_counts(seed, d1, d2, k, groups, pool, combos):
    """Over a case's sweep: (status-0 users whose list differs from the plain top-topk, status-1 users), from the reference."""
    pi, ps = reference_pool(seed, d1, d2, k, pool)
    changed = exhausted = 0
    for topk, cap in combos:
        it, _, st = ref_capped(pi, ps, groups, cap, topk)
        changed += int(((it != pi[:, :topk]).any(1) & (st == CAP_EXACT)).sum())
        exhausted += int((st == CAP_POOL_EXHAUSTED).sum())
    return changed, exhausted


def _model_call(U, V, index, item, users, topk, pool, group, cap, dtype=1, n=None, out=True, f=None, status=True, stats=True):
    """pcr_recommend_capped_model through ctypes, arrays as given (None = NULL); returns the status code."""
    import ctypes as C
    import primalcr_amd as pcr
    n = (len(users) if users is not None else U.shape[0]) if n is None else n
    items = np.empty((max(n, 1), max(topk, 1)), np.int32); scores = np.empty((max(n, 1), max(topk, 1)))
    st = np.empty(max(n, 1), np.uint8)
    cs = pcr.CapStats()
    ptr = lambda a: None if a is None else a.ctypes.data
    return pcr.lib().pcr_recommend_capped_model(ptr(U), U.shape[0], ptr(V), V.shape[0], U.shape[1], ptr(index), ptr(item), n, ptr(users),
                                                topk, pool, ptr(group), cap, dtype, None if f is None else C.byref(f),
                                                ptr(items) if out else None, ptr(scores) if out else None, ptr(st) if status else None,
                                                C.byref(cs) if stats else None, 0)


def _small():
    rng = np.random.default_rng(1)
    U, V = rng.standard_normal((20, 5)), rng.standard_normal((30, 5))
    index = np.array([0] + [2] * 20, np.int64)
    item = np.array([3, 7], np.int32)
    return U, V, index, item, np.arange(20, dtype=np.int32), (np.arange(30) % 4).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_model_entry_argument_checks():
    import primalcr_amd as pcr
    U, V, index, item, users, group = _small()

    def bad(*a, **kw):
        assert _model_call(*a, **kw) == ERR_ARG
        assert b"pcr_recommend_capped_model" in pcr.lib().pcr_last_error()

    bad(U, V, index, item, users, 5, 10, None, 2)
    bad(U, V, index, item, users, 5, 10, group, 0)
    bad(U, V, index, item, users, 5, 10, group, -3)
    bad(U, V, index, item, users, 0, 10, group, 2)
    bad(U, V, index, item, users, -1, 10, group, 2)
    bad(U, V, index, item, users, 5, 4, group, 2)
    bad(U, V, index, item, users, 5, 1025, group, 2)
    bad(U, V, index, item, users, 1025, 1025, group, 2)
    # every argument error of pcr_recommend_filtered_model
    bad(U, V, index, item, users, 5, 10, group, 2, dtype=5)
    bad(U, V, index, item, users, 5, 10, group, 2, out=False)
    bad(U, V, index, item, np.array([0, 20], np.int32), 5, 10, group, 2)
    bad(U, V, index, item, np.array([-1], np.int32), 5, 10, group, 2)
    bad(U, V, index, item, None, 5, 10, group, 2, n=21)
    bad(U, V, index, item, users, 5, 10, group, 2, n=-1)
    nm = index.copy(); nm[5] = 1
    bad(U, V, nm, item, users, 5, 10, group, 2)
    bad(U, V, index, np.array([3, 30], np.int32), users, 5, 10, group, 2)
    bad(U, V, index, None, users, 5, 10, group, 2)
    nz = index.copy(); nz[0] = 1
    bad(U, V, nz, item, users, 5, 10, group, 2)
    bad(U, V, index, item, users, 5, 10, group, 2, f=pcr.api.ItemFilter())           # a filter with nothing in it


def test_solver_entry_checks_its_solver_first():
    import primalcr_amd as pcr
    one = np.array([5], np.int32)
    group = np.zeros(8, np.int32)
    buf_i = np.empty(4, np.int32); buf_s = np.empty(4); st = np.empty(1, np.uint8)
    assert pcr.lib().pcr_recommend_capped(None, 1, one.ctypes.data, 2, 4, group.ctypes.data, 1, 0, None, buf_i.ctypes.data, buf_s.ctypes.data,
                                          st.ctypes.data, None) == ERR_ARG


def test_candidate_rows_are_unsupported():
    import primalcr_amd as pcr
    U, V, index, item, users, group = _small()
    cp = np.arange(21, dtype=np.int64); ci = np.zeros(20, np.int32)
    f = pcr.api.ItemFilter()
    f.cand_ptr = cp.ctypes.data; f.cand_item = ci.ctypes.data
    assert _model_call(U, V, index, item, users, 5, 10, group, 2, f=f) == ERR_UNSUPPORTED
    assert b"pcr_recommend_capped_model" in pcr.lib().pcr_last_error()
    allow = np.ones(30, np.uint8)
    f.allow = allow.ctypes.data                                                        # with an allow set next to them as well
    assert _model_call(U, V, index, item, users, 5, 10, group, 2, f=f) == ERR_UNSUPPORTED
    assert _model_call(U, V, index, item, users, 5, 4, group, 2, f=f) == ERR_ARG       # an argument error comes first


def test_model_entry_without_a_device_is_a_device_error():
    code = ("import sys, numpy as np; sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')\n"
            "import primalcr_amd as pcr\n"
            "from test_group_cap import _model_call, _small\n"
            "U, V, index, item, users, group = _small()\n"
            "f = pcr.api.ItemFilter(); allow = np.ones(30, np.uint8); f.allow = allow.ctypes.data\n"
            "print(_model_call(U, V, index, item, users, 2, 4, group, 1), _model_call(U, V, None, None, None, 2, 4, group, 1, dtype=0, f=f, "
            "status=False, stats=False))\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    assert [int(x) for x in out.stdout.strip().splitlines()[-1].split()] == [ERR_DEVICE] * 2


def test_python_wrappers_refuse_bad_arguments():
    import primalcr_amd as pcr
    rng = np.random.default_rng(2)
    U, V = rng.standard_normal((6, 3)), rng.standard_normal((9, 3))
    g = np.zeros(9, np.int32)
    for kw in (dict(topk=0, groups=g, cap=1), dict(topk=5, groups=g, cap=1, pool=4), dict(topk=5, groups=g, cap=1, pool=1025),
               dict(topk=2000, groups=g, cap=1), dict(topk=5, groups=g, cap=0), dict(topk=5, groups=g, cap=-1), dict(topk=5, groups=None, cap=1),
               dict(topk=5, groups=np.zeros((9, 1), np.int32), cap=1), dict(topk=5, groups=np.zeros(9), cap=1),
               dict(topk=5, groups=np.full(9, 2 ** 31, np.int64), cap=1)):
        with pytest.raises(ValueError):
            pcr.recommend_capped(U, V, **kw)
        with pytest.raises(ValueError):
            pcr.Solver.recommend_capped(None, **kw)                       # (checked before the solver is touched)
    with pytest.raises(ValueError):
        pcr.recommend_capped(U, V, 3, np.zeros(8, np.int32), 1)            # one id per item
    with pytest.raises(ValueError):
        pcr.recommend_capped(U, V, 3, g, 1, exclude=(np.zeros(7, np.int64), np.array([1], np.int32)))
    with pytest.raises(ValueError):
        pcr.recommend_capped(U, V, 3, g, 1, allow=np.ones(8, bool))
    from primalcr_amd.api import _cap_args
    assert _cap_args(10, None, g, 2, 9)[:2] == (10, 100) and _cap_args(200, None, g, 2, 9)[1] == 1024
    assert _cap_args(3, 7, [1, -2, 3], 2, 3)[2].dtype == np.int32
    assert pcr.recommend_capped is pcr.api.recommend_capped and "recommend_capped" in pcr.__all__
    assert (pcr.PCR_CAP_EXACT, pcr.PCR_CAP_POOL_EXHAUSTED) == (CAP_EXACT, CAP_POOL_EXHAUSTED) == (0, 1)
    assert [f[0] for f in pcr.CapStats._fields_] == ["users", "exact", "exhausted", "short_rows", "kept"]


def test_header_marks_both_entries_as_device():
    hdr = open(os.path.join(ROOT, "include", "primalcr.h")).read()
    for name in ("pcr_recommend_capped_model", "pcr_recommend_capped"):
        assert re.search(rf"\bint {name}\([^;]*;\s*/\* \[device\] \*/", hdr), name
    assert "#define PCR_CAP_EXACT          0" in hdr and "#define PCR_CAP_POOL_EXHAUSTED 1" in hdr
    assert re.search(r"typedef struct pcr_cap_stats \{\s*int64_t users, exact, exhausted, short_rows, kept;\s*\} pcr_cap_stats;", hdr)


def test_cli_usage_and_refusals(tmp_path):
    import primalcr_amd as pcr
    from primalcr_amd import synth
    r = run([RECOMMEND], tmp_path)
    assert r.returncode == 1 and r.stdout.startswith("Usage: omp-pmf-recommend [-K topk]")
    assert "--groups file --max-per-group q [--pool P] [--allow items_file] [-K topk]" in r.stdout and "--max-per-group q  " in r.stdout
    assert "capped users n exact n" in r.stdout
    R = synth.generate("tiny", seed=3)
    d = synth.write_dir(R, str(tmp_path / "data"))
    (tmp_path / "g.txt").write_text("0\n" * R.d2)
    missing = str(tmp_path / "missing.model")

    def refused(args, *words):
        r = run([RECOMMEND] + args + [missing, "out.txt"], tmp_path)
        assert r.returncode == 1 and "can't open" not in r.stderr, (args, r.stderr)       # refused before the model is read
        for w in words:
            assert w in r.stderr, (args, w, r.stderr)

    refused(["--groups", "g.txt"], "--groups", "--max-per-group", "go together")
    refused(["--max-per-group", "2"], "--groups", "--max-per-group", "go together")
    both = ["--groups", "g.txt", "--max-per-group", "2"]
    for extra in (["--eval", d], ["--diversity"], ["--mmr", "0.5"], ["--tradeoff", "0,0.5"], ["--eval", d, "--ranks"],
                  ["--fold-in", d, "-l", "1"], ["--fold-in-ridge", d, "-l", "1"], ["--fold-in-nnls", d, "-l", "1"],
                  ["--fold-in-items", "r.txt", "-x", d, "-l", "1"], ["--candidates", "c.txt"]):
        refused(both + extra, "--groups and --max-per-group do not go with")
    for v in ("0", "-1", "x", "", "1.5"):
        r = run([RECOMMEND, "--groups", "g.txt", "--max-per-group", v, missing, "out.txt"], tmp_path)
        assert r.returncode == 1 and "--max-per-group" in r.stderr and "can't open" not in r.stderr, v
    for flag in ("--groups", "--max-per-group"):
        r = run([RECOMMEND, flag], tmp_path)
        assert r.returncode == 1 and flag + " needs a value" in r.stderr and r.stdout.startswith("Usage: omp-pmf-recommend")
    refused(both + ["--pool", "5", "-K", "10"], "--pool")
    # --pool alone keeps its message
    r = run([RECOMMEND, "--pool", "50", missing, "out.txt"], tmp_path)
    assert r.returncode == 1 and r.stderr == "--pool goes with --mmr\n"
    # --pool goes with the cap: the model file is the first thing missing
    r = run([RECOMMEND] + both + ["--pool", "50", missing, "out.txt"], tmp_path)
    assert r.returncode == 1 and "can't open model file" in r.stderr
    rng = np.random.default_rng(2)
    pcr.model_save(str(tmp_path / "ok.model"), rng.standard_normal((R.d1, 4)), rng.standard_normal((R.d2, 4)))
    r = run([RECOMMEND] + both + ["ok.model"], tmp_path)                                   # the plain form's two positionals
    assert r.returncode == 1 and r.stdout.startswith("Usage: omp-pmf-recommend")
    for text, word in (("0\n" * (R.d2 - 1), "fewer lines"), ("0\n" * (R.d2 + 1), "more lines"), ("0\n" * (R.d2 - 1) + "x\n", "not a group id"),
                       ("0\n" * (R.d2 - 1) + "\n", "not a group id"), ("0\n" * (R.d2 - 1) + "3000000000\n", "not a group id")):
        (tmp_path / "bad.txt").write_text(text)
        r = run([RECOMMEND, "--groups", "bad.txt", "--max-per-group", "2", "ok.model", "out.txt"], tmp_path)
        assert r.returncode == 1 and word in r.stderr and "bad.txt" in r.stderr, (word, r.stderr)
    r = run([RECOMMEND, "--groups", "nofile.txt", "--max-per-group", "2", "ok.model", "out.txt"], tmp_path)
    assert r.returncode == 1 and "can't open groups file" in r.stderr


def test_reference_exactness_property():
    """On random tied integer scores: a status-0 row of ref_capped equals ref_capped_full's row, a status-1 row is a proper
    prefix of it, and counting kept entries only gives the same rows.  Both statuses must occur often."""
    rng = np.random.default_rng(11)
    seen = {CAP_EXACT: 0, CAP_POOL_EXHAUSTED: 0}
    for trial in range(600):
        d2 = int(rng.integers(1, 70))
        s = rng.integers(-3, 4, d2).astype(np.float64)
        elig = rng.random(d2) < rng.choice([0.2, 0.7, 1.0])
        kind = trial % 4
        g = (rng.integers(0, 1 + int(rng.integers(1, 6)), d2) if kind == 0 else rng.choice([-1, 0, 1, 2 ** 30], d2) if kind == 1
             else np.zeros(d2, np.int64) if kind == 2 else rng.permutation(d2)).astype(np.int32)
        cap = int(rng.integers(1, 5))
        pool = int(rng.integers(1, d2 + 6))
        topk = int(rng.integers(1, pool + 1))
        pi, ps = ref_topk(s[None, :], ~elig[None, :], pool)
        it, sc, st = ref_capped(pi, ps, g, cap, topk)
        it2, sc2, st2 = ref_capped(pi, ps, g, cap, topk, by_kept=True)
        assert np.array_equal(it, it2) and np.array_equal(bits(sc), bits(sc2)) and np.array_equal(st, st2), trial
        fi, fs = ref_capped_full(s, elig, g, cap, topk)
        L = int((it[0] >= 0).sum())
        assert np.all(it[0, L:] == -1) and np.all(np.isneginf(sc[0, L:])), trial
        if st[0] == CAP_EXACT:
            assert list(it[0, :L]) == fi and list(sc[0, :L]) == fs, trial
        else:
            assert L < topk and int(elig.sum()) >= pool and list(it[0, :L]) == fi[:L] and list(sc[0, :L]) == fs[:L], trial
        if L:
            assert it[0, 0] == pi[0, 0], trial                                       # the first kept entry is pool position 0
        assert stats_of(it, st) == dict(users=1, exact=int(st[0] == 0), exhausted=int(st[0] == 1), short_rows=int(L < topk), kept=L)
        seen[int(st[0])] += 1
    print("exact", seen[CAP_EXACT], "exhausted", seen[CAP_POOL_EXHAUSTED])
    assert seen[CAP_EXACT] >= 100 and seen[CAP_POOL_EXHAUSTED] >= 100


def test_parametrised_gpu_cases_are_not_vacuous():
    """From the reference alone: every parametrised GPU case that is not an identity has a status-0 user whose list differs from
    the plain top-topk, and the two designated exhausted cases (one group, three groups; k = 3) have status-1 users."""
    for pool in POOLS:
        (U, V, index, item), g, combos = edge_case(pool)
        changed, exhausted = vacuity_counts(20 + pool, D1, V.shape[0], 3, g, pool, combos)
        print("pool", pool, "changed", changed, "exhausted", exhausted)
        if all(is_identity("three", c, pool) for _, c in combos):
            assert pool == 1 and changed == 0 and exhausted == 0
        else:
            assert changed >= 1, pool
    for name in LAYOUTS:
        for k in (3, 100):
            _, g, combos = layout_case(name, k)
            changed, exhausted = vacuity_counts(40 + k, D1, D2, k, g, 64, combos)
            print(name, k, "changed", changed, "exhausted", exhausted)
            if name in ("distinct", "negative"):
                assert changed == 0 and exhausted == 0
            else:
                assert changed >= 1, (name, k)
            if name in ("one", "three") and k == 3:
                assert exhausted >= 1, name
    # the other exact GPU cases: the merge across item splits and the two user batches
    U, V, index, item = _merge_case()
    pi, ps = ref_topk(U @ V.T, excl_mask(U.shape[0], V.shape[0], index, item), 100)
    it, _, st = ref_capped(pi, ps, layout("mixed", V.shape[0]), 2, 10)
    assert ((it != pi[:, :10]).any(1) & (st == CAP_EXACT)).sum() >= 1


# ---------------------------------------------------------------------------------------------------------------- GPU helpers
def check_exact(case, groups, dtype, pool, topk, cap, users=None, allow=None, what=None):
    """recommend_capped against ref_capped on recommend()'s pool, and against ref_capped_full over the whole catalogue (the
    integer scores are exact in both dtypes).  Returns the device result."""
    import primalcr_amd as pcr
    U, V, index, item = case
    what = (what, dtype, pool, topk, cap)
    kw = dict(exclude=(index, item), users=users, dtype=dtype, allow=allow)
    pi, ps = pcr.recommend(U, V, pool, **kw)
    it, sc, st, stats = pcr.recommend_capped(U, V, topk, groups, cap, pool=pool, **kw)
    wi, ws, wst = ref_capped(pi, ps, groups, cap, topk)
    assert it.shape == (pi.shape[0], topk) and it.dtype == np.int32 and st.dtype == np.uint8
    assert np.array_equal(it, wi), what
    assert np.array_equal(bits(sc), bits(ws)), what
    assert np.array_equal(st, wst), what
    assert stats == stats_of(wi, wst), what
    S = U @ V.T
    rows = np.arange(U.shape[0]) if users is None else np.asarray(users)
    elig = ~excl_mask(U.shape[0], V.shape[0], index, item)
    if allow is not None:
        elig &= np.asarray(allow, bool)[None, :]
    for i, u in enumerate(rows):
        fi, fs = ref_capped_full(S[u], elig[u], groups, cap, topk)
        L = int((it[i] >= 0).sum())
        if st[i] == CAP_EXACT:
            assert list(it[i, :L]) == fi and np.array_equal(bits(sc[i, :L]), bits(np.array(fs))), (what, i)
        else:
            assert L < topk and list(it[i, :L]) == fi[:L] and np.array_equal(bits(sc[i, :L]), bits(np.array(fs[:L]))), (what, i)
    if is_identity("", cap, pool):
        assert same_lists((it, sc), (pi[:, :topk], ps[:, :topk])) and not st.any(), what
    return it, sc, st, stats


def _merge_case():
    """test_partial_list_merge's inputs: 64 users, 5000 items (four item splits at pool 100), exclusion rows around the boundaries."""
    d1, d2, k, pool = 64, 5000, 3, 100
    per = rec_geometry(d1, d2, pool, 1)[0].per
    rng = np.random.default_rng(41)
    U, V = int_factors(rng, d1, k), int_factors(rng, d2, k)
    index, item = random_csr(rng, d1, d2, {u: boundary_row(u, d2, per) for u in range(d1)})
    return U, V, index, item


def _gauss(seed, d1, d2, k):
    rng = np.random.default_rng(seed)
    U, V = rng.standard_normal((d1, k)), rng.standard_normal((d2, k))
    index, item = random_csr(rng, d1, d2)
    return U, V, index, item


DTYPES = pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.timeout(300)
@DTYPES
@pytest.mark.parametrize("pool", POOLS)
def test_pool_and_lane_edges(dtype, pool):
    case, g, combos = edge_case(pool)
    for topk, cap in combos:
        check_exact(case, g, dtype, pool, topk, cap)


@pytest.mark.gpu
@pytest.mark.timeout(300)
@DTYPES
@pytest.mark.parametrize("k", [3, 100])
@pytest.mark.parametrize("name", LAYOUTS)
def test_group_layouts_and_ranks(dtype, name, k):
    import primalcr_amd as pcr
    case, g, combos = layout_case(name, k)
    U, V, index, item = case
    for topk, cap in combos:
        it, sc, st, stats = check_exact(case, g, dtype, 64, topk, cap, what=name)
        if name in ("distinct", "negative"):
            assert same_lists((it, sc), pcr.recommend(U, V, topk, exclude=(index, item), dtype=dtype)) and not st.any(), (name, cap)
        if name == "one":
            assert np.array_equal((it >= 0).sum(1)[3:], np.full(D1 - 3, cap)) and st[3:].all() and stats["exhausted"] == D1 - 3, cap


@pytest.mark.gpu
@pytest.mark.timeout(300)
@DTYPES
def test_short_and_empty_pools(dtype):
    """Users 0, 1, 2 keep 30 (< pool), 7 (< topk) and 0 eligible items: status 0 whatever is kept, padding (-1, -inf)."""
    case = exact_case(61, D1, D2, 3)
    for name, cap in (("three", 1), ("three", 5), ("one", 2), ("mixed", 1), ("negative", 1)):
        it, sc, st, stats = check_exact(case, layout(name, D2), dtype, 64, 10, cap, what=name)
        assert not st[:3].any(), name
        length = (it >= 0).sum(1)
        assert length[2] == 0 and np.all(it[2] == -1) and np.all(np.isneginf(sc[2])), name
        assert length[1] <= 7 and np.all(it[1, length[1]:] == -1) and np.all(np.isneginf(sc[1, length[1]:])), name
        if name == "negative":
            assert list(length[:3]) == [10, 7, 0]
        if name == "one":
            assert list(length[:3]) == [2, 2, 0] and stats["short_rows"] == D1 and stats["kept"] == 2 * (D1 - 1)


@pytest.mark.gpu
@pytest.mark.timeout(300)
@DTYPES
def test_partial_list_merge(dtype):
    """Four item splits (the shape decides: rec_run has no split knob) with exclusion rows around the split boundaries, against the
    references, which know no splits."""
    case = _merge_case()
    d1, d2 = case[0].shape[0], case[1].shape[0]
    assert splits_of(d1, d2, 100, dtype) == 4
    for name, cap, topk in (("mixed", 2, 10), ("three", 5, 10), ("three", 1, 100), ("sparse", 2, 1)):
        check_exact(case, layout(name, d2), dtype, 100, topk, cap, what=name)


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_two_user_batches():
    """44 000 requests at pool 1024 in fp64 are two batches of rec_run (43 648 + 352): every repeated user id returns identical
    bits whichever batch it sits in, and a sample of rows (the batches' first and last among them) equals the reference."""
    import primalcr_amd as pcr
    n, d1, d2, k, pool, topk, cap, dtype = 44000, 500, 1100, 3, 1024, 3, 1, 1
    geo = rec_geometry(n, d2, pool, dtype)
    assert [(b.b0, b.users) for b in geo] == [(0, 43648), (43648, 352)]
    U, V, index, item = exact_case(51, d1, d2, k)
    g = layout("mixed", d2)
    rng = np.random.default_rng(52)
    users = rng.integers(0, d1, n).astype(np.int32)
    it, sc, st, stats = pcr.recommend_capped(U, V, topk, g, cap, pool=pool, exclude=(index, item), users=users, dtype=dtype)
    first = np.full(d1, -1, np.int64)
    first[users[::-1]] = np.arange(n - 1, -1, -1)
    assert np.array_equal(it, it[first[users]]) and np.array_equal(bits(sc), bits(sc[first[users]])) and np.array_equal(st, st[first[users]])
    assert stats == stats_of(it, st) and stats["users"] == n
    edge = [r for b in geo for r in (b.b0, b.b0 + b.users - 1)]
    rows = np.unique(np.concatenate([edge, rng.integers(0, n, 60 - len(edge))])).astype(np.int64)
    pi, ps = pcr.recommend(U, V, pool, exclude=(index, item), users=users[rows], dtype=dtype)
    wi, ws, wst = ref_capped(pi, ps, g, cap, topk)
    assert np.array_equal(it[rows], wi) and np.array_equal(bits(sc[rows]), bits(ws)) and np.array_equal(st[rows], wst)
    assert (wi != pi[:, :topk]).any()


@pytest.mark.gpu
@pytest.mark.timeout(300)
@DTYPES
def test_identities(dtype):
    """All groups negative, all distinct, or cap >= pool: recommend()'s top-topk bit for bit, every status 0.  The first kept entry
    is pool position 0.  cap = 1 with a single group: exactly one item per list."""
    import primalcr_amd as pcr
    d1, d2, k, topk = 60, 1500, 100, 20
    U, V, index, item = _gauss(81, d1, d2, k)
    ex = (index, item)
    plain = pcr.recommend(U, V, topk, exclude=ex, dtype=dtype)
    three = layout("three", d2)
    for pool in (topk, 100, 1024):
        for g, cap in ((layout("negative", d2), 1), (layout("distinct", d2), 1), (three, pool), (three, pool + 1), (layout("one", d2), 2 ** 31 - 1)):
            it, sc, st, stats = pcr.recommend_capped(U, V, topk, g, cap, pool=pool, exclude=ex, dtype=dtype)
            assert same_lists((it, sc), plain) and not st.any(), (pool, cap)
            assert stats == dict(users=d1, exact=d1, exhausted=0, short_rows=0, kept=d1 * topk)
        it, sc, st, _ = pcr.recommend_capped(U, V, topk, three, 2, pool=pool, exclude=ex, dtype=dtype)
        assert np.array_equal(it[:, 0], plain[0][:, 0]) and np.array_equal(bits(sc[:, 0]), bits(plain[1][:, 0]))
        assert (it != plain[0]).any()
        it, sc, st, stats = pcr.recommend_capped(U, V, topk, layout("one", d2), 1, pool=pool, exclude=ex, dtype=dtype)
        assert np.array_equal(it[:, 0], plain[0][:, 0]) and np.all(it[:, 1:] == -1) and np.all(np.isneginf(sc[:, 1:]))
        assert st.all() and stats == dict(users=d1, exact=0, exhausted=d1, short_rows=d1, kept=d1)


@pytest.mark.gpu
@pytest.mark.timeout(300)
@DTYPES
def test_allow_set(dtype):
    import primalcr_amd as pcr
    case = exact_case(71, D1, D2, 3)
    U, V, index, item = case
    rng = np.random.default_rng(72)
    allow = rng.random(D2) < 0.5
    g = layout("three", D2)
    for pool, topk, cap in ((64, 10, 5), (64, 10, 1), (128, 128, 2), (200, 10, 2)):
        it, sc, st, _ = check_exact(case, g, dtype, pool, topk, cap, allow=allow, what="allow")
        assert allow[it[it >= 0]].all()
    none = np.zeros(D2, bool)
    it, sc, st, stats = pcr.recommend_capped(U, V, 10, g, 2, pool=64, exclude=(index, item), dtype=dtype, allow=none)
    assert np.all(it == -1) and np.all(np.isneginf(sc)) and not st.any()
    assert stats == dict(users=D1, exact=D1, exhausted=0, short_rows=D1, kept=0)


@pytest.mark.gpu
@pytest.mark.timeout(300)
@DTYPES
def test_independence_of_the_other_users(dtype):
    import primalcr_amd as pcr
    d1, d2, k = 300, 2500, 40
    U, V, index, item = _gauss(91, d1, d2, k)
    g = layout("mixed", d2)
    kw = dict(pool=100, exclude=(index, item), dtype=dtype)
    rng = np.random.default_rng(92)
    a = pcr.recommend_capped(U, V, 10, g, 1, **kw)
    b = pcr.recommend_capped(U, V, 10, g, 1, **kw)
    assert same_lists(a, b) and np.array_equal(a[2], b[2]) and a[3] == b[3]
    perm = rng.permutation(d1).astype(np.int32)
    c = pcr.recommend_capped(U, V, 10, g, 1, users=perm, **kw)
    assert same_lists(c, (a[0][perm], a[1][perm])) and np.array_equal(c[2], a[2][perm])
    sub = np.array([299, 0, 17, 17, 64], np.int32)
    d = pcr.recommend_capped(U, V, 10, g, 1, users=sub, **kw)
    assert same_lists(d, (a[0][sub], a[1][sub])) and np.array_equal(d[2], a[2][sub])


@pytest.mark.gpu
@pytest.mark.timeout(300)
@DTYPES
def test_gaussian_factors(dtype):
    """Non-tied scores at k = 100: items, scores and status equal ref_capped applied to recommend(K = pool)'s own output."""
    import primalcr_amd as pcr
    d1, d2, k = 60, 1500, 100
    U, V, index, item = _gauss(70 + dtype, d1, d2, k)
    for name, pool, topk, cap in (("three", 100, 20, 5), ("three", 100, 20, 2), ("mixed", 65, 20, 1), ("sparse", 1024, 10, 3), ("one", 64, 64, 5)):
        g = layout(name, d2)
        pi, ps = pcr.recommend(U, V, pool, exclude=(index, item), dtype=dtype)
        it, sc, st, stats = pcr.recommend_capped(U, V, topk, g, cap, pool=pool, exclude=(index, item), dtype=dtype)
        wi, ws, wst = ref_capped(pi, ps, g, cap, topk)
        assert np.array_equal(it, wi) and np.array_equal(bits(sc), bits(ws)) and np.array_equal(st, wst), (name, pool)
        assert stats == stats_of(wi, wst) and (wi != pi[:, :topk]).any(), (name, pool)


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_composition_with_evaluate_lists():
    """The capped lists go through evaluate_lists(); cap = 1 with every item in one of three groups: at most three items per list,
    at most one per group (checked from the lists on the host)."""
    import primalcr_amd as pcr
    d1, d2, k = 60, 1500, 16
    U, V, index, item = _gauss(95, d1, d2, k)
    g = layout("three", d2)
    it, sc, st, stats = pcr.recommend_capped(U, V, 10, g, 1, pool=100, exclude=(index, item))
    for row in it:
        got = row[row >= 0]
        assert 1 <= got.shape[0] <= 3 and np.unique(g[got]).shape[0] == got.shape[0]
    assert stats["kept"] == int((it >= 0).sum()) and stats["short_rows"] == d1
    res = pcr.evaluate_lists(it, V, d1=d1, cutoffs=(5, 10), per_user=True)
    assert [c["users"] for c in res["diversity"]] == [d1, d1] and [c["recs"] for c in res["diversity"]] == [stats["kept"]] * 2
    assert np.array_equal(res["per_user_diversity"][:, 1, 0], (it >= 0).sum(1))               # len at the last cutoff


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_live_solvers():
    """Solver.recommend_capped on PCR++ and CCDR1 after one iteration equals recommend_capped on get_factors() in the solver's
    storage type, with and without the training exclusion; the profile slot has launches; the factors are bitwise untouched."""
    import primalcr_amd as pcr
    from primalcr_amd import synth
    R = synth.generate("small", seed=17)
    ds = pcr.Dataset.from_ratings(R)
    rng = np.random.default_rng(9)
    g = layout("mixed", R.d2)
    r = 16
    for solver_type in (pcr.PCR_SOLVER_PCRPP, pcr.PCR_SOLVER_CCDR1):
        for prec in (pcr.PCR_F32, pcr.PCR_F64):
            what = (solver_type, prec)
            p = pcr.Parameter(k=r, precision=prec, solver_type=solver_type, **{"lambda": 100.0})
            s = pcr.Solver(ds, p)
            if solver_type == pcr.PCR_SOLVER_CCDR1:
                s.set_factors(pcr.initial_col(R.d1, r), np.zeros((R.d2, r)))
            else:
                s.set_factors(pcr.initial(R.d1, r), pcr.initial(R.d2, r))
            s.iterate(1)
            U, V = s.get_factors()
            s.profile(True)
            a = s.recommend_capped(10, g, 2, pool=64)
            prof = s.profile_all()
            assert prof.get("recommend/cap", (0, 0))[1] >= 1 and "recommend/score" in prof, prof
            s.profile(False)
            b = pcr.recommend_capped(U, V, 10, g, 2, pool=64, exclude=ds, dtype=prec)
            assert same_lists(a, b) and np.array_equal(a[2], b[2]) and a[3] == b[3], what
            assert a[0].shape == (R.d1, 10) and (a[0] != pcr.recommend(U, V, 10, exclude=ds, dtype=prec)[0]).any()
            users = rng.choice(R.d1, 33, replace=False).astype(np.int32)
            allow = rng.random(R.d2) < 0.7
            c = s.recommend_capped(5, g, 1, users=users, exclude_train=False, allow=allow)
            d = pcr.recommend_capped(U, V, 5, g, 1, pool=50, users=users, dtype=prec, allow=allow)
            assert same_lists(c, d) and np.array_equal(c[2], d[2]) and c[3] == d[3], what
            with pytest.raises(pcr.PcrError, match="pcr_recommend_capped"):
                s.recommend_capped(5, g, 1, users=np.array([R.d1], np.int32))           # outside the shard
            U2, V2 = s.get_factors()
            assert np.array_equal(bits(U), bits(U2)) and np.array_equal(bits(V), bits(V2)), what
            s.close()


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_cli_end_to_end(tmp_path):
    import primalcr_amd as pcr
    from primalcr_amd import synth
    R = synth.generate("small", seed=13)
    d = synth.write_dir(R, str(tmp_path / "data"))
    out = run([TRAIN, "-k", "8", "-t", "2", "-l", "100", d, "m.model"], tmp_path)
    assert out.returncode == 0, out.stderr
    U, V = pcr.model_load(str(tmp_path / "m.model"))
    ds = pcr.Dataset.from_ratings(R)
    g = layout("mixed", R.d2)
    (tmp_path / "g.txt").write_text("".join(f"{int(x)}\n" for x in g))

    def line_of(stats):
        return (f"capped users {stats['users']} exact {stats['exact']} pool_exhausted {stats['exhausted']} short {stats['short_rows']} "
                f"kept {stats['kept']}")

    r = run([RECOMMEND, "--groups", "g.txt", "--max-per-group", "1", "--pool", "64", "-x", d, "m.model", "lists.txt"], tmp_path)
    assert r.returncode == 0, r.stderr
    items, _, _, stats = pcr.recommend_capped(U, V, 10, g, 1, pool=64, exclude=ds)
    assert r.stdout.strip().splitlines() == [line_of(stats)]
    lines = (tmp_path / "lists.txt").read_text().strip().splitlines()
    assert len(lines) == R.d1
    for u, line in enumerate(lines):
        f = [int(x) for x in line.split()]
        assert f[0] == u + 1 and f[1:] == [int(j) + 1 for j in items[u] if j >= 0], u
    assert (items != pcr.recommend(U, V, 10, exclude=ds)[0]).any()
    (tmp_path / "users").write_text("3\n1\n3\n")
    allow = np.arange(R.d2) % 3 != 0
    (tmp_path / "allow").write_text("".join(f"{j + 1}\n" for j in np.nonzero(allow)[0]))
    r = run([RECOMMEND, "--groups", "g.txt", "--max-per-group", "2", "-K", "4", "--f32", "--scores", "-u", "users", "--allow", "allow", "m.model",
             "three.txt"], tmp_path)
    assert r.returncode == 0, r.stderr
    it, sc, _, stats = pcr.recommend_capped(U, V, 4, g, 2, users=np.array([2, 0, 2], np.int32), dtype=pcr.PCR_F32, allow=allow)
    assert r.stdout.strip().splitlines() == [line_of(stats)]
    lines = (tmp_path / "three.txt").read_text().strip().splitlines()
    assert [int(l.split()[0]) for l in lines] == [3, 1, 3]
    for i, line in enumerate(lines):
        assert [x.split(":")[0] for x in line.split()[1:]] == [str(int(j) + 1) for j in it[i] if j >= 0]
        assert [x.split(":")[1] for x in line.split()[1:]] == [f"{v:.6f}" for v in sc[i][it[i] >= 0]]
