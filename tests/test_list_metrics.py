"""Metrics of lists the caller brings (pcr_evaluate_lists_model, Python evaluate_lists(); k_list_metrics of pcr_topk.h): the
top-N and the beyond-accuracy metrics of include/primalcr.h with L_u = the given list.

CPU part: every argument error of the entry (reported before a device is looked for), the "no device" error, the wrapper's
ValueErrors, the constants of the header mirrored in api.py.
GPU part (-m gpu): on the lists recommend() returns the per-user rows and the exposure are bit for bit those of evaluate_topn() /
evaluate_diversity() (the kernel runs the same two tails); on lists nobody selected (random permutations of random item subsets,
every length from 0 to L, padded tails) they agree with test_topn_eval.ref_metrics / test_diversity.ref_diversity under those
files' tolerances, and on test_rerank.dyadic_V -- where every cosine is a multiple of 1/16 and every norm 0, 1, 2 or 4, so the
ILD's numerator is exact in any order -- the ILD and every count are equal (==).
"""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_diversity as tdiv
import test_topn_eval as ttop
from conftest import ROOT
from test_diversity import check_rows, ref_diversity, ref_info
from test_recommend_grid import random_csr, sub_test_csr
from test_rerank import dyadic_V
from test_topn_eval import check_per_user, make_test_csr, ref_metrics

ERR_ARG, ERR_DEVICE = -1, -4
DTYPES = pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _lists_call(V, d1, index, item, tindex, titem, tval, users, lists, cutoffs, threshold=-math.inf, dtype=1, n=None, L=None, topn=True,
                per_user_topn=False, div=True):
    """pcr_evaluate_lists_model through ctypes, arrays as given (None = NULL); returns the status code."""
    import primalcr_amd as pcr
    from primalcr_amd.api import TopnStats
    n = lists.shape[0] if n is None else n
    L = lists.shape[1] if L is None else L
    cuts = None if cutoffs is None else np.asarray(cutoffs, np.int32)
    ts, ds = (TopnStats * 16)(), (pcr.DiversityStats * 16)()
    pu = np.empty((max(n, 1), 16, 6))
    ptr = lambda a: None if a is None else a.ctypes.data
    return pcr.lib().pcr_evaluate_lists_model(ptr(V), V.shape[0], V.shape[1], d1, ptr(index), ptr(item), ptr(tindex), ptr(titem), ptr(tval), n,
                                              ptr(users), L, ptr(lists), 0 if cuts is None else len(cuts), ptr(cuts), float(threshold), dtype,
                                              C.cast(ts, C.c_void_p) if topn else None, ptr(pu) if per_user_topn else None,
                                              C.cast(ds, C.c_void_p) if div else None, None, None, 0)


def _small():
    rng = np.random.default_rng(1)
    V = rng.standard_normal((30, 5))
    d1 = 20
    index = np.array([0] + [2] * 20, np.int64)
    item = np.array([3, 7], np.int32)
    tindex = np.array([0, 3] + [4] * 19, np.int64)
    titem = np.array([9, 1, 9, 4], np.int32)
    tval = np.array([5.0, 3.0, 4.0, 1.0])
    users = np.arange(20, dtype=np.int32)
    lists = np.tile(np.array([4, 9, 0, 29, -1, -1], np.int32), (20, 1))
    return V, d1, index, item, tindex, titem, tval, users, lists


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_argument_checks():
    import primalcr_amd as pcr
    V, d1, index, item, tindex, titem, tval, users, lists = _small()

    def bad(*a, **kw):
        assert _lists_call(*a, **kw) == ERR_ARG
        assert b"pcr_evaluate_lists_model" in pcr.lib().pcr_last_error(), pcr.lib().pcr_last_error()

    def with_row(row):
        l = lists.copy(); l[7] = row
        return l

    ok = (V, d1, index, item, tindex, titem, tval, users)
    bad(*ok, with_row([4, 9, 30, 1, -1, -1]), [3])                     # an entry outside [0, d2)
    bad(*ok, with_row([4, 9, -2, 1, -1, -1]), [3])                     # negative and not -1
    bad(*ok, with_row([4, -1, 9, 1, -1, -1]), [3])                     # a non-padding entry after a -1
    bad(*ok, with_row([-1, -1, -1, -1, -1, 2]), [3])
    bad(*ok, with_row([4, 9, 0, 4, -1, -1]), [3])                      # an id twice in one list
    assert b"twice" in pcr.lib().pcr_last_error() and b"list 7" in pcr.lib().pcr_last_error()
    bad(*ok, lists, [3], L=0)                                          # L outside [1, PCR_RECOMMEND_MAX_K]
    bad(*ok, lists, [3], L=1025)
    bad(V, d1, index, item, tindex, titem, tval, np.array([0] * 19 + [20], np.int32), lists, [3])      # a user outside [0, d1)
    bad(V, d1, index, item, tindex, titem, tval, np.array([-1] + [0] * 19, np.int32), lists, [3])
    bad(V, d1, index, item, tindex, titem, tval, None, lists[:19], [3])                                 # users NULL: n == d1
    bad(*ok, lists, [3, 7])                                            # the last cutoff above L
    # the cutoff errors of the existing model entries
    for cuts in ([0], [], None, list(range(1, 10)), [5, 3], [3, 3]):
        bad(*ok, lists, cuts)
    bad(*ok, lists, [3], threshold=math.nan)
    bad(*ok, lists, [3], dtype=5)
    bad(*ok, lists, [3], div=False)
    bad(*ok, lists, [3], topn=False)                                   # a test CSR wants its stats
    bad(*ok, lists, [3], n=-1)
    bad(*ok, None, [3], n=20, L=6)                                     # no lists
    # without a test CSR topn and per_user_topn must be NULL
    bad(V, d1, index, item, None, None, None, users, lists, [3])
    bad(V, d1, index, item, None, None, None, users, lists, [3], topn=False, per_user_topn=True)
    # the CSR errors of the existing model entries
    bad(V, d1, index, item, tindex, None, tval, users, lists, [3])
    t = tindex.copy(); t[5] = 1
    bad(V, d1, index, item, t, titem, tval, users, lists, [3])
    t = tindex.copy(); t[0] = 1
    bad(V, d1, index, item, t, titem, tval, users, lists, [3])
    bad(V, d1, index, item, tindex, np.array([9, 1, 30, 4], np.int32), tval, users, lists, [3])
    bad(V, d1, index, None, tindex, titem, tval, users, lists, [3])
    x = index.copy(); x[5] = 1
    bad(V, d1, x, item, tindex, titem, tval, users, lists, [3])
    bad(V, d1, index, np.array([3, 30], np.int32), tindex, titem, tval, users, lists, [3])


def test_without_a_device_is_a_device_error():
    """Valid arguments on a process that sees no GPU: PCR_ERR_DEVICE (never a CPU path), with and without a test CSR."""
    code = ("import sys, numpy as np; sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')\n"
            "from test_list_metrics import _lists_call, _small\n"
            "V, d1, index, item, tindex, titem, tval, users, lists = _small()\n"
            "print(_lists_call(V, d1, index, item, tindex, titem, tval, users, lists, [1, 6]),\n"
            "      _lists_call(V, d1, None, None, None, None, None, None, lists, [3], dtype=0, topn=False))\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    assert [int(x) for x in out.stdout.strip().splitlines()[-1].split()] == [ERR_DEVICE, ERR_DEVICE]


def test_python_wrapper_refuses_bad_arguments():
    import primalcr_amd as pcr
    V, d1, index, item, tindex, titem, tval, users, lists = _small()
    test, pop = (tindex, titem, tval), (index, item)
    row = lambda r: np.vstack([lists[:19], np.array([r], np.int32)])
    for args, kw in (((row([4, 9, 30, 1, -1, -1]), V), dict()), ((row([4, 9, -2, 1, -1, -1]), V), dict()),
                     ((row([4, -1, 9, 1, -1, -1]), V), dict()), ((row([4, 9, 0, 4, -1, -1]), V), dict()),
                     ((lists[:, :0], V), dict()), ((np.zeros((2, 1025), np.int32), V), dict()), ((lists[0], V), dict()),
                     ((lists, V), dict(cutoffs=(7,))), ((lists, V), dict(cutoffs=(3, 3))), ((lists, V), dict(cutoffs=(0,))),
                     ((lists, V), dict(cutoffs=tuple(range(1, 10)))), ((lists, V), dict(cutoffs=(3,), threshold=math.nan)),
                     ((lists, V), dict(cutoffs=(3,), d1=21)), ((lists, V), dict(cutoffs=(3,), users=users[:5])),
                     ((lists, V), dict(cutoffs=(3,), users=users + 1)), ((lists, V), dict(cutoffs=(3,), test=(tindex, titem[:3], tval[:3]))),
                     ((lists, V), dict(cutoffs=(3,), popularity=(index[:5], item)))):
        with pytest.raises(ValueError):
            pcr.evaluate_lists(*args, **{**dict(cutoffs=(3,), test=test, popularity=pop), **kw})
    assert pcr.evaluate_lists is pcr.api.evaluate_lists and "evaluate_lists" in pcr.__all__ and "evaluate_rerank" in pcr.__all__
    assert "PCR_RERANK_MAX_THETAS" in pcr.__all__


def test_header_constants_are_mirrored():
    import primalcr_amd as pcr
    hdr = open(os.path.join(ROOT, "include", "primalcr.h")).read()
    m = re.search(r"#define PCR_RERANK_MAX_THETAS (\d+)", hdr)
    assert m and int(m.group(1)) == pcr.PCR_RERANK_MAX_THETAS == pcr.api.PCR_RERANK_MAX_THETAS == 8
    for name in ("PCR_RECOMMEND_MAX_K", "PCR_TOPN_MAX_CUTOFFS"):
        assert int(re.search(r"#define " + name + r" (\d+)", hdr).group(1)) == getattr(pcr, name)
    for sym in ("pcr_evaluate_lists_model", "pcr_evaluate_rerank_model", "pcr_evaluate_rerank"):
        assert re.search(r"\bint " + sym + r"\(", hdr) and hasattr(pcr.lib(), sym)


# ---------------------------------------------------------------------------------------------------------------- GPU
def _identity_case(seed, d1, d2, k):
    """Gaussian factors, an exclusion CSR in which user 5 keeps 3 eligible items and user 6 none (padded and empty lists), a test
    CSR with empty rows, duplicated items and rows below the threshold."""
    rng = np.random.default_rng(seed)
    U, V = rng.standard_normal((d1, k)), rng.standard_normal((d2, k))
    V[::17] = 0.0                                                          # rows of norm 0
    special = {5: np.setdiff1d(np.arange(d2), [1, d2 // 2, d2 - 1]).astype(np.int32), 6: np.arange(d2, dtype=np.int32)}
    index, item = random_csr(rng, d1, d2, special)
    return U, V, index, item, make_test_csr(rng, d1, d2, index, item)


@pytest.mark.gpu
@pytest.mark.timeout(300)
@DTYPES
@pytest.mark.parametrize("k", [1, 7, 100, 132, 200])
def test_identity_with_the_existing_sinks_bitwise(dtype, k):
    """lists = recommend(K)'s items: per-user rows and exposure equal evaluate_topn / evaluate_diversity bit for bit (NaNs as
    bits); k = 132 and 200 take the ILD's second 128-component pass."""
    import primalcr_amd as pcr
    d1 = 37
    for L in (1, 2, 63, 64, 65, 128, 1024):
        d2 = 1100 if L == 1024 else 300
        U, V, index, item, test = _identity_case(1000 * k + L, d1, d2, k)
        ex = (index, item)
        sets = sorted({(1, L) if L > 1 else (1,), tuple(c for c in (5, 10, 64) if c < L) + (L,)})
        for cutoffs, thr in zip(sets, (4.0, -math.inf)):
            what = (k, L, cutoffs, thr)
            items, _ = pcr.recommend(U, V, L, exclude=ex, dtype=dtype)
            assert (items[5] >= 0).sum() == min(3, L) and (items[6] == -1).all()
            got = pcr.evaluate_lists(items, V, test=test, popularity=ex, cutoffs=cutoffs, threshold=thr, dtype=dtype, per_user=True, exposure=True)
            ts, tpu = pcr.evaluate_topn(U, V, test, cutoffs=cutoffs, exclude=ex, threshold=thr, dtype=dtype, per_user=True)
            dv, dpu, dex = pcr.evaluate_diversity(U, V, cutoffs=cutoffs, exclude=ex, dtype=dtype, per_user=True, exposure=True)
            assert np.array_equal(bits(got["per_user_topn"]), bits(tpu)), what
            assert np.array_equal(bits(got["per_user_diversity"]), bits(dpu)), what
            assert got["exposure"].dtype == np.int64 and np.array_equal(got["exposure"], dex), what
            counted = ~np.isnan(tpu[:, 0, 0])
            assert 0 < counted.sum() < d1                               # counted and uncounted users are both there
            for g, w in zip(got["topn"], ts):
                assert [g[f] for f in ("cutoff", "users", "users_graded", "hits")] == [w[f] for f in ("cutoff", "users", "users_graded", "hits")], what
            for g, w in zip(got["diversity"], dv):
                for f in ("cutoff", "users", "users_ild", "recs", "items_covered", "coverage", "gini"):
                    assert g[f] == w[f], (what, f)
        # users[] in another order, a user twice: the same rows
        users = np.array([36, 5, 0, 6, 5, 17], np.int32)
        sub = pcr.evaluate_lists(items[users], V, d1=d1, users=users, test=test, popularity=ex, cutoffs=cutoffs, threshold=thr, dtype=dtype,
                                 per_user=True)
        assert np.array_equal(bits(sub["per_user_topn"]), bits(got["per_user_topn"][users])), (k, L)
        assert np.array_equal(bits(sub["per_user_diversity"]), bits(got["per_user_diversity"][users])), (k, L)
        assert sub["diversity"][0]["users"] == 6 and sub["topn"][0]["users"] == int(counted[users].sum())


def _free_lists(rng, n, d2, L):
    """Lists nobody selected: request i holds i % (L + 1) items (every length from 0 to L, so every padded tail), a random
    permutation of a random subset of the catalogue."""
    lists = np.full((n, L), -1, np.int32)
    for i in range(n):
        m = i % (L + 1)
        lists[i, :m] = rng.choice(d2, m, replace=False)
    return lists


@pytest.mark.gpu
@pytest.mark.timeout(300)
@DTYPES
@pytest.mark.parametrize("exact", [False, True], ids=["gauss", "dyadic"])
def test_lists_nobody_selected_against_the_definitions(dtype, exact):
    import primalcr_amd as pcr
    rng = np.random.default_rng(40 + dtype + 2 * exact)
    d1, d2, k, L, n = 60, 90, (16 if exact else 130), 70, 150
    V = dyadic_V(rng, d2, k) if exact else rng.standard_normal((d2, k))
    if not exact:
        V[::13] = 0.0
    index, item = random_csr(rng, d1, d2)
    tindex, titem, tval = make_test_csr(rng, d1, d2, index, item)
    users = rng.integers(0, d1, n).astype(np.int32)                        # ids repeat: each request counts
    lists = _free_lists(rng, n, d2, L)
    assert (np.diff(tindex) == 0).any() and sorted(set((lists >= 0).sum(1))) == list(range(L + 1))
    info = ref_info(d1, d2, item)
    sub = sub_test_csr(tindex, titem, tval, users)                          # row i = the test row of users[i]
    for cutoffs in ((1, 5, 64, 70), (3, 10)):                               # (3, 10): the last cutoff below L
        for thr in (-math.inf, 4.0):
            what = (exact, cutoffs, thr)
            got = pcr.evaluate_lists(lists, V, d1=d1, users=users, test=(tindex, titem, tval), popularity=(index, item), cutoffs=cutoffs,
                                     threshold=thr, dtype=dtype, per_user=True, exposure=True)
            want_t, want_ts = ref_metrics(lists, *sub, cutoffs, thr)
            want_d, want_ex, want_ds = ref_diversity(lists, V, info, cutoffs, dtype == 0)
            check_per_user(got["per_user_topn"], want_t)
            check_rows(got["per_user_diversity"], want_d, what)
            assert np.array_equal(got["exposure"], want_ex), what
            ttop.check_summary(got["topn"], want_ts)
            tdiv.check_summary(got["diversity"], want_ds, what=what)
            assert 0 < got["topn"][0]["users"] < n and got["diversity"][0]["users"] == n
            if exact:                                                       # every cosine a multiple of 1/16: the ILD is the same number
                ild, wild = got["per_user_diversity"][..., 2], want_d[..., 2]
                assert np.array_equal(np.isnan(ild), np.isnan(wild)) and np.array_equal(ild[~np.isnan(wild)], wild[~np.isnan(wild)]), what
                ok = ~np.isnan(want_t[..., 0])
                assert np.array_equal(got["per_user_diversity"][..., 0], want_d[..., 0]), what
                assert np.array_equal(got["per_user_topn"][..., 0][ok], want_t[..., 0][ok]), what
            # users[] and the lists permuted together: the per-user rows permuted, bit for bit; the exposure unchanged
            p = rng.permutation(n)
            per = pcr.evaluate_lists(lists[p], V, d1=d1, users=users[p], test=(tindex, titem, tval), popularity=(index, item), cutoffs=cutoffs,
                                     threshold=thr, dtype=dtype, per_user=True, exposure=True)
            assert np.array_equal(bits(per["per_user_topn"]), bits(got["per_user_topn"][p])), what
            assert np.array_equal(bits(per["per_user_diversity"]), bits(got["per_user_diversity"][p])), what
            assert np.array_equal(per["exposure"], got["exposure"]), what
    # without a test CSR and without popularity: the diversity part alone, pop = 0
    alone = pcr.evaluate_lists(lists[:d1], V, cutoffs=(5,), dtype=dtype, per_user=True)
    assert "topn" not in alone and "per_user_topn" not in alone
    want_d, _, want_ds = ref_diversity(lists[:d1], V, ref_info(d1, d2, None), (5,), dtype == 0)
    check_rows(alone["per_user_diversity"], want_d)
    tdiv.check_summary(alone["diversity"], want_ds)
