"""Exact full-catalogue rank metrics (pcr_evaluate_ranks_model / pcr_evaluate_ranks, omp-pmf-recommend --eval --ranks, Python
evaluate_ranks()): AUC, MRR, mean and percentile rank of every held-out item among all the items a user has not rated.

CPU part: argument checks of the C ABI (before any device is looked for), the "no device" error, the CLI's usage text and the
--ranks without --eval error.
GPU part (-m gpu), all comparisons exact: ranks[], the per-user table and the summary against the brute-force definitions in
numpy on integer factors (ties everywhere); ranks against the positions in recommend()'s own full lists on real-valued factors;
hits and hit rate of evaluate_topn() from the ranks; the same ranks at every item-split count and user-batch size; relevant rows
longer than the kernel's LDS stage; the solver entry, determinism, untouched training, shards, CCDR1; the Netflix shape; the CLI.

The integers (ranks, counts) must be equal.  The per-user doubles must be EQUAL to one fp64 division of the integers the
contract names (include/primalcr.h), which numpy forms here from the brute-force counts; only the means over users, whose
order of summation differs from numpy's, get rtol 1e-12.
"""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import BIN_DIR, ROOT

RECOMMEND = os.path.join(BIN_DIR, "omp-pmf-recommend")
TRAIN = os.path.join(BIN_DIR, "omp-pmf-train")
ERR_ARG, ERR_DEVICE = -1, -4
MEANS = ("mrr", "mean_rank", "auc", "mpr")
RANK_STAGE = 32          # k_rank_count keeps relevant rows up to this length in LDS (rec::RANK_STAGE, pcr_topk.h)


def run(cmd, cwd, timeout=600):
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=timeout)


def _model_call(U, V, index, item, tindex, titem, tval, threshold=-math.inf, dtype=1, stats=True):
    """pcr_evaluate_ranks_model through ctypes, arrays as given (None = NULL); returns the status code."""
    import primalcr_amd as pcr
    from primalcr_amd.api import RankStats
    st = RankStats()
    ptr = lambda a: None if a is None else a.ctypes.data
    return pcr.lib().pcr_evaluate_ranks_model(ptr(U), U.shape[0], ptr(V), V.shape[0], U.shape[1], ptr(index), ptr(item), ptr(tindex),
                                              ptr(titem), ptr(tval), float(threshold), dtype, C_addr(st) if stats else None, None, None, 0)


def C_addr(x):
    import ctypes
    return ctypes.addressof(x)


# ---------------------------------------------------------------------------------------------------------------- CPU
def _small():
    rng = np.random.default_rng(1)
    U, V = rng.standard_normal((20, 5)), rng.standard_normal((30, 5))
    index = np.array([0] + [2] * 20, np.int64)
    item = np.array([3, 7], np.int32)
    tindex = np.array([0, 3] + [4] * 19, np.int64)
    titem = np.array([9, 1, 9, 4], np.int32)
    tval = np.array([5.0, 3.0, 4.0, 1.0])
    return U, V, index, item, tindex, titem, tval


def test_model_entry_argument_checks():
    U, V, index, item, tindex, titem, tval = _small()
    ok = (U, V, index, item, tindex, titem, tval)
    assert _model_call(*ok, threshold=math.nan) == ERR_ARG
    bad = tindex.copy(); bad[5] = 1                                              # test CSR not monotone
    assert _model_call(U, V, index, item, bad, titem, tval) == ERR_ARG
    bad = tindex.copy(); bad[0] = 1
    assert _model_call(U, V, index, item, bad, titem, tval) == ERR_ARG
    assert _model_call(U, V, index, item, tindex, np.array([9, 1, 30, 4], np.int32), tval) == ERR_ARG   # item out of range
    assert _model_call(U, V, index, item, tindex, np.array([9, 1, -1, 4], np.int32), tval) == ERR_ARG
    assert _model_call(U, V, index, item, tindex, None, tval) == ERR_ARG
    assert _model_call(*ok, stats=False) == ERR_ARG                              # NULL stats
    assert _model_call(*ok, dtype=5) == ERR_ARG
    assert _model_call(U, V, index, None, tindex, titem, tval) == ERR_ARG        # exclusion index without item
    ex_bad = index.copy(); ex_bad[3] = 0                                         # exclusion CSR not monotone
    assert _model_call(U, V, ex_bad, item, tindex, titem, tval) == ERR_ARG
    assert _model_call(U, V, index, np.array([3, 30], np.int32), tindex, titem, tval) == ERR_ARG
    import primalcr_amd as pcr
    assert b"pcr_evaluate_ranks_model" in pcr.lib().pcr_last_error()
    with pytest.raises(pcr.PcrError):
        pcr.evaluate_ranks(U, V, (tindex, titem, tval), threshold=math.nan)
    with pytest.raises(ValueError):                                              # last index entry != length of item
        pcr.evaluate_ranks(U, V, (tindex, titem[:3], tval[:3]))
    assert pcr.RANK_FIELDS == ("first_rank", "rr", "mean_rank", "auc", "mpr")
    hdr = open(os.path.join(ROOT, "include", "primalcr.h")).read()
    assert re.search(r"#define PCR_RANK_FIELDS 5\b", hdr)
    topk = open(os.path.join(ROOT, "primalcr_amd", "csrc", "pcr_topk.h")).read()
    assert re.search(rf"constexpr int RANK_STAGE = {RANK_STAGE};", topk)


def test_model_entry_without_a_device_is_a_device_error():
    """Valid arguments on a process that sees no GPU: PCR_ERR_DEVICE (never a CPU path)."""
    code = ("import sys, math, numpy as np; sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')\n"
            "from test_rank_metrics import _model_call, _small\n"
            "print(_model_call(*_small()), _model_call(*_small(), threshold=4.0, dtype=0))\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    assert [int(x) for x in out.stdout.strip().splitlines()[-1].split()] == [ERR_DEVICE, ERR_DEVICE]


def test_cli_usage_and_ranks_without_eval(tmp_path):
    r = run([RECOMMEND], tmp_path)
    assert r.returncode == 1 and "--ranks" in r.stdout
    import primalcr_amd as pcr
    rng = np.random.default_rng(2)
    pcr.model_save(str(tmp_path / "ok.model"), rng.standard_normal((6, 4)), rng.standard_normal((9, 4)))
    r = run([RECOMMEND, "--ranks", "ok.model", "out"], tmp_path)
    assert r.returncode == 1 and "--eval" in r.stderr
    assert not (tmp_path / "out").exists()


# ---------------------------------------------------------------------------------------------------------------- GPU helpers
def ref_ranks(S, index, item, tindex, titem, tval, threshold):
    """The brute-force definitions of include/primalcr.h on a score matrix S (rows = users): (ranks[tnnz], per_user[d1, 5],
    summary).  index / item: the exclusion CSR or None."""
    d1, d2 = S.shape
    ids = np.arange(d2)
    ranks = np.zeros(titem.shape[0], np.int64)
    per = np.full((d1, 5), np.nan)
    relevant = 0
    for u in range(d1):
        z = np.arange(tindex[u], tindex[u + 1])
        z = z[tval[z] >= threshold]
        if z.shape[0] == 0:
            continue
        rel = np.unique(titem[z])
        nonrel = np.ones(d2, bool)
        if index is not None:
            nonrel[item[index[u]:index[u + 1]]] = False
        nonrel[rel] = False
        isrel = np.zeros(d2, bool); isrel[rel] = True
        s = S[u]
        rk, right = {}, 0
        for j in rel:
            before = (s > s[j]) | ((s == s[j]) & (ids < j))
            rk[int(j)] = 1 + int((before & nonrel).sum()) + int((before & isrel).sum())
            right += int((~before & nonrel).sum())          # (j itself is not in nonrel)
        ranks[z] = [rk[int(j)] for j in titem[z]]
        R, N, tot = len(rk), int(nonrel.sum()), sum(rk.values())
        first = min(rk.values())
        per[u] = (first, 1.0 / first, tot / R, right / (R * N) if N else np.nan, (tot - R) / (R * (N + R - 1)) if N + R > 1 else 0.0)
        relevant += R
    return ranks, per, summary_of(per, relevant)


def summary_of(per, relevant):
    c = ~np.isnan(per[:, 0])
    a = c & ~np.isnan(per[:, 3])
    n, na = int(c.sum()), int(a.sum())
    mean = lambda x, k: float(x.sum()) / k if k else 0.0
    return dict(users=n, users_auc=na, relevant=int(relevant), mrr=mean(per[c, 1], n), mean_rank=mean(per[c, 2], n),
                auc=mean(per[a, 3], na), mpr=mean(per[c, 4], n))


def per_user_from_ranks(d1, tindex, ranks, nonrel_count):
    """The per-user table from the integer ranks and |N_u| alone (duplicated test items carry the same rank: counted once by
    the caller's nonrel_count contract, so this helper wants distinct test items)."""
    per = np.full((d1, 5), np.nan)
    for u in range(d1):
        r = ranks[tindex[u]:tindex[u + 1]]
        r = r[r > 0]
        if r.shape[0] == 0:
            continue
        R, N, tot, first = int(r.shape[0]), int(nonrel_count[u]), int(r.sum()), int(r.min())
        right = R * N - (tot - R - R * (R - 1) // 2)
        per[u] = (first, 1.0 / first, tot / R, right / (R * N) if N else np.nan, (tot - R) / (R * (N + R - 1)) if N + R > 1 else 0.0)
    return per


def check_per_user(got, want):
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    bad = np.nonzero(ok & (got != want))
    assert bad[0].shape[0] == 0, (bad[0][:5], bad[1][:5], got[bad][:5], want[bad][:5])


def check_summary(got, want):
    for f in ("users", "users_auc", "relevant"):
        assert got[f] == want[f], (f, got, want)
    for f in MEANS:
        assert got[f] == pytest.approx(want[f], rel=1e-12, abs=0), (f, got, want)


def disjoint_test_csr(rng, d1, d2, index, item, lo=1, hi=12, empty_every=7):
    """A test CSR of distinct items that are not in the user's training row (random order within a row), ratings 1..5; every
    empty_every-th user has no test row."""
    rows = []
    for u in range(d1):
        free = np.setdiff1d(np.arange(d2, dtype=np.int32), item[index[u]:index[u + 1]])
        n = 0 if (empty_every and u % empty_every == 3) else min(int(rng.integers(lo, hi + 1)), free.shape[0])
        rows.append(rng.choice(free, n, replace=False).astype(np.int32))
    tindex = np.zeros(d1 + 1, np.int64)
    tindex[1:] = np.cumsum([r.shape[0] for r in rows])
    titem = np.concatenate(rows).astype(np.int32)
    return tindex, titem, rng.integers(1, 6, titem.shape[0]).astype(np.float64)


def random_csr(rng, d1, d2, lo, hi):
    rows = [np.sort(rng.choice(d2, int(rng.integers(lo, hi + 1)), replace=False)).astype(np.int32) for _ in range(d1)]
    index = np.zeros(d1 + 1, np.int64)
    index[1:] = np.cumsum([r.shape[0] for r in rows])
    return index, np.concatenate(rows).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
def test_exact_ranks_on_integer_factors(dtype):
    """Entries in -3..3: every score is exact in f32 and f64 whatever the order of summation, and ties are everywhere."""
    import primalcr_amd as pcr
    from test_recommend import special_csr
    from test_topn_eval import make_test_csr
    rng = np.random.default_rng(101 + dtype)
    d1 = 150
    for k, d2 in ((1, 70), (7, 30), (100, 500), (200, 3706)):
        U = rng.integers(-3, 4, (d1, k)).astype(np.float64)
        V = rng.integers(-3, 4, (d2, k)).astype(np.float64)
        S = U @ V.T
        index, item = special_csr(rng, d1, d2)                      # users without ratings, one who rated all but 3 items, duplicates
        # test rows with items also in training, duplicated items, users without rows, users with nothing at or above 4
        tindex, titem, tval = make_test_csr(rng, d1, d2, index, item)
        # user 7: every item it has not rated is relevant, so that N_u is empty with exclusion on
        u = 7
        free = np.setdiff1d(np.arange(d2), item[index[u]:index[u + 1]]).astype(np.int32)
        titem = np.concatenate([titem[:tindex[u]], free, titem[tindex[u + 1]:]]).astype(np.int32)
        tval = np.concatenate([tval[:tindex[u]], np.full(free.shape[0], 5.0), tval[tindex[u + 1]:]])
        tindex = tindex.copy(); tindex[u + 1:] += free.shape[0] - (tindex[u + 1] - tindex[u])
        test = (tindex, titem, tval)
        for exclude in ((index, item), None):
            for thr in (-math.inf, 4.0):
                want_r, want_pu, want = ref_ranks(S, *(exclude or (None, None)), tindex, titem, tval, thr)
                got, pu, ranks = pcr.evaluate_ranks(U, V, test, exclude=exclude, threshold=thr, dtype=dtype, per_user=True, ranks=True)
                assert ranks.dtype == np.int64 and np.array_equal(ranks, want_r), (k, d2, exclude is None, thr)
                check_per_user(pu, want_pu)
                check_summary(got, want)
                assert got["users"] < d1                            # users without (relevant) test ratings are not counted
                if exclude is not None:
                    assert math.isnan(pu[7, 3]) and pu[7, 0] == 1 and got["users_auc"] < got["users"]
                assert pcr.evaluate_ranks(U, V, test, exclude=exclude, threshold=thr, dtype=dtype) == got   # summary alone


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_ranks_are_the_positions_in_recommend_lists():
    """Real-valued factors, d2 <= 1024 and K = d2: recommend() returns the full ordered list, and with train and test disjoint
    rank_u(j) is the position of j in it plus one -- no host arithmetic on scores."""
    import primalcr_amd as pcr
    rng = np.random.default_rng(5)
    for d1, d2, k in ((90, 1024, 24), (130, 777, 100), (40, 64, 3)):
        U, V = rng.standard_normal((d1, k)), rng.standard_normal((d2, k))
        V[5] = V[9]                                                  # equal scores for every user
        index, item = random_csr(rng, d1, d2, 0, min(60, d2 // 2))
        tindex, titem, tval = disjoint_test_csr(rng, d1, d2, index, item)
        for dtype in (0, 1):
            for exclude in ((index, item), None):
                items, _ = pcr.recommend(U, V, d2, exclude=exclude, dtype=dtype)
                pos = np.zeros((d1, d2), np.int64)
                for u in range(d1):
                    n = int((items[u] >= 0).sum())
                    pos[u, items[u, :n]] = np.arange(1, n + 1)
                got, ranks = pcr.evaluate_ranks(U, V, (tindex, titem, tval), exclude=exclude, dtype=dtype, ranks=True)
                users = np.repeat(np.arange(d1), np.diff(tindex))
                assert np.array_equal(ranks, pos[users, titem]) and ranks.min() >= 1, (d1, d2, dtype, exclude is None)
                assert got["relevant"] == titem.shape[0]


@pytest.mark.gpu
@pytest.mark.timeout(1200)
@pytest.mark.parametrize("d1, d2, k", [(40, 21000, 16), (5000, 4000, 32)], ids=["few_users_16_splits", "many_users"])
def test_hits_and_hit_rate_of_evaluate_topn_follow_from_the_ranks(d1, d2, k):
    import primalcr_amd as pcr
    rng = np.random.default_rng(d1)
    U, V = rng.standard_normal((d1, k)), rng.standard_normal((d2, k)) * (1.0 + 3.0 * (rng.random((d2, 1)) < 0.02))
    index, item = random_csr(rng, d1, d2, 0, 40)
    rows = []
    for u in range(d1):                                             # held-out items that are not in the training row; some land high
        top = np.argsort(-(V @ U[u]))[:30]
        cand = np.concatenate([rng.choice(top, 3, replace=False), rng.integers(0, d2, int(rng.integers(0, 9)))])
        rows.append(np.setdiff1d(cand, item[index[u]:index[u + 1]]).astype(np.int32) if u % 9 else np.zeros(0, np.int32))
    tindex = np.zeros(d1 + 1, np.int64); tindex[1:] = np.cumsum([r.shape[0] for r in rows])
    titem = np.concatenate(rows).astype(np.int32)
    tval = rng.integers(1, 6, titem.shape[0]).astype(np.float64)
    cutoffs = (1, 10, 100, 1024)
    for dtype in (0, 1):
        stats, topn = pcr.evaluate_topn(U, V, (tindex, titem, tval), cutoffs=cutoffs, exclude=(index, item), dtype=dtype, per_user=True)
        got, pu, ranks = pcr.evaluate_ranks(U, V, (tindex, titem, tval), exclude=(index, item), dtype=dtype, per_user=True, ranks=True)
        counted = np.diff(tindex) > 0
        assert np.array_equal(~np.isnan(pu[:, 0]), counted) and got["users"] == stats[0]["users"] == int(counted.sum())
        users = np.repeat(np.arange(d1), np.diff(tindex))
        total_hits = 0
        for c, cut in enumerate(cutoffs):
            hits = np.bincount(users[ranks <= cut], minlength=d1)
            assert np.array_equal(topn[counted, c, 0], hits[counted]), cut
            assert stats[c]["hits"] == int(hits.sum())
            assert stats[c]["hit_rate"] == float((pu[counted, 0] <= cut).sum()) / int(counted.sum())
            total_hits += int(hits.sum())
        assert total_hits > 0
        first = np.full(d1, np.iinfo(np.int64).max); np.minimum.at(first, users, ranks)
        assert np.array_equal(pu[counted, 0], first[counted])


@pytest.mark.gpu
@pytest.mark.timeout(1200)
def test_same_ranks_at_every_split_count_and_batch_size():
    """rec_run's split rule: the number of item splits follows from the number of counted users (1 user: 16 splits at d2 >= 16384;
    thousands: fewer) and d2 (below 2048: one).  A user's ranks are the same in every geometry, equal to the brute-force ones, and
    the same when the users go in several batches (pcr_tune ranks_batch_users: the natural batch holds far more users than a test)."""
    import primalcr_amd as pcr
    from test_recommend_grid import only_rows, splits_of
    rng = np.random.default_rng(77)
    for d2, k, d1 in ((2047, 7, 1500), (5000, 16, 1500), (17770, 9, 6000)):
        U = rng.integers(-2, 3, (d1, k)).astype(np.float64)
        V = rng.integers(-2, 3, (d2, k)).astype(np.float64)
        index, item = random_csr(rng, d1, d2, 0, 50)
        tindex, titem, tval = disjoint_test_csr(rng, d1, d2, index, item, 1, 40, empty_every=0)
        sel = np.arange(0, 60, 7)
        S = U[sel] @ V.T
        sub_index = np.zeros(sel.shape[0] + 1, np.int64); sub_index[1:] = np.cumsum(index[sel + 1] - index[sel])
        sub_item = np.concatenate([item[index[u]:index[u + 1]] for u in sel]).astype(np.int32)
        sub_t = np.zeros(sel.shape[0] + 1, np.int64); sub_t[1:] = np.cumsum(tindex[sel + 1] - tindex[sel])
        zs = np.concatenate([np.arange(tindex[u], tindex[u + 1]) for u in sel])
        want_r, want_pu, _ = ref_ranks(S, sub_index, sub_item, sub_t, titem[zs], tval[zs], -math.inf)
        for dtype in (0, 1):
            full, full_pu, full_r = pcr.evaluate_ranks(U, V, (tindex, titem, tval), exclude=(index, item), dtype=dtype, per_user=True, ranks=True)
            assert np.array_equal(full_r[zs], want_r), (d2, dtype)
            check_per_user(full_pu[sel], want_pu)
            seen = {splits_of(d1, d2, 1, dtype)}
            for users in (sel[:1], sel):                            # fewer counted users: more splits
                t = only_rows(tindex, titem, tval, users)
                st, pu, r = pcr.evaluate_ranks(U, V, t, exclude=(index, item), dtype=dtype, per_user=True, ranks=True)
                z = np.concatenate([np.arange(tindex[u], tindex[u + 1]) for u in users])
                assert st["users"] == users.shape[0] and np.array_equal(r, full_r[z]), (d2, dtype, users.shape[0])
                assert np.array_equal(pu[users].view(np.int64), full_pu[users].view(np.int64))
                seen.add(splits_of(users.shape[0], d2, 1, dtype))
            assert seen == {2047: {1}, 5000: {4}, 17770: {16, 11}}[d2], seen
            for cap in (64, 448):                                   # one workgroup per batch; full batches and a short last one
                with pcr.tuned(ranks_batch_users=cap):
                    st, pu, r = pcr.evaluate_ranks(U, V, (tindex, titem, tval), exclude=(index, item), dtype=dtype, per_user=True, ranks=True)
                assert np.array_equal(r, full_r) and np.array_equal(pu.view(np.int64), full_pu.view(np.int64)), (d2, dtype, cap)
                assert st == full


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_relevant_rows_longer_than_the_lds_stage():
    """k_rank_count stages relevant rows of at most RANK_STAGE = 32 entries in LDS and searches longer ones in global memory: rows
    of length 1, 32, 33, 200 and 3000 side by side in one wave, against the brute-force ranks."""
    import primalcr_amd as pcr
    rng = np.random.default_rng(9)
    d1, d2, k = 40, 6000, 7
    lens = [1, RANK_STAGE, RANK_STAGE + 1, 200, 3000, 1, 31, 64]
    U = rng.integers(-3, 4, (d1, k)).astype(np.float64)
    V = rng.integers(-3, 4, (d2, k)).astype(np.float64)
    index, item = random_csr(rng, d1, d2, 0, 300)
    rows = [rng.choice(d2, lens[u % len(lens)], replace=False).astype(np.int32) for u in range(d1)]   # may overlap the training row
    tindex = np.zeros(d1 + 1, np.int64); tindex[1:] = np.cumsum([r.shape[0] for r in rows])
    titem = np.concatenate(rows); tval = np.ones(titem.shape[0])
    S = U @ V.T
    for dtype in (0, 1):
        for exclude in ((index, item), None):
            want_r, want_pu, want = ref_ranks(S, *(exclude or (None, None)), tindex, titem, tval, -math.inf)
            got, pu, ranks = pcr.evaluate_ranks(U, V, (tindex, titem, tval), exclude=exclude, dtype=dtype, per_user=True, ranks=True)
            assert np.array_equal(ranks, want_r), (dtype, exclude is None)
            check_per_user(pu, want_pu); check_summary(got, want)


def _train_data(seed=21):
    from primalcr_amd import synth
    import primalcr_amd as pcr
    R = synth.generate("small", seed=seed)
    return R, pcr.Dataset.from_ratings(R)


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_solver_entry_equals_model_entry_and_leaves_training_alone():
    import primalcr_amd as pcr
    R, ds = _train_data()
    r = 16
    for solver_type in (pcr.PCR_SOLVER_PCRPP, pcr.PCR_SOLVER_CCDR1):
        for prec in (pcr.PCR_F32, pcr.PCR_F64):
            p = pcr.Parameter(k=r, precision=prec, solver_type=solver_type, **{"lambda": 100.0})
            s, t = pcr.Solver(ds, p), pcr.Solver(ds, p)
            if solver_type == pcr.PCR_SOLVER_CCDR1:
                U0, V0 = pcr.initial_col(R.d1, r), np.zeros((R.d2, r))
            else:
                U0, V0 = pcr.initial(R.d1, r), pcr.initial(R.d2, r)
            s.set_factors(U0, V0); t.set_factors(U0, V0)
            s.iterate(2); t.iterate(2)
            U, V = s.get_factors()
            for thr in (-math.inf, 4.0):
                a, apu, ar = s.evaluate_ranks(threshold=thr, per_user=True, ranks=True)
                b, bpu, br = pcr.evaluate_ranks(U, V, ds, exclude=ds, threshold=thr, dtype=prec, per_user=True, ranks=True)
                assert a == b, (solver_type, prec, thr)
                assert np.array_equal(ar, br) and np.array_equal(apu.view(np.int64), bpu.view(np.int64))
                again, again_pu, again_r = s.evaluate_ranks(threshold=thr, per_user=True, ranks=True)
                assert again == a and np.array_equal(again_pu.view(np.int64), apu.view(np.int64)) and np.array_equal(again_r, ar)
                assert a["users"] > 0 and ar.max() <= R.d2
            assert s.evaluate_ranks(exclude_train=False) == pcr.evaluate_ranks(U, V, ds, dtype=prec)
            # training after the calls: bitwise the factors of training without them
            s.iterate(2); t.iterate(2)
            Us, Vs = s.get_factors(); Ut, Vt = t.get_factors()
            assert np.array_equal(Us, Ut) and np.array_equal(Vs, Vt), (solver_type, prec)
            s.close(); t.close()


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_shards_give_their_own_rows_and_partials():
    import primalcr_amd as pcr
    R, ds = _train_data(seed=8)
    idx, it, val = ds.csr(0)
    tidx, tit, tval = ds.csr(1)
    r = 10
    U, V = pcr.initial(R.d1, r), pcr.initial(R.d2, r)
    for prec in (pcr.PCR_F32, pcr.PCR_F64):
        p = pcr.Parameter(k=r, precision=prec, **{"lambda": 100.0})
        one = pcr.Solver(ds, p)
        one.set_factors(U, V)
        want, want_pu, want_r = one.evaluate_ranks(per_user=True, ranks=True)
        one.close()
        cut = [0, 211, R.d1]
        parts, rows, rks = [], [], []
        for rank in range(2):
            a, b = cut[rank], cut[rank + 1]
            dsl = pcr.Dataset.from_csr(b - a, R.d2, idx[a:b + 1] - idx[a], it[idx[a]:idx[b]], val[idx[a]:idx[b]].copy(),
                                       tidx[a:b + 1] - tidx[a], tit[tidx[a]:tidx[b]], tval[tidx[a]:tidx[b]].copy())
            s = pcr.Solver(dsl, p, rank=rank, nranks=2, shard=(a, R.d1))
            s.set_local_only(True)
            s.set_factors_local(U[a:b], V)
            st, pu, rk = s.evaluate_ranks(per_user=True, ranks=True)
            parts.append(st); rows.append(pu); rks.append(rk)
            s.close()
        assert np.array_equal(np.concatenate(rows).view(np.int64), want_pu.view(np.int64))
        assert np.array_equal(np.concatenate(rks), want_r)
        for f in ("users", "users_auc", "relevant"):
            assert sum(q[f] for q in parts) == want[f]
        for f in MEANS:
            wk = "users_auc" if f == "auc" else "users"
            tot = sum(q[f] * q[wk] for q in parts) / want[wk]
            assert tot == pytest.approx(want[f], rel=1e-12, abs=1e-15), f


@pytest.mark.gpu
@pytest.mark.timeout(1800)
def test_netflix_shape_f32():
    """Size-independent properties on the Netflix shape, and rank <= 1024 <=> listed by recommend(K = 1024) on the first users."""
    import primalcr_amd as pcr
    from primalcr_amd import synth
    R = synth.generate_fast("netflix")
    d1, d2, k = R.d1, R.d2, 100
    U = pcr.initial(d1, k).astype(np.float32).astype(np.float64)
    V = (pcr.initial(d2, k) * 0.3).astype(np.float32).astype(np.float64)
    index = np.ascontiguousarray(R.index, np.int64); item = np.ascontiguousarray(R.item, np.int32)
    tindex = np.ascontiguousarray(R.tindex, np.int64); titem = np.ascontiguousarray(R.titem, np.int32)
    tval = np.ascontiguousarray(R.tval, np.float64)
    got, pu, ranks = pcr.evaluate_ranks(U, V, (tindex, titem, tval), exclude=(index, item), dtype=pcr.PCR_F32, per_user=True, ranks=True)
    users = np.repeat(np.arange(d1), np.diff(tindex))
    counted = np.diff(tindex) > 0
    assert np.array_equal(~np.isnan(pu[:, 0]), counted) and got["users"] == int(counted.sum())
    # distinct relevant items per user (a duplicated test item counts once), and the items eligible next to them
    key = users.astype(np.int64) * d2 + titem
    uniq, firstpos = np.unique(key, return_index=True)
    uu, ur = users[firstpos], ranks[firstpos]
    Rn = np.bincount(uu, minlength=d1).astype(np.int64)
    assert got["relevant"] == int(Rn.sum())
    tkey = np.repeat(np.arange(d1, dtype=np.int64), np.diff(index)) * d2 + item
    train_distinct = np.bincount((np.unique(tkey) // d2).astype(np.int64), minlength=d1)
    both = np.bincount((np.intersect1d(uniq, tkey) // d2).astype(np.int64), minlength=d1)
    Nn = d2 - train_distinct - (Rn - both)                          # all items, minus the training row, minus R_u outside it
    assert ranks.min() >= 1 and np.all(ranks <= (Nn + Rn)[users])
    o = np.lexsort((ur, uu))
    same_user = uu[o][1:] == uu[o][:-1]
    assert not np.any(same_user & (ur[o][1:] == ur[o][:-1]))        # ranks of one user's relevant items pairwise distinct
    tot = np.bincount(uu, weights=ur.astype(np.float64), minlength=d1).astype(np.int64)   # (exact: below 2^53)
    ok = counted & (Nn > 0)
    assert got["users_auc"] == int(ok.sum())
    auc = pu[ok, 3]
    assert np.all((auc >= 0.0) & (auc <= 1.0))
    want = 1.0 - (tot[ok] - Rn[ok] - Rn[ok] * (Rn[ok] - 1) / 2) / (Rn[ok] * Nn[ok])
    np.testing.assert_allclose(auc, want, rtol=0, atol=1e-12)
    first = np.full(d1, np.iinfo(np.int64).max); np.minimum.at(first, users, ranks)
    assert np.array_equal(pu[counted, 0], first[counted]) and np.array_equal(pu[counted, 2], (tot[counted] / Rn[counted]))
    assert got["mrr"] == pytest.approx(float((1.0 / first[counted]).sum()) / int(counted.sum()), rel=1e-12)
    # the cross-check needs train and test disjoint: the counted users among the first 3000 whose rows are
    n = 3000
    sample = np.nonzero((both[:n] == 0) & counted[:n])[0].astype(np.int32)
    assert sample.shape[0] > 1000
    items, _ = pcr.recommend(U, V, 1024, exclude=(index, item), users=sample, dtype=pcr.PCR_F32)
    for i, u in enumerate(sample):
        z = slice(tindex[u], tindex[u + 1])
        assert np.array_equal(ranks[z] <= 1024, np.isin(titem[z], items[i])), u
        listed = ranks[z] <= 1024
        assert np.array_equal(items[i][ranks[z][listed] - 1], titem[z][listed])


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_cli_end_to_end(tmp_path):
    import primalcr_amd as pcr
    from primalcr_amd import synth
    R = synth.generate("small", seed=13)
    d = synth.write_dir(R, str(tmp_path / "data"))
    out = run([TRAIN, "-k", "8", "-t", "2", "-l", "100", d, "m.model"], tmp_path)
    assert out.returncode == 0, out.stderr
    U, V = pcr.model_load(str(tmp_path / "m.model"))
    ds = pcr.Dataset.load(d)
    plain = run([RECOMMEND, "--eval", d, "-x", d, "-c", "5,10,20", "m.model"], tmp_path)
    assert plain.returncode == 0, plain.stderr
    r = run([RECOMMEND, "--eval", d, "-x", d, "-c", "5,10,20", "--ranks", "m.model", "per_user.txt"], tmp_path)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[:-1] == plain.stdout.splitlines() and len(lines) == 4           # the cutoff lines are unchanged
    want, pu = pcr.evaluate_ranks(U, V, ds, exclude=ds, per_user=True)
    f = lines[-1].split()
    assert f[0] == "ranks"
    assert f[1::2] == ["users", "users_auc", "relevant", "mrr", "mean_rank", "auc", "mpr"]
    for key, v in zip(f[1::2], f[2::2]):
        assert float(v) == float(f"{want[key]:g}"), (key, v, want)
    rows = (tmp_path / "per_user.txt").read_text().splitlines()
    counted = np.nonzero(~np.isnan(pu[:, 0]))[0]
    assert len(rows) == counted.shape[0] > 0
    for line, u in zip(rows, counted):
        g = line.split()
        assert int(g[0]) == u + 1
        got = [float(x) for x in g[1:]]
        exp = [float(f"{v:g}") for v in pu[u]]
        assert len(got) == 5 and all((a == b) or (math.isnan(a) and math.isnan(b)) for a, b in zip(got, exp))
    r = run([RECOMMEND, "--eval", d, "-K", "7", "--threshold", "4", "--f32", "--ranks", "m.model"], tmp_path)
    assert r.returncode == 0, r.stderr
    want = pcr.evaluate_ranks(U, V, ds, threshold=4.0, dtype=pcr.PCR_F32)
    f = r.stdout.splitlines()[-1].split()
    for key, v in zip(f[1::2], f[2::2]):
        assert float(v) == float(f"{want[key]:g}"), (key, v, want)
