"""Top-K recommendation and top-N evaluation across the launch geometries of rec_run (primalcr_amd/csrc/pcr_serve.hip).

rec_run splits the catalogue across workgroups (1 to 16 item splits, merged by rank counting in k_rec_merge /
k_rec_merge_topn) and runs the users in batches whose partial lists fit its scratch.  include/primalcr.h promises that a
list depends on (u, j) alone, not on the other users of the call, their order or the launch grid.  rec_geometry() mirrors
rec_run's arithmetic; every GPU test asserts that its shapes reach the geometry it claims.

CPU part: the mirror's constants against the source, the batch and split counts the GPU tests rely on.
GPU part (-m gpu): exact rankings at every split count with exclusion rows built around the split boundaries, bitwise grid
invariance on real-valued factors, top-N evaluation across geometries, multi-batch runs (the shrink loop and the clamped
short last batch) and live solvers with split catalogues.
"""
import math
import os
import re
from collections import namedtuple

import numpy as np
import pytest

from conftest import ROOT
from test_recommend import check_real, excl_mask, ref_topk
from test_topn_eval import check_per_user, check_summary, make_test_csr, ref_metrics

# rec_run's launch arithmetic.  Copied constants: REC_SCRATCH, REC_TARGET_WG, REC_MAX_SPLIT, REC_MIN_SPLIT_ITEMS
# (pcr_serve.hip) and rec::WAVES * rec::UW users per workgroup, rec::TILE items per step (pcr_topk.h);
# test_geometry_mirror_matches_the_source keeps them in step.
REC_SCRATCH = 1 << 30
REC_TARGET_WG, REC_MAX_SPLIT, REC_MIN_SPLIT_ITEMS = 1024, 16, 1024
REC_WAVES, REC_UW, REC_TILE = 4, 16, 64
USERS_PER_WG = REC_WAVES * REC_UW

Batch = namedtuple("Batch", "b0 users fit splits per")   # fit: splits the batch alone would take; splits: splits launched


def rec_geometry(n, d2, K, dtype):
    """The batches of rec_run for n users, d2 items, top K, dtype 0 (f32) / 1 (f64): [Batch(b0, users, fit, splits, per)]."""
    per_user = K * ((4 if dtype == 0 else 8) + 4) + 4

    def splits_for(users):
        wg = -(-users // USERS_PER_WG)
        s = max(1, -(-REC_TARGET_WG // wg))
        return min(s, max(1, d2 // REC_MIN_SPLIT_ITEMS), REC_MAX_SPLIT)

    nb = min(n, max(USERS_PER_WG, REC_SCRATCH // (per_user * 2) // USERS_PER_WG * USERS_PER_WG))
    while nb > USERS_PER_WG and nb * splits_for(nb) * per_user > REC_SCRATCH:
        nb = max(USERS_PER_WG, nb // 2)
    smax = splits_for(min(nb, n))
    out = []
    for b0 in range(0, n, nb):
        m = min(nb, n - b0)
        ns = min(splits_for(m), smax)
        per = -(-(-(-d2 // ns)) // REC_TILE) * REC_TILE
        out.append(Batch(b0, m, splits_for(m), -(-d2 // per), per))
    return out


def splits_of(n, d2, K, dtype):
    """The split count of a single-batch call."""
    g = rec_geometry(n, d2, K, dtype)
    assert len(g) == 1, g
    return g[0].splits


def boundaries(d2, per):
    return list(range(per, d2, per))


def csr_of(rows):
    index = np.zeros(len(rows) + 1, np.int64)
    index[1:] = np.cumsum([r.shape[0] for r in rows])
    return index, (np.concatenate(rows) if rows else np.zeros(0)).astype(np.int32)


def boundary_row(u, d2, per):
    """Exclusion row of user u around the split boundaries of split width per (item-ascending, duplicates allowed).
    u % 8: 0 items jb - 1, jb, jb + 1 of every boundary jb (jb doubled); 1 every item of one whole split (its partial list is
    empty); 2 everything but the last third of the last split (fewer eligible items than K = 1024); 3 every item (all
    padding); 4 nothing; 5 a whole split and the neighbours of every other boundary; 6, 7 a few items around one boundary."""
    nsp = -(-d2 // per)
    jbs = boundaries(d2, per)
    t = u % 8
    if t == 0:
        r = [0, d2 - 1] + [j for jb in jbs for j in (jb - 1, jb, jb, jb + 1)]
    elif t == 1 or t == 5:
        s = (u // 8) % nsp
        r = list(range(s * per, min(d2, (s + 1) * per)))
        if t == 5:
            r += [j for i, jb in enumerate(jbs) if i % 2 for j in (jb - 1, jb + 1)]
    elif t == 2:
        jl = (nsp - 1) * per
        r = list(range(0, d2 - (d2 - jl) // 3))
    elif t == 3:
        r = list(range(d2))
    elif t == 4:
        r = []
    else:
        jb = jbs[(u // 8) % len(jbs)] if jbs else d2 // 2
        r = [j for j in (jb - 2, jb - 1, jb, jb + 3, 5, 5) if 0 <= j < d2]
    return np.sort(np.array(r, np.int32))


def boundary_csr(d1, d2, per):
    return csr_of([boundary_row(u, d2, per) for u in range(d1)])


def random_csr(rng, d1, d2, special=None, lo=0, hi=12):
    """d1 rows of lo..hi-1 random items (duplicates allowed), item-ascending; special: {user: row} replaces those rows."""
    cnt = rng.integers(lo, hi, d1)
    for u, r in (special or {}).items():
        cnt[u] = r.shape[0]
    index = np.zeros(d1 + 1, np.int64)
    index[1:] = np.cumsum(cnt)
    item = rng.integers(0, d2, int(index[-1])).astype(np.int32)
    for u, r in (special or {}).items():
        item[index[u]:index[u + 1]] = r
    row = np.repeat(np.arange(d1), cnt)
    item = item[np.lexsort((item, row))]
    return index, item


def mask_rows(index, item, users, d2):
    """excl_mask of the given users only."""
    M = np.zeros((len(users), d2), bool)
    for i, u in enumerate(users):
        M[i, item[index[u]:index[u + 1]]] = True
    return M


def shuffled_rows(rng, index, item):
    out = item.copy()
    for u in range(index.shape[0] - 1):
        rng.shuffle(out[index[u]:index[u + 1]])
    return out


def int_factors(rng, n, k, lo=-2, hi=2):
    return rng.integers(lo, hi + 1, (n, k)).astype(np.float64)


def sub_test_csr(tindex, titem, tval, users):
    """The test rows of the given users, in that order: (index, item, val) over len(users) rows."""
    users = np.asarray(users)
    idx = np.zeros(users.shape[0] + 1, np.int64)
    idx[1:] = np.cumsum(tindex[users + 1] - tindex[users])
    sel = np.concatenate([np.arange(tindex[u], tindex[u + 1]) for u in users]).astype(np.int64)
    return idx, titem[sel], tval[sel]


def only_rows(tindex, titem, tval, users):
    """The test CSR with every row outside `users` emptied (same d1)."""
    keep = np.zeros(tindex.shape[0] - 1, bool)
    keep[users] = True
    cnt = np.where(keep, np.diff(tindex), 0)
    idx = np.zeros_like(tindex)
    idx[1:] = np.cumsum(cnt)
    sel = np.concatenate([np.arange(tindex[u], tindex[u + 1]) for u in np.nonzero(keep)[0]]).astype(np.int64)
    return idx, titem[sel], tval[sel]


def same_bits(a, b):
    """(items, scores) pairs equal bitwise."""
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int64), b[1].view(np.int64))


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_geometry_mirror_matches_the_source():
    src = open(os.path.join(ROOT, "primalcr_amd", "csrc", "pcr_serve.hip")).read()
    assert re.search(r"REC_SCRATCH = \(size_t\)1 << 30;", src)
    m = re.search(r"REC_TARGET_WG = (\d+), REC_MAX_SPLIT = (\d+), REC_MIN_SPLIT_ITEMS = (\d+);", src)
    assert m and tuple(int(x) for x in m.groups()) == (REC_TARGET_WG, REC_MAX_SPLIT, REC_MIN_SPLIT_ITEMS)
    topk = open(os.path.join(ROOT, "primalcr_amd", "csrc", "pcr_topk.h")).read()
    for name, v in (("WAVES", REC_WAVES), ("UW", REC_UW), ("NQ", REC_TILE // 16)):
        assert re.search(rf"constexpr int {name} = {v};", topk), name
    assert "constexpr int TILE = 16 * NQ;" in topk
    # the geometries the GPU tests below claim
    assert [splits_of(1, d2, 1024, 1) for d2 in (2047, 2048, 5000, 5120, 16385, 17770, 40000)] == [1, 2, 4, 5, 16, 16, 16]
    g = rec_geometry(1, 16385, 10, 0)[0]
    assert (g.per, 16385 - 15 * g.per) == (1088, 65)
    g = rec_geometry(1, 17770, 10, 0)[0]
    assert (g.per, 17770 - 15 * g.per) == (1152, 490)
    assert splits_of(2000, 5000, 10, 0) == 4
    for dtype in (0, 1):
        assert splits_of(6000, 17770, 1024, dtype) == 11 and splits_of(20000, 17770, 1024, dtype) == 4
        assert splits_of(6040, 17770, 1024, dtype) == 11 and splits_of(40, 17770, 1024, dtype) == 16
    assert [(b.b0, b.users, b.fit, b.splits) for b in rec_geometry(30000, 5120, 1024, 1)] == [(0, 15000, 5, 5), (15000, 15000, 5, 5)]
    assert [(b.b0, b.users, b.fit, b.splits) for b in rec_geometry(44000, 5120, 1024, 1)] == [(0, 43648, 2, 2), (43648, 352, 5, 2)]


# ---------------------------------------------------------------------------------------------------------------- GPU
# A: (d2, k, value range, [(n, K), ...]); n = 1 runs once for every exclusion type of boundary_row
A_CASES = [
    (2047, 7, 2, [(1, 1024), (65, 1024), (16, 1), (200, 100)]),
    (2048, 7, 2, [(1, 1024), (65, 1024), (17, 10), (64, 1)]),
    (5000, 16, 2, [(1, 1024), (65, 1024), (2000, 10), (15, 100)]),
    (5120, 16, 2, [(1, 1024), (65, 100)]),
    (16385, 64, 2, [(1, 1024), (65, 1024), (15, 10), (16, 100)]),
    (17770, 1, 1, [(1, 1024), (65, 1024), (17, 1), (64, 100)]),
    (17770, 9, 2, [(1, 1024), (65, 1024), (200, 10)]),
    (40000, 5, 2, [(1, 1024), (65, 1024), (64, 1)]),
]


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
def test_exact_rankings_at_every_split_count(dtype):
    import primalcr_amd as pcr
    rng = np.random.default_rng(41 + dtype)
    seen, empty_split, padded, all_padding = set(), False, False, False
    for d2, k, vr, combos in A_CASES:
        d1 = max(n for n, _ in combos)
        per = rec_geometry(1, d2, 1024, dtype)[0].per
        U = int_factors(rng, d1, k, -vr, vr)
        V = int_factors(rng, d2, k, -vr, vr)
        if k == 1:                                     # whole splits tie: split 1 all +1, split 2 all -1, user 0's scores all 0
            V[per:2 * per] = 1.0; V[2 * per:3 * per] = -1.0; U[0] = 0.0
        index, item = boundary_csr(d1, d2, per)
        M = excl_mask(d1, d2, index, item)
        none = np.zeros((1, d2), bool)
        for n, K in combos:
            calls = [np.array([u], np.int32) for u in range(8)] if n == 1 else [rng.permutation(d1)[:n].astype(np.int32)]
            for users in calls:
                g = rec_geometry(n, d2, K, dtype)
                assert len(g) == 1 and g[0].per == per
                seen.add(g[0].splits)
                S = U[users] @ V.T                     # exact: |s| <= 4 k
                gi, gs = pcr.recommend(U, V, K, exclude=(index, item), users=users, dtype=dtype)
                ri, rs = ref_topk(S, M[users], K)
                assert np.array_equal(gi, ri), (d2, k, n, K, users[:3])
                assert np.array_equal(gs, rs), (d2, k, n, K, users[:3])
                if g[0].splits > 1 and any(u % 8 == 1 for u in users):
                    empty_split = True
                if K == 1024:
                    padded |= bool(((ri[:, 0] >= 0) & (ri[:, -1] < 0)).any())
                    all_padding |= bool((ri[:, 0] < 0).any())
                if n == 1 and users[0] == 0:
                    gi, gs = pcr.recommend(U, V, K, users=users, dtype=dtype)
                    ri, rs = ref_topk(S, none, K)
                    assert np.array_equal(gi, ri) and np.array_equal(gs, rs), (d2, k, K, "no exclusion")
                if n == 65 and K == 1024:               # rows not item-ascending: the same lists
                    b = pcr.recommend(U, V, K, exclude=(index, shuffled_rows(rng, index, item)), users=users, dtype=dtype)
                    assert np.array_equal(b[0], gi) and np.array_equal(b[1], gs)
    assert {1, 2, 4, 5, 16} <= seen and empty_split and padded and all_padding, (seen, empty_split, padded, all_padding)


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
def test_grid_invariance_bitwise(dtype):
    import primalcr_amd as pcr
    rng = np.random.default_rng(51 + dtype)
    d1, d2, k, K = 20000, 17770, 24, 1024
    U, V = pcr.initial(d1, k), pcr.initial(d2, k) * 0.5
    if dtype == 0:
        U, V = U.astype(np.float32).astype(np.float64), V.astype(np.float32).astype(np.float64)
    per16 = rec_geometry(1, d2, K, dtype)[0].per
    special = {u: boundary_row(u, d2, per16) for u in range(0, d1, 997)}
    index, item = random_csr(rng, d1, d2, special)
    ex = (index, item)
    assert splits_of(d1, d2, K, dtype) == 4
    full = pcr.recommend(U, V, K, exclude=ex, dtype=dtype)
    first = np.arange(6000, dtype=np.int32)
    assert splits_of(6000, d2, K, dtype) == 11
    a = pcr.recommend(U, V, K, exclude=ex, users=first, dtype=dtype)
    assert same_bits(a, (full[0][first], full[1][first]))
    rev = first[::-1].copy()
    a = pcr.recommend(U, V, K, exclude=ex, users=rev, dtype=dtype)
    assert same_bits(a, (full[0][rev], full[1][rev]))
    assert splits_of(1, d2, K, dtype) == 16
    one = np.concatenate([np.array(sorted(special))[:8], rng.choice(d1, 8, replace=False)]).astype(np.int32)
    gi, gs = np.empty((one.shape[0], K), np.int32), np.empty((one.shape[0], K))
    for i, u in enumerate(one):
        gi[i], gs[i] = (x[0] for x in pcr.recommend(U, V, K, exclude=ex, users=np.array([u], np.int32), dtype=dtype))
    assert same_bits((gi, gs), (full[0][one], full[1][one]))
    check_real(U[one], V, mask_rows(index, item, one, d2), gi, gs, K, dtype == 0)


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
def test_topn_across_geometries(dtype):
    """A few counted users (16 splits) against the same users inside a call that counts all of them (11 splits): per-user rows
    bitwise equal, and equal to numpy's metrics on the exact lists."""
    import primalcr_amd as pcr
    rng = np.random.default_rng(61 + dtype)
    d1, d2, k, cutoffs = 6000, 17770, 9, (1, 10, 100, 1024)
    K = cutoffs[-1]
    U, V = int_factors(rng, d1, k), int_factors(rng, d2, k)
    per16 = rec_geometry(1, d2, K, dtype)[0].per
    sel = np.sort(np.concatenate([np.arange(8, 24), rng.choice(np.arange(24, d1), 24, replace=False)])).astype(np.int32)
    index, item = random_csr(rng, d1, d2, {int(u): boundary_row(int(u), d2, per16) for u in sel})
    tindex, titem, tval = make_test_csr(rng, d1, d2, index, item, empty_every=d1 + 1)   # only user 2 without test rows
    few = only_rows(tindex, titem, tval, sel)
    others = np.ones(d1, bool); others[sel] = False
    for exclude in ((index, item), None):
        items, scores = pcr.recommend(U, V, K, exclude=exclude, users=sel, dtype=dtype)
        M = mask_rows(index, item, sel, d2) if exclude else np.zeros((sel.shape[0], d2), bool)
        ri, rs = ref_topk(U[sel] @ V.T, M, K)
        assert np.array_equal(items, ri) and np.array_equal(scores, rs)
        for thr in (-math.inf, 4.0):
            full, full_pu = pcr.evaluate_topn(U, V, (tindex, titem, tval), cutoffs=cutoffs, exclude=exclude, threshold=thr, dtype=dtype,
                                              per_user=True)
            got, pu = pcr.evaluate_topn(U, V, few, cutoffs=cutoffs, exclude=exclude, threshold=thr, dtype=dtype, per_user=True)
            if thr == -math.inf:
                assert full[0]["users"] == d1 - 1 and splits_of(d1 - 1, d2, K, dtype) == 11
            assert 0 < got[0]["users"] <= sel.shape[0] and splits_of(got[0]["users"], d2, K, dtype) == 16
            assert np.array_equal(pu[sel].view(np.int64), full_pu[sel].view(np.int64)), (exclude is None, thr)
            assert np.isnan(pu[others]).all()
            want_pu, want = ref_metrics(items, *sub_test_csr(tindex, titem, tval, sel), cutoffs, thr)
            check_per_user(pu[sel], want_pu)
            check_summary(got, want)


# D: (users, first batch) of the two multi-batch shapes at d2 = 5120, K = 1024, f64
D_CASES = [(30000, [(0, 15000, 5, 5), (15000, 15000, 5, 5)]), (44000, [(0, 43648, 2, 2), (43648, 352, 5, 2)])]


@pytest.mark.gpu
@pytest.mark.timeout(1200)
@pytest.mark.parametrize("n, batches", D_CASES, ids=["shrink_loop", "clamped_last_batch"])
def test_user_batches(n, batches):
    """Several user batches at their natural size: rows around every batch boundary equal single-batch calls bitwise and
    numpy's exact lists; the top-N rows there equal a single-batch evaluation, the summaries numpy's over all users."""
    import primalcr_amd as pcr
    rng = np.random.default_rng(n)
    d2, k, K, dtype, cutoffs = 5120, 8, 1024, 1, (1, 10, 100, 1024)
    g = rec_geometry(n, d2, K, dtype)
    assert [(b.b0, b.users, b.fit, b.splits) for b in g] == batches
    U, V = int_factors(rng, n, k), int_factors(rng, d2, k)
    rows = set(range(10)) | set(range(n - 10, n)) | set(int(u) for u in rng.choice(n, 40, replace=False))
    for b in g[1:]:
        rows |= set(range(b.b0 - 10, b.b0 + 10))
    rows = np.array(sorted(rows), np.int32)
    index, item = random_csr(rng, n, d2, {int(u): boundary_row(int(u), d2, g[0].per) for u in rows})
    ex = (index, item)
    full = pcr.recommend(U, V, K, exclude=ex, dtype=dtype)
    assert splits_of(rows.shape[0], d2, K, dtype) == 5
    part = pcr.recommend(U, V, K, exclude=ex, users=rows, dtype=dtype)
    assert same_bits(part, (full[0][rows], full[1][rows]))
    ri, rs = ref_topk(U[rows] @ V.T, mask_rows(index, item, rows, d2), K)
    assert np.array_equal(part[0], ri) and np.array_equal(part[1], rs)
    # every user has a relevant test rating: the evaluation counts n users and runs the same batches
    cnt = rng.integers(1, 4, n)
    tindex = np.zeros(n + 1, np.int64); tindex[1:] = np.cumsum(cnt)
    titem = rng.integers(0, d2, int(tindex[-1])).astype(np.int32)
    tval = rng.integers(1, 6, int(tindex[-1])).astype(np.float64)
    got, pu = pcr.evaluate_topn(U, V, (tindex, titem, tval), cutoffs=cutoffs, exclude=ex, dtype=dtype, per_user=True)
    assert got[0]["users"] == n
    one, one_pu = pcr.evaluate_topn(U, V, only_rows(tindex, titem, tval, rows), cutoffs=cutoffs, exclude=ex, dtype=dtype, per_user=True)
    assert one[0]["users"] == rows.shape[0]
    assert np.array_equal(one_pu[rows].view(np.int64), pu[rows].view(np.int64))
    want_pu, want = ref_metrics(full[0], tindex, titem, tval, cutoffs, -math.inf)
    check_per_user(pu[rows], want_pu[rows])
    check_summary(got, want)


def _grid_data(seed=71):
    import primalcr_amd as pcr
    from primalcr_amd import synth
    R = synth.generate("small", seed=seed, d1=6040, d2=17770, nnz=200000)
    return R, pcr.Dataset.from_ratings(R)


@pytest.mark.gpu
@pytest.mark.timeout(1200)
def test_live_solvers_with_split_catalogues():
    """Solver.recommend / Solver.evaluate_topn with 11 and 16 splits against the model entry on get_factors(), local-only
    shards of 40 and 6000 users (16 and 11 splits; PCR++ only: CCDR1 runs on one rank) and training afterwards."""
    import primalcr_amd as pcr
    R, ds = _grid_data()
    idx, it, val = ds.csr(0)
    tidx, tit, tval = ds.csr(1)
    rng = np.random.default_rng(7)
    r, K, cutoffs = 16, 1024, (1, 10, 100, 1024)
    for solver_type in (pcr.PCR_SOLVER_PCRPP, pcr.PCR_SOLVER_CCDR1):
        for prec in (pcr.PCR_F32, pcr.PCR_F64):
            what = (solver_type, prec)
            p = pcr.Parameter(k=r, precision=prec, solver_type=solver_type, **{"lambda": 100.0})
            s, t = pcr.Solver(ds, p), pcr.Solver(ds, p)
            if solver_type == pcr.PCR_SOLVER_CCDR1:
                U0, V0 = pcr.initial_col(R.d1, r), np.zeros((R.d2, r))
            else:
                U0, V0 = pcr.initial(R.d1, r), pcr.initial(R.d2, r)
            s.set_factors(U0, V0); t.set_factors(U0, V0)
            s.iterate(1); t.iterate(1)
            U, V = s.get_factors()
            assert splits_of(R.d1, R.d2, K, prec) == 11
            full = s.recommend(K)
            assert same_bits(full, pcr.recommend(U, V, K, exclude=ds, dtype=prec)), what
            for n in (1, 17, 65):
                users = rng.choice(R.d1, n, replace=False).astype(np.int32)
                assert splits_of(n, R.d2, K, prec) == 16
                a = s.recommend(K, users=users)
                assert same_bits(a, pcr.recommend(U, V, K, exclude=ds, users=users, dtype=prec)), (what, n)
                assert same_bits(a, (full[0][users], full[1][users])), (what, n)
            for thr in (-math.inf, 4.0):
                a, apu = s.evaluate_topn(cutoffs, threshold=thr, per_user=True)
                b, bpu = pcr.evaluate_topn(U, V, ds, cutoffs=cutoffs, exclude=ds, threshold=thr, dtype=prec, per_user=True)
                assert a == b and np.array_equal(apu.view(np.int64), bpu.view(np.int64)), (what, thr)
                if thr == -math.inf:
                    assert a[0]["users"] == R.d1
                    want = (a, apu)
            if solver_type == pcr.PCR_SOLVER_PCRPP:
                cut = [0, 40, R.d1]
                parts, rows, recs = [], [], []
                for rank in range(2):
                    lo, hi = cut[rank], cut[rank + 1]
                    assert splits_of(hi - lo, R.d2, K, prec) == (16, 11)[rank]
                    dsl = pcr.Dataset.from_csr(hi - lo, R.d2, idx[lo:hi + 1] - idx[lo], it[idx[lo]:idx[hi]], val[idx[lo]:idx[hi]].copy(),
                                               tidx[lo:hi + 1] - tidx[lo], tit[tidx[lo]:tidx[hi]], tval[tidx[lo]:tidx[hi]].copy())
                    sh = pcr.Solver(dsl, p, rank=rank, nranks=2, shard=(lo, R.d1))
                    sh.set_local_only(True)
                    sh.set_factors_local(U[lo:hi], V)
                    st, pu = sh.evaluate_topn(cutoffs, per_user=True)
                    assert st[0]["users"] == hi - lo
                    parts.append(st); rows.append(pu); recs.append(sh.recommend(K))
                    sh.close()
                assert np.array_equal(np.concatenate(rows).view(np.int64), want[1].view(np.int64)), what
                assert same_bits((np.concatenate([x[0] for x in recs]), np.concatenate([x[1] for x in recs])), full), what
                for c in range(len(cutoffs)):
                    for f in ("users", "users_graded", "hits"):
                        assert sum(q[c][f] for q in parts) == want[0][c][f]
                    for f in ("precision", "recall", "hit_rate", "map", "ndcg", "ndcg_graded"):
                        wk = "users_graded" if f == "ndcg_graded" else "users"
                        tot = sum(q[c][f] * q[c][wk] for q in parts) / want[0][c][wk]
                        assert tot == pytest.approx(want[0][c][f], rel=1e-12, abs=1e-15), (what, f)
            # training after the calls: bitwise the factors of training without them
            s.iterate(1); t.iterate(1)
            Us, Vs = s.get_factors(); Ut, Vt = t.get_factors()
            assert np.array_equal(Us, Ut) and np.array_equal(Vs, Vt), what
            s.close(); t.close()
