"""explain_ridge() / Solver.explain_ridge() / omp-pmf-recommend --explain-ridge (include/primalcr.h, "explaining squared-loss
recommendations"): the score of a squared-loss row split into rating x similarity through the inverse of the user's
regularised Gram matrix, against the plain-numpy fp64 reference of tests/explain_ridge_ref.py.

Exact part: systems whose Gram matrix is diagonal with entries 4 or 16, so the Cholesky factor, both solves, every contribution
and every sum are exact in any order; the device must match bit for bit (the sign of a zero is not compared).
General part: Gaussian factors with cond(G) <= 1e3, every entry held to 1e-10 |r_p| |v_p| |v_j| / mu: |G^-1| <= 1 / mu, the
worst-case relative error of a Cholesky solve is of order k 2^-52 cond(G) (2.5e-11 at k = 112 and the fixture's cap), and numpy's own
error is orders below that.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import primalcr_amd as pcr
from primalcr_amd import synth
from conftest import BIN_DIR, ROOT
import explain_ridge_ref as xr

ERR_ARG, ERR_STATE, ERR_DEVICE, ERR_UNSUPPORTED = -1, -6, -4, -7
PREC = {"F64": pcr.PCR_F64, "F32": pcr.PCR_F32}
RECOMMEND = os.path.join(BIN_DIR, "omp-pmf-recommend")
PAIR = {f: i for i, f in enumerate(pcr.PCR_EXPLAIN_PAIR_FIELDS)}
USER = {f: i for i, f in enumerate(pcr.PCR_EXPLAIN_RIDGE_USER_FIELDS)}


def bits(x):
    """The bit patterns of x with -0.0 folded onto +0.0 (NaNs of the padding compare equal: one pattern on both sides)."""
    x = np.asarray(x, np.float64) + 0.0
    return np.where(np.isnan(x), np.int64(-1), x.view(np.int64))


def assert_same_bits(got, want, what):
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.shape[0] == 0, f"{what}: {bad.shape[0]} entries differ, first at {bad[0]}: {np.asarray(got)[tuple(bad[0])]!r} != {np.asarray(want)[tuple(bad[0])]!r}"


def same(x, y):
    return np.array_equal(x.view(np.int64) if x.dtype == np.float64 else x, y.view(np.int64) if y.dtype == np.float64 else y)


def sub_csr(ratings, users):
    idx, item, val = ratings
    lens = np.diff(idx)[users]
    return (np.concatenate([[0], np.cumsum(lens)]).astype(np.int64),
            np.concatenate([item[idx[i]:idx[i + 1]] for i in users] + [np.zeros(0, np.int32)]).astype(np.int32),
            np.concatenate([val[idx[i]:idx[i + 1]] for i in users] + [np.zeros(0)]))


def run(F, ratings, U, lists, lam, top, pname, **kw):
    return pcr.explain_ridge(F, ratings, U, lists, lam, top=top, dtype=PREC[pname], per_pair=True, per_user=True, **kw)


# ------------------------------------------------------------------------------------------------ the diagonal fixture
def diagonal_case(k, weighted, seed):
    """Rated rows with ONE nonzero +-1 or +-2; per user and coordinate three rated rows of magnitude 2, or twelve of magnitude 1,
    or none, so A^T A is diagonal with entries 12 or 0 and, with mu = 4, G has entries 16 or 4.  Plain: lambda = 4.  Weighted:
    lambda = 1 / 4 at len = 16 -- twelve rows on one coordinate, three on another and ONE rated item whose row of F is all zeros
    (a row count under this recipe is a multiple of 3: a square of a power of two is 1 mod 3 and they sum to 12; the zero row
    contributes nothing to G and exactly 0 to every score).  The rows hold repeated items and are not sorted; ratings are integers
    in -2 .. 5; the listed rows are dense multiples of 1/4; the lists hold ids from the row, ids twice, trailing -1 and all -1."""
    rng = np.random.default_rng(seed)
    per, dense, n, L = 6, 24, 30, 20
    d2 = 2 * per * k + dense + 1
    F = np.zeros((d2, k))
    pool = {}
    for t in range(k):
        for m, mag in enumerate((1.0, 2.0)):
            ids = np.arange(per) + (2 * t + m) * per
            F[ids, t] = mag * rng.choice([-1.0, 1.0], size=per)
            pool[t, mag] = ids
    dense0 = 2 * per * k
    F[dense0:dense0 + dense] = rng.integers(-8, 9, size=(dense, k)) / 4.0
    zero_item = d2 - 1
    idx, item = [0], []
    for i in range(n):
        row = []
        if weighted:
            t1, t2 = rng.choice(k, size=2, replace=False) if k > 1 else (0, 0)
            if k > 1:
                row += list(rng.choice(pool[t1, 1.0], size=12)) + list(rng.choice(pool[t2, 2.0], size=3)) + [zero_item]
            else:
                row += list(rng.choice(pool[0, 1.0], size=12 if i % 2 else 0)) + list(rng.choice(pool[0, 2.0], size=0 if i % 2 else 3))
                row += [zero_item] * (16 - len(row))
        elif i % 7 != 3:                                               # (plain: every seventh user has no ratings)
            for t in range(k):
                mode = rng.integers(0, 3)
                if mode == 1:
                    row += list(rng.choice(pool[t, 2.0], size=3))
                elif mode == 2:
                    row += list(rng.choice(pool[t, 1.0], size=12))
        row = list(rng.permutation(row)) if row else row
        item += row
        idx.append(len(item))
    idx, item = np.array(idx, np.int64), np.array(item, np.int32)
    val = rng.integers(-2, 6, size=len(item)).astype(np.float64)
    lists = rng.integers(dense0, dense0 + dense, size=(n, L)).astype(np.int32)
    for i in range(n):
        a, b = int(idx[i]), int(idx[i + 1])
        lists[i, 2] = lists[i, 0]
        if b > a:
            lists[i, 1] = item[a + (b - a) // 2]
            lists[i, 5] = item[a]
        keep = 0 if i % 5 == 4 else L - (i % 4)
        lists[i, keep:] = -1
    U = rng.integers(-8, 9, size=(n, k)) / 4.0
    return F, (idx, item, val), U, lists, (0.25 if weighted else 4.0)


def test_the_diagonal_fixture_is_exact_in_the_reference():
    """G is diagonal with entries 4 or 16, every e_p equals r_p v_pt v_jt / G_tt computed directly, and there are hundreds of ties."""
    ties = 0
    for k, weighted in ((5, False), (5, True), (40, False), (1, True)):
        F, ratings, U, lists, lam = diagonal_case(k, weighted, 11 + k)
        ref = xr.ref_explain_ridge(F, ratings, U, lists, lam, weighted=weighted)
        for i, u in enumerate(ref):
            if len(u["items"]) == 0:
                continue
            assert u["mu"] == 4.0 and (not weighted or len(u["items"]) == 16)
            G, _ = xr.user_system(F, u["items"], lam, weighted, u["P"])
            assert np.array_equal(G, np.diag(np.diag(G))) and set(np.diag(G)) <= {4.0, 16.0}
            lst = lists[i][lists[i] >= 0]
            direct = u["r"][:, None] * ((F[u["items"]] / np.diag(G)) @ F[lst].T)
            assert np.array_equal(u["e"], direct)
            assert np.array_equal(u["e"].sum(axis=0), F[lst] @ u["ustar"])
            ties += int((np.diff(np.sort(u["e"], axis=0), axis=0) == 0).sum())
    assert ties > 300


@pytest.mark.gpu
@pytest.mark.parametrize("pname", ["F64", "F32"])
@pytest.mark.parametrize("weighted", [False, True])
def test_a_diagonal_system_is_explained_bit_for_bit(weighted, pname):
    for k in (1, 5, 40):
        F, ratings, U, lists, lam = diagonal_case(k, weighted, 11 + k)
        for rows in (U, None):
            ref = xr.ref_explain_ridge(F, ratings, rows, lists, lam, weighted=weighted)
            for top in (16, 3):
                items, contrib, stats, pp, pu = run(F, ratings, rows, lists, lam, top, pname, weighted=weighted)
                ri, rc, rpp, rpu = xr.tables(ref, lists.shape[1], top)
                assert np.array_equal(items, ri), "contributor ids"
                assert_same_bits(contrib, rc, "contributions")
                assert_same_bits(pp, rpp, "per_pair")
                assert_same_bits(pu, rpu, "per_user")
                real = lists >= 0
                assert stats == {"users": len(ref), "pairs": int(real.sum()), "contributors": int((ri >= 0).sum()), "singular": 0,
                                 "residual_abs_max": np.abs(rpp[:, :, 3][real]).max()}
                if rows is None:
                    assert np.all(pp[:, :, 3][real] == 0.0) and not np.signbit(pp[:, :, 3][real]).any() and np.all(pu[:, USER["dist2"]] == 0.0)


# ------------------------------------------------------------------------------------------------ the general fixture
GEN_ROWS, GEN_LMAX = 3000, pcr.PCR_EXPLAIN_MAX_L
GEN_K = [1, 4, 5, 16, 17, 64, 65, 100, 112]
_general, _general_ref = {}, {}


def general_lengths(k):
    b = pcr.explain_ridge_boundaries(k)
    return sorted({0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 2049} | {max(x + d, 0) for x in b["rows"] for d in (-1, 0, 1)})


def general_case(k):
    """F ~ N(0, 1) / sqrt(k) rounded to f32 (both storage types hold the same values), rows = 3000; one user per row length,
    distinct items in random order, integer ratings 1 .. 5; lists [n, 128] with trailing -1 on every third user and one all -1.
    lam_w = 1e-2 mean|row|^2 (weighted); lam_p[i] = 1e-2 mean|row|^2 max(1, len_i / 50) (plain: a call per distinct value)."""
    if k not in _general:
        rng = np.random.default_rng(900 + k)
        F = xr.rounded(rng.standard_normal((GEN_ROWS, k)) / np.sqrt(k), True)
        lens = np.array(general_lengths(k))
        idx = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        item = np.concatenate([rng.choice(GEN_ROWS, size=n, replace=False) for n in lens]).astype(np.int32)
        val = rng.integers(1, 6, size=len(item)).astype(np.float64)
        U = xr.rounded(rng.standard_normal((len(lens), k)) / np.sqrt(k), True)
        lists = rng.integers(0, GEN_ROWS, size=(len(lens), GEN_LMAX)).astype(np.int32)
        msq = float((F * F).sum(axis=1).mean())
        _general[k] = (F, (idx, item, val), U, lists, 1e-2 * msq, 1e-2 * msq * np.maximum(1.0, lens / 50.0))
    return _general[k]


def general_lists(k, L):
    lists = general_case(k)[3][:, :L].copy()
    for i in range(lists.shape[0]):
        if i % 3 == 1:
            lists[i, L - L // 3:] = -1
    lists[4, :] = -1
    return lists


def general_ref(k, weighted):
    """The reference at the full list length, shared by every L, E and storage type (a column does not depend on the others)."""
    if (k, weighted) not in _general_ref:
        F, ratings, U, lists, lam_w, lam_p = general_case(k)
        _general_ref[k, weighted] = xr.ref_explain_ridge(F, ratings, U, lists, lam_w if weighted else lam_p, weighted=weighted)
    return _general_ref[k, weighted]


@pytest.mark.parametrize("k", [5, 16, 100, 112])
def test_the_general_fixture_is_well_conditioned(k):
    F, ratings, U, lists, lam_w, lam_p = general_case(k)
    worst = 0.0
    for weighted in (True, False):
        for i in range(len(ratings[0]) - 1):
            it, _ = xr.sorted_row(ratings, i)
            if len(it):
                G, _ = xr.user_system(F, it, lam_w if weighted else lam_p[i], weighted, np.arange(k))
                worst = max(worst, np.linalg.cond(G))
    assert worst <= 1e3, worst


def check_user(F, u, lst_full, L, top, items, contrib, pp, pu):
    """One user's device tables against its reference u (columns of the full list; the first Lu of them are this call's)."""
    lst = lst_full[:L]
    Lu = int((lst >= 0).sum())
    lst = lst[:Lu]
    n = len(u["items"])
    assert np.isnan(pp[Lu:]).all() and (items[Lu:] == -1).all() and (contrib[Lu:] == 0.0).all()
    assert pu[USER["ratings"]] == n and pu[USER["free"]] == len(u["P"]) and pu[USER["status"]] == pcr.PCR_RIDGE_OK
    e, tol = u["e"][:, :Lu], xr.entry_tolerance(F, u, lst)
    solved = n > 0 and len(u["P"]) > 0                                          # (else no system is formed: no contributor)
    have = min(top, n) if solved else 0
    assert (items[:Lu, :have] >= 0).all() and (items[:Lu, have:] == -1).all() and (contrib[:Lu, have:] == 0.0).all()
    scale = np.abs(F[lst]) @ np.abs(u["uh"]) * (F.shape[1] + 2) * 2.0 ** -52
    assert np.all(np.abs(pp[:Lu, PAIR["score"]] - u["score"][:Lu]) <= scale)
    total = tol.sum(axis=0)
    assert np.all(np.abs(pp[:Lu, 0] - (pp[:Lu, 1] + pp[:Lu, 2] + pp[:Lu, 3])) <= total), "score = support + opposition + residual"
    assert np.all(np.abs(pp[:Lu, PAIR["support"]] - u["support"][:Lu]) <= total) and np.all(np.abs(pp[:Lu, PAIR["opposition"]] - u["opposition"][:Lu]) <= total)
    assert abs(pu[USER["loss"]] - u["loss"]) <= 1e-9 * (u["loss"] + 1.0)
    if not solved:
        assert same(pp[:Lu, PAIR["residual"]], pp[:Lu, PAIR["score"]]) and np.all(pp[:Lu, 1:3] == 0.0)
        return
    assert abs(np.sqrt(pu[USER["dist2"]]) - np.sqrt(u["dist2"])) <= 1e-9 * (np.linalg.norm(u["ustar"]) + np.linalg.norm(u["uh"]))
    if Lu == 0:
        return
    c, ids = contrib[:Lu, :have], items[:Lu, :have]
    assert np.all(np.diff(c, axis=1) <= 0.0), "contributions are non-increasing"
    pos = np.searchsorted(u["items"], ids)                                  # (distinct items, ascending)
    assert np.array_equal(u["items"][pos], ids)
    col = np.arange(Lu)[:, None]
    assert np.all(np.abs(c - e[pos, col]) <= tol[pos, col]), "a contributor's value"
    listed = np.zeros(e.shape, bool)
    listed[pos, col] = True
    assert listed.sum(axis=0).min() == have, "a rating is listed twice"
    assert not np.any(~listed & (e - c[:, -1][None, :] > 2.0 * tol)), "an unlisted rating beats the last listed one"


@pytest.mark.gpu
@pytest.mark.parametrize("pname", ["F64", "F32"])
@pytest.mark.parametrize("k", GEN_K)
def test_every_edge_against_the_reference(k, pname):
    """Row lengths at every chunk edge of the kernel, list lengths at the tile edges, E = 1 and 16, weighted and plain."""
    F, ratings, U, lists_full, lam_w, lam_p = general_case(k)
    n = len(ratings[0]) - 1
    for weighted in (True, False):
        ref = general_ref(k, weighted)
        groups = [np.arange(n)] if weighted else [np.flatnonzero(lam_p == v) for v in np.unique(lam_p)]
        for L in (1, 16, 17, GEN_LMAX):
            lists = general_lists(k, L)
            for top in (1, 16):
                for g in groups:
                    items, contrib, stats, pp, pu = run(F, sub_csr(ratings, g), U[g], lists[g], lam_w if weighted else lam_p[g[0]], top, pname,
                                                        weighted=weighted)
                    assert stats["users"] == len(g) and stats["singular"] == 0 and stats["pairs"] == int((lists[g] >= 0).sum())
                    for q, i in enumerate(g):
                        check_user(F, ref[i], lists[i], L, top, items[q], contrib[q], pp[q], pu[q])


# ------------------------------------------------------------------------------------------------ properties of the reference
def test_reference_contributions_sum_to_the_minimisers_score():
    F, ratings, U, lists, lam_w, lam_p = general_case(16)
    for weighted in (True, False):
        for i, u in enumerate(general_ref(16, weighted)):
            lst = lists[i][lists[i] >= 0]
            assert np.allclose(u["e"].sum(axis=0), F[lst] @ u["ustar"], rtol=1e-10, atol=1e-12)
            assert np.allclose(u["score"], u["support"] + u["opposition"] + u["residual"], rtol=1e-10, atol=1e-12)


def test_reference_masked_form_is_the_unmasked_form_restricted_to_the_free_set():
    rng = np.random.default_rng(5)
    k, rows = 9, 60
    F = rng.standard_normal((rows, k))
    it = rng.choice(rows, size=25, replace=False); it.sort()
    r = rng.integers(1, 6, size=25).astype(np.float64)
    uh = np.maximum(rng.standard_normal(k), 0.0)
    P = np.flatnonzero(uh > 0)
    assert 0 < len(P) < k
    lst = np.arange(10)
    a = xr.ref_user(F, it, r, uh, lst, 0.3, True, nonneg=True)
    b = xr.ref_user(F[:, P], it, r, uh[P], lst, 0.3, True, nonneg=False)
    assert np.allclose(a["e"], b["e"], rtol=1e-12, atol=1e-14) and np.allclose(a["ustar"][P], b["ustar"]) and np.all(np.delete(a["ustar"], P) == 0.0)
    assert np.allclose(a["residual"], F[lst] @ uh - a["e"].sum(axis=0))


# ------------------------------------------------------------------------------------------------ rows from the library
def library_case():
    rng = np.random.default_rng(77)
    k, rows = 20, 500
    F = xr.rounded(rng.standard_normal((rows, k)) / np.sqrt(k), True)
    lens = np.array([0, 1, 5, 19, 20, 21, 40, 100, 300, 30])
    idx = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    item = np.concatenate([rng.choice(rows, size=n, replace=False) for n in lens]).astype(np.int32)
    val = rng.integers(1, 6, size=len(item)).astype(np.float64)
    lists = rng.integers(0, rows, size=(len(lens), 12)).astype(np.int32)
    lists[2, 9:] = -1
    return F, (idx, item, val), lists, 0.02


@pytest.mark.gpu
@pytest.mark.parametrize("pname", ["F64", "F32"])
def test_rows_of_ridge_fold_in_have_the_residual_of_their_rounding(pname):
    F, ratings, lists, lam = library_case()
    U, _ = pcr.fold_in_ridge(F, ratings, lam, dtype=PREC[pname])
    items, contrib, stats, pp, pu = run(F, ratings, U, lists, lam, 5, pname)
    vj = np.linalg.norm(F[np.maximum(lists, 0)], axis=2)
    real = lists >= 0
    dist = np.sqrt(pu[:, USER["dist2"]])
    assert np.all(np.abs(pp[:, :, 3])[real] <= (vj * dist[:, None])[real] * (1.0 + 1e-12))
    ref = xr.ref_explain_ridge(F, ratings, None, lists, lam)
    un = np.array([np.linalg.norm(u["ustar"]) for u in ref])
    assert np.all(dist <= (1e-9 if pname == "F64" else 2.0 ** -23) * un)
    assert stats["residual_abs_max"] == np.abs(pp[:, :, 3][real]).max()
    # the minimiser itself: no residual at all
    items0, contrib0, stats0, pp0, pu0 = run(F, ratings, None, lists, lam, 5, pname)
    assert np.all(pp0[:, :, 3][real] == 0.0) and not np.signbit(pp0[:, :, 3][real]).any() and np.all(pu0[:, USER["dist2"]] == 0.0)
    assert stats0["residual_abs_max"] == 0.0
    for i, u in enumerate(ref):
        Lu = int(real[i].sum())
        assert np.all(np.abs(pp0[i, :Lu, 0] - u["score"]) <= 1e-10 * (np.abs(F[lists[i, :Lu]]) @ np.abs(u["ustar"]) + 1e-300))


@pytest.mark.gpu
@pytest.mark.parametrize("pname", ["F64", "F32"])
def test_rows_of_nnls_fold_in_against_the_masked_reference(pname):
    """nonneg = True on fold_in_nnls rows; the last user's ratings are all negative on a non-negative F: its row is all zeros,
    |P| = 0, no contributor."""
    F, (idx, item, val), lists, lam = library_case()
    F = np.abs(F)
    val = val.copy(); val[idx[-2]:] *= -1.0
    ratings = (idx, item, val)
    U, st = pcr.fold_in_nnls(F, ratings, lam, dtype=PREC[pname])
    assert np.all(U[-1] == 0.0) and st["zeros"] > F.shape[1]
    items, contrib, stats, pp, pu = run(F, ratings, U, lists, lam, 16, pname, nonneg=True)
    ref = xr.ref_explain_ridge(F, ratings, U, lists, lam, nonneg=True, f32=pname == "F32")
    for i, u in enumerate(ref):
        check_user(F, u, lists[i], lists.shape[1], 16, items[i], contrib[i], pp[i], pu[i])
    assert pu[-1, USER["free"]] == 0 and (items[-1] == -1).all() and same(pp[-1, :, 3], pp[-1, :, 0]) and np.all(pp[-1, :, 1:3] == 0.0)
    assert np.all(pu[:, USER["free"]] == (xr.rounded(U, pname == "F32") > 0).sum(axis=1))


# ------------------------------------------------------------------------------------------------ independence
@pytest.mark.gpu
@pytest.mark.parametrize("pname", ["F64", "F32"])
def test_a_user_does_not_depend_on_the_batch(pname):
    """Alone, inside a batch of 300 users, with the batch reversed, and across two identical calls: the same bits."""
    rng = np.random.default_rng(12)
    k, rows, n, L = 20, 2500, 300, 18
    lens = rng.integers(0, 120, size=n); lens[7], lens[150], lens[290] = 300, 2100, 64
    idx = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    item = np.concatenate([rng.choice(rows, size=m, replace=False) for m in lens]).astype(np.int32)
    val = rng.integers(1, 6, size=len(item)).astype(np.float64)
    F, U = rng.standard_normal((rows, k)) * 0.4, rng.standard_normal((n, k)) * 0.4
    lists = rng.integers(0, rows, size=(n, L)).astype(np.int32)
    lists[::7, 11:] = -1
    ratings = (idx, item, val)
    for kw in (dict(), dict(nonneg=True, weighted=False)):
        whole = run(F, ratings, U, lists, 0.5, 6, pname, **kw)
        again = run(F, ratings, U, lists, 0.5, 6, pname, **kw)
        for q in (0, 1, 3, 4):
            assert same(whole[q], again[q])
        rev = np.arange(n)[::-1]
        back = run(F, sub_csr(ratings, rev), U[rev], lists[rev], 0.5, 6, pname, **kw)
        for q in (0, 1, 3, 4):
            assert same(np.ascontiguousarray(back[q][rev]), whole[q])
        for i in (0, 7, 150, 290, 299):
            one = run(F, sub_csr(ratings, [i]), U[i:i + 1], lists[i:i + 1], 0.5, 6, pname, **kw)
            for q in (0, 1, 3, 4):
                assert same(one[q][0], whole[q][i]), (i, q)


# ------------------------------------------------------------------------------------------------ solver entry
@pytest.mark.gpu
@pytest.mark.parametrize("pname", ["F64", "F32"])
def test_solver_entry(pname):
    """Solver.explain_ridge on a CCDR1 solver after two iterations equals explain_ridge() on get_factors() and the data set's CSR
    bitwise; training that continues gives the factors of a twin that never called it; a shard solver is refused; the profile
    slot is counted."""
    R = synth.generate("small", seed=41, d1=200, d2=500, nnz=200 * 30)
    ds = pcr.Dataset.from_ratings(R)
    k, lam = 12, 0.05
    prm = dict(k=k, precision=PREC[pname], solver_type=pcr.PCR_SOLVER_CCDR1, **{"lambda": lam})
    s, twin = pcr.Solver(ds, pcr.Parameter(**prm)), pcr.Solver(ds, pcr.Parameter(**prm))
    for x in (s, twin):
        x.set_factors(pcr.initial_col(R.d1, k), None)
        x.iterate(2)
    lists, _ = s.recommend(topk=10)
    Us, Vs = s.get_factors()
    s.profile(True)
    for kw in (dict(), dict(weighted=False), dict(nonneg=True)):
        a = s.explain_ridge(lists, top=5, per_pair=True, per_user=True, **kw)
        b = pcr.explain_ridge(Vs, ds, Us, lists, lam, top=5, dtype=PREC[pname], per_pair=True, per_user=True, **kw)
        assert np.array_equal(a[0], b[0]) and a[2] == b[2] and a[2]["pairs"] == lists.shape[0] * 10 and a[2]["singular"] == 0
        for x, y in zip((a[1], a[3], a[4]), (b[1], b[3], b[4])):
            assert same(x, y)
    assert s.profile_launches("explain/ridge") == 3
    s.profile(False)
    users = np.array([5, 199, 0, 5], np.int32)
    c = s.explain_ridge(lists[users], users=users, train=ds, top=5, nonneg=True, per_pair=True)
    assert np.array_equal(c[0], a[0][users]) and same(c[1], a[1][users]) and same(c[3], a[3][users])
    ra, rb = s.iterate(1), twin.iterate(1)
    assert all(np.array_equal(x, y) for x, y in zip(s.get_factors(), twin.get_factors()))
    other = pcr.Dataset.from_csr(R.d1, R.d2, np.zeros(R.d1 + 1, np.int64), np.zeros(0, np.int32), np.zeros(0))
    with pytest.raises(pcr.PcrError, match=f"error {ERR_ARG}: pcr_explain_ridge: the data set is not the one"):
        s.explain_ridge(lists, train=other)
    with pytest.raises(pcr.PcrError, match=f"error {ERR_ARG}: pcr_explain_ridge: user id 200"):
        s.explain_ridge(lists[:1], users=np.array([200], np.int32))
    with pytest.raises(pcr.PcrError, match=f"error {ERR_ARG}: pcr_explain_ridge: E = 17"):
        s.explain_ridge(lists, top=17)
    s.close(); twin.close()
    idx, it, val = ds.csr(0)
    tidx, tit, tval = ds.csr(1)
    hi = R.d1 // 3
    dsl = pcr.Dataset.from_csr(hi, R.d2, idx[:hi + 1], it[:idx[hi]], val[:idx[hi]].copy(), tidx[:hi + 1], tit[:tidx[hi]], tval[:tidx[hi]].copy())
    sh = pcr.Solver(dsl, pcr.Parameter(k=k, precision=PREC[pname], solver_type=2, **{"lambda": lam}), rank=0, nranks=2, shard=(0, R.d1))
    sh.set_local_only(True)
    with pytest.raises(pcr.PcrError, match=f"error {ERR_STATE}: pcr_explain_ridge: needs every user on the rank"):
        sh.explain_ridge(lists[:hi], train=dsl)
    sh.close()


# ------------------------------------------------------------------------------------------------ refusals (CPU)
def has_device():
    try:
        pcr.predict(np.zeros((1, 1)), np.zeros((1, 1)), np.zeros(1, np.int32), np.zeros(1, np.int32))
        return True
    except pcr.PcrError:
        return False


def test_refusals_name_the_entry_and_come_before_the_device():
    F, U = np.ones((6, 3)), np.ones((2, 3))
    rows = (np.array([0, 2, 3], np.int64), np.array([4, 1, 2], np.int32), np.array([3.0, 1.0, 5.0]))
    lists = np.array([[1, 5, -1], [0, -1, -1]], np.int32)

    def refused(text, code=ERR_ARG, F=F, rows=rows, U=U, lists=lists, lam=0.5, **kw):
        with pytest.raises(pcr.PcrError, match=f"error {code}: pcr_explain_ridge_model: .*{text}"):
            pcr.explain_ridge(F, rows, U, lists, lam, **kw)

    refused("precision", dtype=7)
    refused("lambda", lam=0.0)
    refused("lambda", lam=-1.0)
    refused("lambda", lam=np.inf)
    refused("lambda", lam=np.nan)
    refused("outside", rows=(rows[0], np.array([4, 1, 6], np.int32), rows[2]))
    refused("not finite", rows=(rows[0], rows[1], np.array([3.0, np.nan, 5.0])))
    refused(r"index\[0\]", rows=(np.array([1, 2, 3], np.int64), rows[1], rows[2]))
    refused("monotone", rows=(np.array([0, 2, 1, 3], np.int64), rows[1], rows[2]), U=np.ones((3, 3)), lists=np.zeros((3, 3), np.int32))
    refused("L = 129", lists=np.zeros((2, 129), np.int32))
    refused("E = 0", top=0)
    refused("E = 17", top=17)
    refused("list id", lists=np.array([[1, 6, -1], [0, -1, -1]], np.int32))
    refused("list id", lists=np.array([[1, -2, -1], [0, -1, -1]], np.int32))
    refused("after a -1", lists=np.array([[1, -1, 2], [0, -1, -1]], np.int32))
    refused("rank 116", code=ERR_UNSUPPORTED, F=np.ones((6, 116)), U=np.ones((2, 116)))
    refused("rank 113", code=ERR_UNSUPPORTED, F=np.ones((6, 113)), U=None)
    refused("E = 17", F=np.ones((6, 116)), U=np.ones((2, 116)), top=17)       # an argument error wins over the rank
    for bad in (lambda: pcr.explain_ridge(F, rows, U[:1], lists, 0.5), lambda: pcr.explain_ridge(F, rows, U, lists[:1], 0.5),
                lambda: pcr.explain_ridge(F, rows, np.ones((2, 4)), lists, 0.5), lambda: pcr.explain_ridge(F, rows, None, lists, 0.5, nonneg=True),
                lambda: pcr.explain_ridge(np.ones(6), rows, U, lists, 0.5), lambda: pcr.explain_ridge(F, (rows[0], rows[1][:2], rows[2]), U, lists, 0.5)):
        with pytest.raises(ValueError):
            bad()
    # the null pointers and sizes, straight at the ABI
    ei, ec = np.zeros((2, 3, 5), np.int32), np.zeros((2, 3, 5))
    good = [F.ctypes.data, 6, 3, 0.5, 1, 0, pcr.PCR_F64, 0, 2, rows[0].ctypes.data, rows[1].ctypes.data, rows[2].ctypes.data, U.ctypes.data, 3,
            lists.ctypes.data, 5, ei.ctypes.data, ec.ctypes.data, None, None, None]
    L = pcr.lib()
    for at, value, text in ((0, None, "null F"), (1, 0, "rows must be"), (2, 0, "rank k"), (8, -1, "bad argument"), (9, None, "bad argument"),
                            (10, None, "null item / val"), (11, None, "null item / val"), (14, None, "null lists"), (16, None, "null expl_item"),
                            (17, None, "null expl_item / expl_contrib"), (13, 0, "L = 0"), (15, -1, "E = -1")):
        a = list(good); a[at] = value
        assert L.pcr_explain_ridge_model(*a) == ERR_ARG, (at, value)
        msg = L.pcr_last_error().decode()
        assert msg.startswith("pcr_explain_ridge_model: ") and text in msg, (at, value, msg)
    a = list(good); a[12] = None; a[5] = 1                          # U == NULL with nonneg
    assert L.pcr_explain_ridge_model(*a) == ERR_ARG and "nonneg needs the rows U" in L.pcr_last_error().decode()
    assert L.pcr_explain_ridge(None, None, 0, None, 1, 0, 1, None, 1, None, None, None, None, None) == ERR_ARG
    if not has_device():                                            # valid calls reach the device question last
        for rows_U in (U, None):
            with pytest.raises(pcr.PcrError, match=f"error {ERR_DEVICE}:"):
                pcr.explain_ridge(F, rows, rows_U, lists, 0.5)


def test_symbols_header_marks_and_constants():
    h = open(os.path.join(ROOT, "include", "primalcr.h")).read()
    for sym in ("pcr_explain_ridge_model", "pcr_explain_ridge"):
        assert hasattr(pcr.lib(), sym)
        assert re.search(r"\bint " + sym + r"\([^;]*;\s*/\* \[device\] \*/", h), sym
    assert int(re.search(r"#define PCR_EXPLAIN_RIDGE_USER_FIELDS +(\d+)", h).group(1)) == len(pcr.PCR_EXPLAIN_RIDGE_USER_FIELDS)
    fields = re.search(r"typedef struct pcr_explain_ridge_stats \{(.*?)\}", h, re.S).group(1)
    assert re.findall(r"(\w+)[,;]", fields) == [f for f, _ in pcr.ExplainRidgeStats._fields_]
    b = pcr.explain_ridge_boundaries(100)
    kern = open(os.path.join(ROOT, "primalcr_amd", "csrc", "pcr_explain.h")).read()
    tile, chunk = (int(re.search(rf"#define {n} (\d+)", kern).group(1)) for n in ("EXPLAIN_TILE", "EXPLAIN_CHUNK"))
    assert b["rows"] == sorted({0, 16, 32, chunk, 2 * chunk}) and b["lists"] == list(range(tile, pcr.PCR_EXPLAIN_MAX_L + 1, tile))
    assert (112 + 15) // 16 * 16 <= pcr.PCR_RIDGE_DIRECT_MAX < (113 + 15) // 16 * 16


# ------------------------------------------------------------------------------------------------ CLI
def cli(cmd, cwd):
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True)


def test_cli_refuses_the_documented_combinations(tmp_path):
    base = ["--explain-ridge", "why.txt", "-x", "data", "-l", "0.5"]
    tail = ["m.model", "out.txt"]
    no = "--explain-ridge does not go with --eval"
    for extra, text in ((["--eval", "data"], no), (["--diversity"], no), (["--mmr", "0.5"], no), (["--tradeoff", "0.2,0.4"], no),
                        (["--fold-in", "data"], no), (["--fold-in-ridge", "data"], no), (["--fold-in-nnls", "data"], no),
                        (["--fold-in-items", "f"], no), (["--groups", "g", "--max-per-group", "2"], no), (["--candidates", "c"], no),
                        (["--explain", "other.txt"], "--explain-ridge does not go with --explain\n"),
                        (["--steps", "3"], "--explain-ridge takes no -s and no --steps"), (["-s", "2"], "--explain-ridge takes no -s"),
                        (["-K", "129"], "at most 128"), (["--top", "17"], "--top 17")):
        r = cli([RECOMMEND] + base + extra + tail, tmp_path)
        assert r.returncode == 1 and text in r.stderr, (extra, r.stderr)
    for cmd, text in ((["--explain-ridge", "why.txt", "-l", "0.5"], "--explain-ridge needs -x"),
                      (["--explain-ridge", "why.txt", "-x", "data"], "--explain-ridge needs -l"),
                      (["--explain-ridge", "why.txt", "-x", "data", "-l", "0"], "must be > 0"),
                      (["--explain", "why.txt", "--explain-ridge", "other.txt", "-x", "data", "-l", "1"], "--explain-ridge does not go with --explain\n"),
                      (["--nonneg"], "--nonneg goes with --explain-ridge"),
                      (["--explain", "why.txt", "-x", "data", "-l", "1", "--nonneg"], "--nonneg goes with --explain-ridge")):
        r = cli([RECOMMEND] + cmd + tail, tmp_path)
        assert r.returncode == 1 and text in r.stderr, (cmd, r.stderr)
    r = cli([RECOMMEND], tmp_path)
    assert r.returncode == 1 and "--explain-ridge file [--top E] -x data_dir -l lambda [--plain-reg] [--nonneg]" in r.stdout


@pytest.mark.gpu
def test_cli_writes_the_explanations_of_its_lists(tmp_path):
    R = synth.generate("small", seed=5, d1=60, d2=90, nnz=60 * 12)
    d = synth.write_dir(R, str(tmp_path / "data"))
    rng = np.random.default_rng(2)
    k, lam = 6, 0.75
    U, V = rng.standard_normal((R.d1, k)) * 0.5, rng.standard_normal((R.d2, k)) * 0.5
    pcr.model_save(str(tmp_path / "m.model"), U, V)
    ds = pcr.Dataset.load(d)
    lists, _ = pcr.recommend(U, V, 4, exclude=ds.csr(0)[:2])
    for flags, kw in (([], dict()), (["--plain-reg", "--nonneg"], dict(weighted=False, nonneg=True))):
        r = cli([RECOMMEND, "--explain-ridge", "why.txt", "--top", "3", "-K", "4", "-x", d, "-l", str(lam)] + flags + ["m.model", "out.txt"], tmp_path)
        assert r.returncode == 0, r.stderr
        items, contrib, stats, pp = pcr.explain_ridge(V, ds, U, lists, lam, top=3, per_pair=True, **kw)
        lines = open(tmp_path / "why.txt").read().splitlines()
        assert len(lines) == int((lists >= 0).sum())
        u, l = 17, 2
        want = "%d %d %g %g %g %g " % (u + 1, lists[u, l] + 1, *pp[u, l]) + "".join(" %d:%g" % (items[u, l, e] + 1, contrib[u, l, e]) for e in range(3) if items[u, l, e] >= 0)
        assert lines[u * 4 + l] == want
