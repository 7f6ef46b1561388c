"""explain() / Solver.explain() / omp-pmf-recommend --explain (include/primalcr.h, "explaining recommendations"): a
score v_j . u split into one contribution per item of the user's own training row plus a residual, against the plain-numpy
reference of tests/explain_ref.py.

Exact part: dyadic factors (tests/exact_data.py::dyadic_matrix), lambda and weights powers of two.  Every score is a multiple of
1/4, every coefficient of 1/2, every product and sum below 2^50 units (asserted from the reference), so fp32 and fp64 storage give
the reference's values in ANY summation order and the device must match bit for bit (the sign of a zero is not compared: a
coefficient that is exactly 0 gives +-0 by the sign of the dot beside it).
General part: Gaussian factors against bounds evaluated from the data (explain_ref.term_bounds).
"""
import os
import subprocess

import numpy as np
import pytest

import primalcr_amd as pcr
from primalcr_amd import synth
from conftest import BIN_DIR
import explain_ref as er
import foldin_ref as fr
from exact_data import LAMBDA, density, dyadic_matrix

ERR_ARG, ERR_STATE, ERR_DEVICE, ERR_UNSUPPORTED = -1, -6, -4, -7
PREC = {"F64": pcr.PCR_F64, "F32": pcr.PCR_F32}
RECOMMEND = os.path.join(BIN_DIR, "omp-pmf-recommend")
PAIR = {f: i for i, f in enumerate(pcr.PCR_EXPLAIN_PAIR_FIELDS)}
USER = {f: i for i, f in enumerate(pcr.PCR_EXPLAIN_USER_FIELDS)}


def bits(x):
    """The bit patterns of x with -0.0 folded onto +0.0 (NaNs of the padding compare equal: one pattern on both sides)."""
    x = np.asarray(x, np.float64) + 0.0
    return np.where(np.isnan(x), np.int64(-1), x.view(np.int64))


def assert_same_bits(got, want, what):
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.shape[0] == 0, f"{what}: {bad.shape[0]} entries differ, first at {bad[0]}: {np.asarray(got)[tuple(bad[0])]!r} != {np.asarray(want)[tuple(bad[0])]!r}"


def run_explain(V, X, U, lists, lam, top, solver, pname, weights=None):
    return pcr.explain(V, fr.csr_args(X) if not isinstance(X, tuple) else X, U, lists, lam, top=top, solver_type=solver, weights=weights,
                       dtype=PREC[pname], per_pair=True, per_user=True)


def assert_exact(dev, ref, top):
    items, contrib, stats, pp, pu = dev
    assert np.array_equal(items, ref["items"][:, :, :top]), "contributor ids"
    assert_same_bits(contrib, ref["contrib"][:, :, :top], "contributions")
    assert_same_bits(pp, ref["per_pair"], "per_pair")
    assert_same_bits(pu, ref["per_user"], "per_user")
    L = pp.shape[1]
    real = ~np.isnan(ref["per_pair"][:, :L, 0])
    assert stats["users"] == items.shape[0] and stats["pairs"] == int(real.sum()) and stats["contributors"] == int((items >= 0).sum())
    assert stats["residual_abs_max"] == (np.abs(ref["per_pair"][:, :L, 3][real]).max() if real.any() else 0.0)


def assert_dyadic_headroom(ref):
    """Every sum the entry forms stays below 2^50 units of 1/16 (sums of non-negative terms bound their partial sums)."""
    for e, t, g in zip(ref["e"], ref["t"], ref["g"]):
        assert 16 * max(np.abs(e).sum(axis=0).max() if e.size else 0.0, float(g @ g), np.abs(t).sum()) < 2.0 ** 50


def dyadic_lists(rng, X, d2, L):
    """lists [n, L]: random ids; row i keeps L - (i mod 4) of them (trailing -1), every fifth row none; where the row is long
    enough position 0 repeats at 2 and position 1 is an item of the user's own training row."""
    n = X.d1
    lists = rng.integers(0, d2, size=(n, L)).astype(np.int32)
    for i in range(n):
        a, b = int(X.idx[i]), int(X.idx[i + 1])
        if L >= 3:
            lists[i, 2] = lists[i, 0]
        if L >= 2 and b > a:
            lists[i, 1] = X.item[a + (b - a) // 2]
        keep = 0 if i % 5 == 4 else L - (i % 4)
        lists[i, max(keep, 0):] = -1
    return lists


# ------------------------------------------------------------------------------------------------ 1 exact on dyadic inputs
@pytest.mark.gpu
@pytest.mark.parametrize("pname", ["F64", "F32"])
@pytest.mark.parametrize("solver", [2, 1])
def test_dyadic_inputs_are_explained_bit_for_bit(solver, pname):
    """Unsorted rows with repeated items (the same item twice with the same rating: equal contributions, the tie rule decides), few
    distinct factor values at k = 4 (many equal e_p), list ids inside the training row and twice in a list, weights 1/2 .. 4."""
    rng = np.random.default_rng(100 + solver)
    d2, n, L, top = 40, 24, 7, 16
    for k in (4, 12):
        V, U = dyadic_matrix(rng, d2, k, density(k)), dyadic_matrix(rng, n, k, density(k))
        lens = rng.integers(0, 60, size=n); lens[:3] = (0, 1, 2)
        idx = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        item = rng.integers(0, d2, size=int(idx[-1])).astype(np.int32)           # with replacement, not sorted
        val = rng.integers(1, 6, size=int(idx[-1])).astype(np.float64) if solver == 2 else 1.125 + 0.25 * rng.integers(0, 6, size=int(idx[-1]))
        for i in range(3, n):                                                    # the same item twice with the same rating
            a = int(idx[i])
            if lens[i] >= 4:
                item[a + 3], val[a + 3] = item[a], val[a]
        X = fr.CSR(n, d2, idx, item, val)
        lists = dyadic_lists(rng, X, d2, L)
        w = 2.0 ** rng.integers(-1, 3, size=n)
        ref = er.ref_explain(V, (idx, item, val), U, lists, LAMBDA, top, solver, weights=w, keep=True)
        assert_dyadic_headroom(ref)
        ties = sum(int((np.diff(np.sort(e, axis=0), axis=0) == 0).sum()) for e in ref["e"] if e.size)
        assert ties > 100                                                        # the tie rule is exercised
        assert_exact(run_explain(V, (idx, item, val), U, lists, LAMBDA, top, solver, pname, weights=w), ref, top)


# ------------------------------------------------------------------------------------------------ 2 every boundary
def boundary_lengths():
    b = pcr.explain_boundaries()
    return sorted({0, 1, 2} | {x + d for x in b["rows"] for d in (-1, 0, 1)}), b["lists"]


@pytest.mark.gpu
@pytest.mark.parametrize("pname", ["F64", "F32"])
@pytest.mark.parametrize("solver", [2, 1])
@pytest.mark.parametrize("k", [1, 4, 5, 100])
def test_every_form_chunk_tile_and_rank_edge_is_exact(k, solver, pname):
    """One user per row length at the form and chunk edges (from explain_boundaries()), list lengths at the tile edges, E = 1, 16
    (beyond the length of the short rows), trailing -1 and all -1 lists, d2 = 3000; one reference per case, shared by the calls."""
    lengths, tiles = boundary_lengths()
    assert lengths == [0, 1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049] and tiles[0] == 16 and tiles[-1] == pcr.PCR_EXPLAIN_MAX_L
    d2, Lmax = 3000, pcr.PCR_EXPLAIN_MAX_L
    rng = np.random.default_rng(7 * k + solver)
    V, U = dyadic_matrix(rng, d2, k, density(k)), dyadic_matrix(rng, len(lengths), k, density(k))
    X = fr.make_users(d2, lengths, solver, seed=50 + k)
    full = rng.integers(0, d2, size=(len(lengths), Lmax)).astype(np.int32)
    for L in (1, tiles[0], tiles[0] + 1, Lmax):
        lists = full[:, :L].copy()
        for i in range(len(lengths)):                                            # trailing padding; one all -1 row
            if i % 3 == 1:
                lists[i, L - L // 3:] = -1
        lists[4, :] = -1
        ref = er.ref_explain(V, fr.csr_args(X), U, lists, LAMBDA, 16, solver, keep=True)
        assert_dyadic_headroom(ref)
        for top in (1, 16):
            assert_exact(run_explain(V, X, U, lists, LAMBDA, top, solver, pname), ref, top)


# ------------------------------------------------------------------------------------------------ 3 general data
GEN_K, GEN_LAM, GEN_L, GEN_TOP, GEN_D2 = 100, 2.0, 10, 5, 2000
_general = {}


def general_case(solver):
    """Seeded Gaussian factors, k = 100, integer ratings 1 .. 5 (solver 1: quarter steps), 36 rows of 5 .. 600 ratings."""
    if solver not in _general:
        rng = np.random.default_rng(2024 + solver)
        lengths = [5, 6, 63, 64, 65, 255, 256, 257, 600] + list(rng.integers(5, 601, size=27))
        X = fr.make_users(GEN_D2, lengths, solver, seed=77)
        V = rng.standard_normal((GEN_D2, GEN_K)) / np.sqrt(GEN_K) * 2.0
        U = rng.standard_normal((len(lengths), GEN_K)) / np.sqrt(GEN_K) * 2.0
        lists = rng.integers(0, GEN_D2, size=(len(lengths), GEN_L)).astype(np.int32)
        lists[3, 7:] = -1
        _general[solver] = (X, V, U, lists)
    return _general[solver]


def slot_bounds(b, e, l, top):
    """Column l of a user: (order, srt, bound) -- the reference's ratings by descending contribution (stable), their values, and
    per slot the bound b[p, l] of the rating p the reference puts there; one slot more than top where the row has it, for the gap
    below the last reported slot."""
    order = np.argsort(-e[:, l], kind="stable")[:top + 1]
    return order, e[order, l], b[order, l]


def ids_comparable(srt, bound, r):
    """Slot r's id is compared when the reference's gaps to both neighbouring contributions exceed twice the per-term bound --
    the larger of the slot's own and that neighbour's, so that two terms inside their bounds cannot have changed places."""
    ok = True
    if r > 0:
        ok = ok and srt[r - 1] - srt[r] > 2.0 * max(bound[r - 1], bound[r])
    if r + 1 < len(srt):
        ok = ok and srt[r] - srt[r + 1] > 2.0 * max(bound[r], bound[r + 1])
    return ok


def check_general(solver, pname):
    """Device against reference, bounds from explain_ref.term_bounds.  Slot r's value is held to the bound of the rating the
    reference puts there: in fp64 the documented per-term bound b0 = (k + 2) 2^-52 sum_t |v_pt v_jt| |c_p| / lambda_u alone; in
    fp32 b0 + bc, bc = dc |v_p . v_j| / lambda_u with |dc_p| <= 2 n dm and dm <= (k + 2) 2^-24 sum_t |u_t v_t| -- the f32 error of m,
    propagated linearly.  Ids wherever ids_comparable() says so.  The identity is checked on the device's own numbers within the
    documented bound alone.  Returns (slots, slots left out of the id comparison)."""
    X, V, U, lists = general_case(solver)
    f32 = pname == "F32"
    ref = er.ref_explain(V, fr.csr_args(X), U, lists, GEN_LAM, GEN_TOP, solver, f32=f32, keep=True)
    items, contrib, stats, pp, pu = run_explain(V, X, U, lists, GEN_LAM, GEN_TOP, solver, pname)
    Vr, Ur = er.rounded(V, f32), er.rounded(U, f32)
    slots = skipped = 0
    worst = {"identity": 0.0, "value": 0.0, "pair": 0.0}
    for i in range(X.d1):
        b0, bc, extra = er.term_bounds(Vr, Ur, lists, ref, i, GEN_K, 2.0 ** -24)
        b = b0 + bc if f32 else b0
        e = ref["e"][i]
        Lu = e.shape[1]
        assert np.isnan(pp[i, Lu:]).all() and (items[i, Lu:] == -1).all() and (contrib[i, Lu:] == 0.0).all()
        ident = np.abs(pp[i, :Lu, 0] - (pp[i, :Lu, 1] + pp[i, :Lu, 2] + pp[i, :Lu, 3]))
        lim = b0.sum(axis=0) + extra
        worst["identity"] = max(worst["identity"], float((ident / lim).max()))
        assert (ident <= lim).all(), f"user {i}: identity off by {ident} against {lim}"
        psum = b.sum(axis=0)                                                    # a sum of terms is off by no more than theirs
        for f in ("support", "opposition"):
            d = np.abs(pp[i, :Lu, PAIR[f]] - ref["per_pair"][i, :Lu, PAIR[f]])
            worst["pair"] = max(worst["pair"], float((d / psum).max()))
            assert (d <= psum).all(), f"user {i}: {f} off by {d} against {psum}"
        assert (np.abs(pp[i, :Lu, 0] - ref["per_pair"][i, :Lu, 0]) <= extra).all()
        for l in range(Lu):
            order, srt, bound = slot_bounds(b, e, l, GEN_TOP)
            m = min(GEN_TOP, e.shape[0])
            dv = np.abs(contrib[i, l, :m] - srt[:m])
            worst["value"] = max(worst["value"], float((dv / np.maximum(bound[:m], 1e-300)).max()))
            assert (dv <= bound[:m]).all(), f"user {i} list {l}: contribution values off by {dv} against {bound[:m]}"
            for r in range(m):
                slots += 1
                if ids_comparable(srt, bound, r):
                    assert items[i, l, r] == ref["items"][i, l, r], f"user {i} list {l} slot {r}"
                else:
                    skipped += 1
    print(f"explain general solver {solver} {pname}: slots {slots} left out {skipped} worst ratios to the bounds {worst}")
    return slots, skipped


@pytest.mark.gpu
@pytest.mark.parametrize("solver", [2, 1])
def test_general_data_fp64_meets_the_documented_bounds(solver):
    slots, skipped = check_general(solver, "F64")
    assert skipped == 0 and slots > 1500           # the seed's own gaps are far above a 1e-12-scale bound (checked on the CPU below)


@pytest.mark.gpu
@pytest.mark.parametrize("solver", [2, 1])
def test_general_data_fp32_meets_the_bound_of_its_scores(solver):
    """The reference runs on the f32-rounded factors; m is formed in f32 on the device."""
    slots, skipped = check_general(solver, "F32")
    assert skipped <= slots // 100


@pytest.mark.parametrize("solver", [2, 1])
def test_the_seed_leaves_no_slot_out_of_the_id_comparison(solver):
    """CPU: with the documented per-term bound of fp64, every reported slot of the general case is id-comparable -- the GPU test
    compares every id; with the fp32 bounds at most 1 % of the slots are left out."""
    X, V, U, lists = general_case(solver)
    for f32 in (False, True):
        ref = er.ref_explain(V, fr.csr_args(X), U, lists, GEN_LAM, GEN_TOP, solver, f32=f32, keep=True)
        Vr, Ur = er.rounded(V, f32), er.rounded(U, f32)
        slots = skipped = 0
        for i in range(X.d1):
            b0, bc, _ = er.term_bounds(Vr, Ur, lists, ref, i, GEN_K, 2.0 ** -24)
            e = ref["e"][i]
            for l in range(e.shape[1]):
                order, srt, bound = slot_bounds(b0 + bc if f32 else b0, e, l, GEN_TOP)
                for r in range(min(GEN_TOP, e.shape[0])):
                    slots += 1
                    skipped += 0 if ids_comparable(srt, bound, r) else 1
        assert slots > 1500 and (skipped <= slots // 100 if f32 else skipped == 0), (f32, slots, skipped)


def test_the_reference_satisfies_the_identity():
    """Self-check of explain_ref on random data: score = support + opposition + residual to 1e-10 relative."""
    for solver in (2, 1):
        X, V, U, lists = general_case(solver)
        w = np.random.default_rng(1).uniform(0.5, 2.0, size=X.d1)
        ref = er.ref_explain(V, fr.csr_args(X), U, lists, GEN_LAM, GEN_TOP, solver, weights=w, keep=True)
        pp = ref["per_pair"]
        real = ~np.isnan(pp[:, :, 0])
        scale = np.abs(pp[:, :, 1]) + np.abs(pp[:, :, 2]) + np.abs(pp[:, :, 3]) + np.abs(pp[:, :, 0])
        err = np.abs(pp[:, :, 0] - (pp[:, :, 1] + pp[:, :, 2] + pp[:, :, 3]))
        assert real.sum() > 300 and (err[real] <= 1e-10 * scale[real]).all()
        assert np.isnan(pp[~real]).all()


# ------------------------------------------------------------------------------------------------ 4 cross-checks
@pytest.mark.gpu
@pytest.mark.parametrize("pname", ["F64", "F32"])
@pytest.mark.parametrize("solver", [2, 1])
def test_a_converged_fold_in_has_small_residuals_and_the_same_gradient_norm(solver, pname):
    """After fold_in() has converged a user (gn2 < 1e-4), |residual| = |v_j . g| / lambda <= |v_j| 0.01 / lambda, and gnorm2
    agrees with fold-in's: both have the same m bits; fold-in rounds c to the storage type and adds its lane groups' shares in
    it, so g_t moves by at most (n + 2) eps sum_p |c_p v_pt| and |g|^2 by 2 |g| |dg| + |dg|^2."""
    rng = np.random.default_rng(5 + solver)
    k, d2, lam = 16, 300, 4.0
    X = fr.make_users(d2, [0, 1, 3, 8, 20, 40, 64, 65, 90, 130], solver, seed=9)
    V = rng.standard_normal((d2, k)) * 0.5
    Un, st, per = pcr.fold_in(V, fr.csr_args(X), lam, solver_type=solver, steps=60, dtype=PREC[pname], per_user=True)
    conv = np.flatnonzero(per[:, pcr.PCR_FOLDIN_FIELDS.index("status")] == pcr.PCR_FOLDIN_CONVERGED)
    assert len(conv) >= 5
    lists = rng.integers(0, d2, size=(X.d1, 8)).astype(np.int32)
    items, contrib, stats, pp, pu = run_explain(V, X, Un, lists, lam, 5, solver, pname)
    f32 = pname == "F32"
    Vr = er.rounded(V, f32)
    ref = er.ref_explain(V, fr.csr_args(X), Un, lists, lam, 5, solver, f32=f32, keep=True)
    eps = 2.0 ** -24 if f32 else 2.0 ** -53
    for i in conv:
        assert (np.abs(pp[i, :, PAIR["residual"]]) <= np.linalg.norm(Vr[lists[i]], axis=1) * 0.01 / lam).all()
        it, t = ref["rows"][i], ref["t"][i]
        dg = np.linalg.norm((len(it) + 2) * eps * (np.abs(t) @ np.abs(Vr[it]))) if len(it) else 0.0
        gn_fold, gn = per[i, pcr.PCR_FOLDIN_FIELDS.index("gnorm2")], pu[i, USER["gnorm2"]]
        if len(it) == 0:
            continue                                   # (fold-in reports 0 for a user without ratings; here g = lambda u, and u = 0)
        assert abs(gn - gn_fold) <= 2.0 * np.sqrt(max(gn, gn_fold)) * dg + dg * dg, (i, gn, gn_fold, dg)
    assert pu[0, USER["gnorm2"]] == 0.0 and pu[0, USER["ratings"]] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("pname", ["F64", "F32"])
@pytest.mark.parametrize("solver", [2, 1])
def test_a_weight_is_the_regulariser_divided(solver, pname):
    X, V, U, lists = general_case(solver)
    a = run_explain(V, X, U, lists, GEN_LAM, 4, solver, pname, weights=np.full(X.d1, 4.0))
    b = run_explain(V, X, U, lists, GEN_LAM / 4.0, 4, solver, pname)
    assert np.array_equal(a[0], b[0]) and a[2] == b[2]
    for x, y in zip((a[1], a[3], a[4]), (b[1], b[3], b[4])):
        assert np.array_equal(x.view(np.int64), y.view(np.int64))


# ------------------------------------------------------------------------------------------------ 5 independence
@pytest.mark.gpu
@pytest.mark.parametrize("pname", ["F64", "F32"])
@pytest.mark.parametrize("solver", [2, 1])
def test_a_user_does_not_depend_on_the_batch(solver, pname):
    """Alone, inside a batch of 300 users, with the batch reversed, and across two identical calls: the same bits."""
    rng = np.random.default_rng(12)
    k, d2, n, L = 20, 2500, 300, 18
    lengths = list(rng.integers(0, 120, size=n)); lengths[7], lengths[150], lengths[290] = 300, 2100, 64
    X = fr.make_users(d2, lengths, solver, seed=3)
    V, U = rng.standard_normal((d2, k)) * 0.4, rng.standard_normal((n, k)) * 0.4
    lists = rng.integers(0, d2, size=(n, L)).astype(np.int32)
    lists[::7, 11:] = -1
    idx, item, val = fr.csr_args(X)
    whole = run_explain(V, X, U, lists, 1.5, 6, solver, pname)
    again = run_explain(V, X, U, lists, 1.5, 6, solver, pname)
    same = lambda x, y: np.array_equal(x.view(np.int64) if x.dtype == np.float64 else x, y.view(np.int64) if y.dtype == np.float64 else y)
    for q in (0, 1, 3, 4):
        assert same(whole[q], again[q])
    rev = np.arange(n)[::-1]
    ridx = np.concatenate([[0], np.cumsum(np.diff(idx)[rev])]).astype(np.int64)
    ritem = np.concatenate([item[idx[i]:idx[i + 1]] for i in rev]); rval = np.concatenate([val[idx[i]:idx[i + 1]] for i in rev])
    back = run_explain(V, (ridx, ritem, rval), U[rev], lists[rev], 1.5, 6, solver, pname)
    for q in (0, 1, 3, 4):
        assert same(np.ascontiguousarray(back[q][rev]), whole[q])
    for i in (0, 7, 150, 290, 299):
        one = run_explain(V, (np.array([0, idx[i + 1] - idx[i]], np.int64), item[idx[i]:idx[i + 1]], val[idx[i]:idx[i + 1]]), U[i:i + 1],
                          lists[i:i + 1], 1.5, 6, solver, pname)
        for q in (0, 1, 3, 4):
            assert same(one[q][0], whole[q][i]), (i, q)


# ------------------------------------------------------------------------------------------------ 6 solver entry
@pytest.mark.gpu
@pytest.mark.parametrize("pname", ["F64", "F32"])
def test_solver_entry(pname):
    """Solver.explain on Solver.recommend's lists equals explain() on get_factors() and the data set's CSR bitwise; training that
    continues gives the factors of a twin that never called it; a CCDR1 solver and a mismatching train are refused."""
    R = synth.generate("small", seed=41, d1=200, d2=500, nnz=200 * 30)
    ds = pcr.Dataset.from_ratings(R)
    k, lam = 12, 20.0
    par = lambda **kw: pcr.Parameter(k=k, precision=PREC[pname], **{"lambda": lam}, **kw)
    s, twin = pcr.Solver(ds, par(solver_type=2)), pcr.Solver(ds, par(solver_type=2))
    U0, V0 = pcr.initial(R.d1, k), pcr.initial(R.d2, k)
    for x in (s, twin):
        x.set_factors(U0, V0)
        x.iterate(3)
    lists, _ = s.recommend(topk=10)
    Us, Vs = s.get_factors()
    a = s.explain(lists, top=5, per_pair=True, per_user=True)
    b = pcr.explain(Vs, ds, Us, lists, lam, top=5, solver_type=2, dtype=PREC[pname], per_pair=True, per_user=True)
    assert np.array_equal(a[0], b[0]) and a[2] == b[2] and a[2]["pairs"] == lists.shape[0] * 10
    for x, y in zip((a[1], a[3], a[4]), (b[1], b[3], b[4])):
        assert np.array_equal(x.view(np.int64), y.view(np.int64))
    users = np.array([5, 199, 0, 5], np.int32)
    c = s.explain(lists[users], users=users, train=ds, top=5, per_pair=True)
    assert np.array_equal(c[0], a[0][users]) and np.array_equal(c[1].view(np.int64), a[1][users].view(np.int64))
    w = np.full(R.d1, 2.0)
    d = s.explain(lists, weights=w, top=5)
    e = pcr.explain(Vs, ds, Us, lists, lam, top=5, weights=w, dtype=PREC[pname])
    assert np.array_equal(d[0], e[0]) and np.array_equal(d[1].view(np.int64), e[1].view(np.int64))
    s.iterate(1); twin.iterate(1)
    for x, y in zip(s.get_factors(), twin.get_factors()):
        assert np.array_equal(x, y)
    other = pcr.Dataset.from_csr(R.d1, R.d2, np.zeros(R.d1 + 1, np.int64), np.zeros(0, np.int32), np.zeros(0))
    with pytest.raises(pcr.PcrError, match=f"error {ERR_ARG}: pcr_explain: the data set is not the one"):
        s.explain(lists, train=other)
    with pytest.raises(pcr.PcrError, match=f"error {ERR_ARG}: pcr_explain: user id 200"):
        s.explain(lists[:1], users=np.array([200], np.int32))
    s.close(); twin.close()
    c0 = pcr.Solver(ds, pcr.Parameter(k=k, solver_type=pcr.PCR_SOLVER_CCDR1, **{"lambda": lam}))
    with pytest.raises(pcr.PcrError, match=f"error {ERR_STATE}: pcr_explain"):
        c0.explain(lists)
    c0.close()
    idx, it, val = ds.csr(0)
    tidx, tit, tval = ds.csr(1)
    hi = R.d1 // 3
    dsl = pcr.Dataset.from_csr(hi, R.d2, idx[:hi + 1], it[:idx[hi]], val[:idx[hi]].copy(), tidx[:hi + 1], tit[:tidx[hi]], tval[:tidx[hi]].copy())
    sh = pcr.Solver(dsl, par(solver_type=2), rank=0, nranks=2, shard=(0, R.d1))
    sh.set_local_only(True)
    with pytest.raises(pcr.PcrError, match=f"error {ERR_STATE}: pcr_explain: needs every user on the rank"):
        sh.explain(lists[:hi], train=dsl)
    sh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pname", ["F64", "F32"])
def test_a_rank_beyond_the_lds_is_refused_by_the_form_and_the_next_call_runs(pname):
    """The smallest rank whose one-wave form (64 ratings, a level per rating) exceeds a CU's 160 KiB, derived from the KERNEL: every
    array k_explain carves out of LDS (its `take<type>(count)` lines in pcr_explain.h) evaluated at the form's largest user -- not
    from the host's byte formulas, which decide the refusal; the rank below it runs."""
    import re
    from conftest import ROOT
    elt = 8 if pname == "F64" else 4
    takes = re.findall(r"= (?:small|big)\.take<(\w+)>\((.*?)\);", open(os.path.join(ROOT, "primalcr_amd", "csrc", "pcr_explain.h")).read())
    assert len(takes) == 20
    size = {"T": elt, "double": 8, "int32_t": 4, "uint16_t": 2, "LI": 4, "int": 4}          # (LI: 32 bits in the LDS forms)

    def nbytes(k):
        env = dict(ld=(k + 3) & ~3, BLOCK=64, PCR_WAVE=64, VEC=16 // elt, EXPLAIN_TILE=16, cap=pcr.PCR_FOLDIN_WAVE_MAX,
                   rs_cap=pcr.PCR_FOLDIN_WAVE_MAX + 1, erows=min(pcr.PCR_FOLDIN_WAVE_MAX, pcr.EXPLAIN_CHUNK))
        return sum((eval(expr.replace("(size_t)", "").replace("geo.ld", "ld").replace("/", "//"), {}, env) * size[ty] + 15) & ~15
                   for ty, expr in takes)

    k = 1
    while nbytes(k) <= 160 * 1024:
        k += 1
    one = (np.array([0, 1], np.int64), np.array([2], np.int32), np.array([3.0]))
    rng = np.random.default_rng(0)
    call = lambda r: pcr.explain(rng.standard_normal((4, r)) / np.sqrt(r), one, rng.standard_normal((1, r)), np.array([[1, 3]], np.int32), 0.5,
                                 dtype=PREC[pname])
    with pytest.raises(pcr.PcrError) as e:
        call(k)
    assert str(e.value) == (f"libprimalcr error {ERR_UNSUPPORTED}: explain: rank {k} is too large for the LDS of the workgroup form of users "
                            f"of up to {pcr.PCR_FOLDIN_WAVE_MAX} ratings")
    items, contrib, stats = call(k - 1)
    assert items[0, 0, 0] == 2 and np.isfinite(contrib).all() and stats["pairs"] == 2


# ------------------------------------------------------------------------------------------------ refusals (CPU)
def has_device():
    try:
        pcr.predict(np.zeros((1, 1)), np.zeros((1, 1)), np.zeros(1, np.int32), np.zeros(1, np.int32))
        return True
    except pcr.PcrError:
        return False


def test_refusals_name_the_entry_and_come_before_the_device():
    V, U = np.ones((6, 3)), np.ones((2, 3))
    rows = (np.array([0, 2, 3], np.int64), np.array([4, 1, 2], np.int32), np.array([3.0, 1.0, 5.0]))
    lists = np.array([[1, 5, -1], [0, -1, -1]], np.int32)

    def refused(text, code=ERR_ARG, V=V, rows=rows, U=U, lists=lists, lam=0.5, **kw):
        with pytest.raises(pcr.PcrError, match=f"error {code}: pcr_explain_model: .*{text}"):
            pcr.explain(V, rows, U, lists, lam, **kw)

    refused("precision", dtype=7)
    refused("lambda", lam=0.0)
    refused("lambda", lam=-1.0)
    refused("lambda", lam=np.inf)
    refused("solver type", solver_type=3)
    refused("CCDR1", code=ERR_UNSUPPORTED, solver_type=pcr.PCR_SOLVER_CCDR1)
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
    refused("weight of user 1", weights=np.array([1.0, 0.0]))
    refused("weight of user 0", weights=np.array([np.inf, 1.0]))
    refused("weight of user 1", weights=np.array([1.0, np.nan]))
    many = np.arange(70000, dtype=np.float64)                       # more levels than the level builder's 16 bits (PrimalCR: raw doubles)
    refused("65535", code=ERR_UNSUPPORTED, V=np.zeros((70000, 3)), U=U[:1], lists=lists[:1], solver_type=1,
            rows=(np.array([0, 70000], np.int64), np.arange(70000, dtype=np.int32), many))
    with pytest.raises(ValueError):
        pcr.explain(V, rows, U[:1], lists, 0.5)
    with pytest.raises(ValueError):
        pcr.explain(V, rows, U, lists[:1], 0.5)
    # the null pointers, straight at the ABI
    p = pcr.Parameter(k=3, **{"lambda": 0.5})
    ei, ec = np.zeros((2, 3, 5), np.int32), np.zeros((2, 3, 5))
    good = [V.ctypes.data, 6, 2, rows[0].ctypes.data, rows[1].ctypes.data, rows[2].ctypes.data, U.ctypes.data, None, 3, lists.ctypes.data, 5,
            ei.ctypes.data, ec.ctypes.data, None, None, None]
    import ctypes as C
    for at, value, text in ((0, None, "null V"), (6, None, "null U"), (9, None, "null lists"), (11, None, "null expl_item"),
                            (12, None, "null expl_item / expl_contrib"), (3, None, "bad argument"), (2, -1, "bad argument"), (1, 0, "bad argument"),
                            (4, None, "null item / val"), (5, None, "null item / val"), (8, 0, "L = 0"), (10, -1, "E = -1")):
        a = list(good); a[at] = value
        assert pcr.lib().pcr_explain_model(C.byref(p), *a) == ERR_ARG, (at, value)
        msg = pcr.lib().pcr_last_error().decode()
        assert msg.startswith("pcr_explain_model: ") and text in msg, (at, value, msg)
    for bad_p, text in ((pcr.Parameter(k=0, **{"lambda": 0.5}), "rank k"), (pcr.Parameter(k=3, **{"lambda": float("nan")}), "lambda")):
        assert pcr.lib().pcr_explain_model(C.byref(bad_p), *good) == ERR_ARG
        msg = pcr.lib().pcr_last_error().decode()
        assert msg.startswith("pcr_explain_model: ") and text in msg, msg
    assert pcr.lib().pcr_explain_model(None, *good) == ERR_ARG and "null parameters" in pcr.lib().pcr_last_error().decode()
    assert pcr.lib().pcr_explain(None, None, 0, None, None, 1, None, 1, None, None, None, None, None) == ERR_ARG
    if not has_device():                                            # a valid call reaches the device question last
        with pytest.raises(pcr.PcrError, match=f"error {ERR_DEVICE}:"):
            pcr.explain(V, rows, U, lists, 0.5)


def test_boundaries_and_constants_mirror_the_header():
    import re
    from conftest import ROOT
    h = open(os.path.join(ROOT, "include", "primalcr.h")).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (PCR_EXPLAIN_\w+|PCR_FOLDIN_\w+_MAX) +(\d+)", h)}
    assert defs["PCR_EXPLAIN_MAX_L"] == pcr.PCR_EXPLAIN_MAX_L and defs["PCR_EXPLAIN_MAX_E"] == pcr.PCR_EXPLAIN_MAX_E
    assert defs["PCR_EXPLAIN_PAIR_FIELDS"] == len(pcr.PCR_EXPLAIN_PAIR_FIELDS) and defs["PCR_EXPLAIN_USER_FIELDS"] == len(pcr.PCR_EXPLAIN_USER_FIELDS)
    k = open(os.path.join(ROOT, "primalcr_amd", "csrc", "pcr_explain.h")).read()
    tile, chunk = (int(re.search(rf"#define {n} (\d+)", k).group(1)) for n in ("EXPLAIN_TILE", "EXPLAIN_CHUNK"))
    b = pcr.explain_boundaries()
    assert b["rows"] == sorted({defs["PCR_FOLDIN_WAVE_MAX"], chunk, defs["PCR_FOLDIN_LDS_MAX"]}) and b["lists"] == list(range(tile, 129, tile))


# ------------------------------------------------------------------------------------------------ CLI
def run(cmd, cwd):
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True)


def test_cli_refuses_the_documented_combinations(tmp_path):
    base = ["--explain", "why.txt", "-x", "data", "-l", "0.5"]
    tail = ["m.model", "out.txt"]
    for extra, text in ((["--eval", "data"], "--explain does not go with"), (["--diversity"], "--explain does not go with"),
                        (["--mmr", "0.5"], "--explain does not go with"), (["--tradeoff", "0.2,0.4"], "--explain does not go with"),
                        (["--eval", "data", "--ranks"], "--explain does not go with"), (["--fold-in", "data"], "--explain does not go with"),
                        (["--fold-in-ridge", "data"], "--explain does not go with"), (["--fold-in-nnls", "data"], "--explain does not go with"),
                        (["--fold-in-items", "f"], "--explain does not go with"),
                        (["--groups", "g", "--max-per-group", "2"], "--explain does not go with"), (["--candidates", "c"], "--explain does not go with"),
                        (["--steps", "3"], "--explain takes no --steps"), (["-K", "129"], "at most 128"), (["--top", "17"], "--top 17"),
                        (["--top", "0"], "--top 0")):
        r = run([RECOMMEND] + base + extra + tail, tmp_path)
        assert r.returncode == 1 and text in r.stderr, (extra, r.stderr)
    for cmd, text in ((["--explain", "why.txt", "-l", "0.5"], "--explain needs -x"), (["--explain", "why.txt", "-x", "data"], "--explain needs -l"),
                      (["--explain", "why.txt", "-x", "data", "-l", "0"], "must be > 0"), (["--top", "3"], "--top goes with --explain"),
                      (["-l", "0.5"], "-l, -s and --steps go with --fold-in")):
        r = run([RECOMMEND] + cmd + tail, tmp_path)
        assert r.returncode == 1 and text in r.stderr, (cmd, r.stderr)
    r = run([RECOMMEND], tmp_path)
    assert r.returncode == 1 and "--explain file" in r.stdout and "--top E" in r.stdout


@pytest.mark.gpu
def test_cli_writes_the_explanations_of_its_lists(tmp_path):
    R = synth.generate("small", seed=5, d1=60, d2=90, nnz=60 * 12)
    d = synth.write_dir(R, str(tmp_path / "data"))
    rng = np.random.default_rng(2)
    k, lam = 6, 0.75
    U, V = rng.standard_normal((R.d1, k)) * 0.5, rng.standard_normal((R.d2, k)) * 0.5
    pcr.model_save(str(tmp_path / "m.model"), U, V)
    r = run([RECOMMEND, "--explain", "why.txt", "--top", "3", "-K", "4", "-x", d, "-l", str(lam), "m.model", "out.txt"], tmp_path)
    assert r.returncode == 0, r.stderr
    ds = pcr.Dataset.load(d)
    lists, _ = pcr.recommend(U, V, 4, exclude=ds.csr(0)[:2])
    got = [ln.split() for ln in open(tmp_path / "out.txt").read().splitlines()]
    assert [int(x) - 1 for x in got[17][1:]] == list(lists[17])
    items, contrib, stats, pp = pcr.explain(V, ds, U, lists, lam, top=3, per_pair=True)
    lines = open(tmp_path / "why.txt").read().splitlines()
    assert len(lines) == int((lists >= 0).sum())
    u, l = 17, 2
    want = "%d %d %g %g %g %g " % (u + 1, lists[u, l] + 1, *pp[u, l]) + "".join(" %d:%g" % (items[u, l, e] + 1, contrib[u, l, e]) for e in range(3) if items[u, l, e] >= 0)
    assert lines[u * 4 + l] == want
