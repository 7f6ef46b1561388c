"""Per-rating confidence weights in CCDR1 training (pcr_solver_set_rating_weights) against the weighted numpy reference
of tests/ccd_weight_ref.py, on the data sets and parameter rows of tests/test_ccd_reference.py.

CPU part: with all-ones weights the weighted reference IS tests/ccd_ref.py, bit for bit (which ties it to the goldens of the
reference binary); weights that are all the same power of two leave the factors where they are and scale loss, obj and reg
exactly; the bounds of the GPU part are computed from the reference alone, the way tests/test_ccd_reference.py computes them (fp64:
16 x the spread over summation orders and a long-double run; fp32: bit-identical across orders, 4 x the spread of a one-ulp nudge
of one stored u;
scalars with the 64 x 2^-53 floor) -- no tolerance is a literal; seeded defects (one weight read as 1, the count in the place of W)
land at least 100 x outside them; the host helpers, the CLI's refusals and the exports.
GPU part (-m gpu): the Python binding and omp-pmf-train against that reference and against the unweighted solver.
"""
import functools
import math
import os
import re
import subprocess

import numpy as np
import pytest

from ccd_data import ratings
from ccd_ref import ccd_ref
from ccd_weight_ref import ccd_weight_ref
from conftest import BIN_DIR, ROOT
from primalcr_amd import synth
from test_ccd_reference import (BIG, LAM, MAXITER, ROWS, SUM_FLOOR, assert_lines, bits, counts, data, dataset, dist, initial, parse_lines,
                                scalar_dist, solver)

TRAIN = os.path.join(BIN_DIR, "omp-pmf-train")
W_ROWS = ("default", "nmf", "eps05", "T0", "T1", "k1")
DRAWS = np.array([0.25, 0.5, 1.0, 2.0, 4.0])
DEFECT_LENGTHS = (1, 65, 4096, 4097, 8200)


# ------------------------------------------------------------------------------------------------------------ helpers
@functools.lru_cache(maxsize=None)
def parity_weights(name):
    """The non-trivial weights of the parity tests, in the order of the set's ratings (user-major, items ascending: the training
    CSR's order): (n_max / n_item)^0.5 times a seeded draw from {1/4, 1/2, 1, 2, 4}."""
    R = data(name)[0]
    ni = np.bincount(R.item, minlength=R.d2)
    w = (ni.max() / ni[R.item]) ** 0.5 * np.random.default_rng(41).choice(DRAWS, R.nnz)
    w.setflags(write=False)
    return w


def params(row):
    return BIG if row == "big" else ROWS[row]


def wref_run(name, row, w, maxiter=MAXITER, R=None, **kw):
    R = R or data(name)[0]
    p = params(row)
    return ccd_weight_ref(R.d1, R.d2, R.user, R.item, R.val, w, initial(R.d1, p["k"]), p["k"], LAM, maxiter, T=p["T"], eps=p["eps"],
                          nmf=p["nmf"], test=(R.tuser, R.titem, R.tval), **kw)


def plain_run(name, row, maxiter=MAXITER, **kw):
    R = data(name)[0]
    p = params(row)
    return ccd_ref(R.d1, R.d2, R.user, R.item, R.val, initial(R.d1, p["k"]), p["k"], LAM, maxiter, T=p["T"], eps=p["eps"], nmf=p["nmf"],
                   test=(R.tuser, R.titem, R.tval), **kw)


@functools.lru_cache(maxsize=None)
def wstudy(name, row, f32=True):
    """test_ccd_reference.study under parity_weights: the weighted references of one row and the bounds that follow from them.
    The fp32 allowance is for one rounding flip in ONE stored u and its spread: the u of a user of the median length, moved by one
    fp32 ulp at (outer 1, rank 1).  (test_ccd_reference.study also nudges the longest user and a hundred users at once; under these
    weights the longest user's flip alone spreads 600 x further, 9e-5 of the maximum, and an allowance that wide would sit within
    100 x of the seeded defects of the popular items' columns, whose ratings carry little weight: 4e-4 to 4e-3.  The narrower
    allowance asks more of the device, not less; in fp32 it is expected to equal the emulated reference bit for bit.)"""
    R = data(name)[0]
    w = parity_weights(name)
    rng = np.random.default_rng(101)
    ref64 = wref_run(name, row, w)
    others = [wref_run(name, row, w, perm=rng.permutation(R.nnz)) for _ in range(3)] + [wref_run(name, row, w, acc=np.longdouble)]
    for o in others:
        assert counts(o) == counts(ref64), (name, row)              # the same inner iterations and ranks in every order
    b64 = (16 * max(dist(o.W, ref64.W) for o in others), 16 * max(dist(o.H, ref64.H) for o in others),
           max(SUM_FLOOR, 16 * max(scalar_dist(o, ref64) for o in others)))
    out = dict(ref64=ref64, b64=b64)
    if not f32:
        return out
    ref32 = wref_run(name, row, w, store=np.float32)
    same = [wref_run(name, row, w, store=np.float32, perm=rng.permutation(R.nnz)), wref_run(name, row, w, store=np.float32, acc=np.longdouble)]
    bit_identical = all(np.array_equal(o.W, ref32.W) and np.array_equal(o.H, ref32.H) and counts(o) == counts(ref32) for o in same)
    cnt = np.bincount(R.user, minlength=R.d1)
    typical = np.sort(cnt[cnt > 0])[(cnt > 0).sum() // 2]
    choices = [np.array([int(np.flatnonzero(cnt == typical)[0])])]
    nudged = []
    for users in choices:
        def hook(oi, t, us, vs, users=users):
            if oi == 1 and t == 0:
                us[users] = np.nextafter(us[users].astype(np.float32), np.float32(np.inf)).astype(us.dtype)
        nudged.append(wref_run(name, row, w, store=np.float32, hook=hook))
    b32 = (4 * max(dist(o.W, ref32.W) for o in nudged), 4 * max(dist(o.H, ref32.H) for o in nudged),
           max(SUM_FLOOR, 4 * max(scalar_dist(o, ref32) for o in nudged)))
    out.update(ref32=ref32, b32=b32, bit_identical=bit_identical, nudged_counts=[counts(o) == counts(ref32) for o in nudged])
    return out


def same_result(a, b):
    return (np.array_equal(a.W.view(np.uint64), b.W.view(np.uint64)) and np.array_equal(a.H.view(np.uint64), b.H.view(np.uint64))
            and a.recs == b.recs and a.inner == b.inner and a.ranks == b.ranks and a.ratios == b.ratios)


# ---------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("store", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("row", ["default", "nmf"])
def test_all_ones_weights_are_the_unweighted_reference_bit_for_bit(row, store):
    R = data("edge")[0]
    a = wref_run("edge", row, np.ones(R.nnz), store=store)
    b = plain_run("edge", row, store=store)
    assert same_result(a, b)
    assert len(a.recs) == 3 * MAXITER and a.recs[-1][6] > 0            # (every rank ran; the rmse is there)


@pytest.mark.parametrize("store", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("c", [2.0, 0.25])
def test_a_common_power_of_two_scales_the_objective_exactly_and_leaves_the_factors(c, store):
    R = data("edge")[0]
    for row in ("default", "nmf"):
        a = wref_run("edge", row, np.full(R.nnz, c), store=store)
        b = plain_run("edge", row, store=store)
        assert np.array_equal(a.W.view(np.uint64), b.W.view(np.uint64)) and np.array_equal(a.H.view(np.uint64), b.H.view(np.uint64))
        assert counts(a) == counts(b) and a.ratios == b.ratios
        for x, y in zip(a.recs, b.recs):
            assert (x[2], x[3], x[4], x[5]) == (c * y[2], c * y[3], c * y[4], c * y[5]) and x[6] == y[6]     # loss, obj, diff, reg; rmse


def test_parity_weights_span_their_range():
    w = parity_weights("edge")
    R = data("edge")[0]
    assert w.shape == (R.nnz,) and w.min() == 0.25 and 300 < w.max() <= 4 * 8200 ** 0.5
    assert np.all(np.diff(R.user.astype(np.int64) * R.d2 + R.item) > 0)         # the set's order is the training CSR's
    assert len(np.unique(w.astype(np.float32).astype(np.float64) != w)) == 2     # some weights round in fp32, some do not


def test_bounds_of_every_row_and_their_preconditions():
    """The bounds themselves (printed for NOTES.md).  Every stopping ratio is at least 1 % from its threshold and the counts are
    the same in every order (asserted inside wstudy) and in both storage types; fp32 storage is bit-identical across orders."""
    for row in W_ROWS:
        s = wstudy("edge", row)
        print(f"edge/{row} weighted: fp64 bound U {s['b64'][0]:.2e} V {s['b64'][1]:.2e} s {s['b64'][2]:.2e}; fp32 bound U {s['b32'][0]:.2e} "
              f"V {s['b32'][1]:.2e} s {s['b32'][2]:.2e}; inner {s['ref64'].inner} ranks {s['ref64'].ranks}")
        assert s["bit_identical"], row
        for res in (s["ref64"], s["ref32"]):
            assert all(abs(math.log(x)) > 0.01 for x in res.ratios), (row, sorted(res.ratios))
        assert counts(s["ref32"]) == counts(s["ref64"]) and all(s["nudged_counts"]), row
        assert all(math.isfinite(b) for b in s["b64"] + s["b32"]), row
    st = {row: wstudy("edge", row) for row in W_ROWS}
    assert st["default"]["ref64"].inner == 3 * 3 * MAXITER
    assert st["eps05"]["ref64"].inner < 3 * 3 * MAXITER and st["eps05"]["ref64"].ranks == 3 * MAXITER
    assert st["T0"]["ref64"].inner == 0 and st["T1"]["ref64"].inner == 3 * MAXITER and st["k1"]["ref64"].ranks == MAXITER
    nmf = st["nmf"]["ref64"]
    assert nmf.W.min() >= 0 and nmf.H.min() >= 0 and (st["default"]["ref64"].W.min() < 0 or st["default"]["ref64"].H.min() < 0)
    # the weights matter: the weighted model is far from the unweighted one
    assert dist(st["default"]["ref64"].W, plain_run("edge", "default").W) > 1e-2


def test_seeded_defects_land_far_outside_both_bounds():
    """One weight read as 1 in a column of length 1, 65, 4096, 4097 or 8200 on either side, and the rating count in the place of W:
    each at least 100 x outside both bounds in the factors.  Dropping the weights from the loss alone leaves the factors where
    they are and moves obj outside the scalar bound."""
    R, user_of, item_of = data("edge")
    s = wstudy("edge", "default")
    w = parity_weights("edge")
    bU, bV, bs = (max(s["b64"][i], s["b32"][i]) for i in range(3))
    print(f"weighted fp64 bound U {s['b64'][0]:.2e} V {s['b64'][1]:.2e} scalars {s['b64'][2]:.2e}; "
          f"fp32 bound U {s['b32'][0]:.2e} V {s['b32'][1]:.2e} scalars {s['b32'][2]:.2e}")
    smallest = math.inf
    for side, of, col in (("item", item_of, R.item), ("user", user_of, R.user)):
        for L in DEFECT_LENGTHS:
            z = np.flatnonzero(col == of[L])
            assert z.shape[0] == L
            far = z[np.argmax(np.abs(np.log(w[z])))]                  # (a weight that is not 1 already)
            assert not 0.6 < w[far] < 1.7
            bad_w = w.copy()
            bad_w[far] = 1.0
            for store, ref in ((np.float64, s["ref64"]), (np.float32, s["ref32"])):
                bad = wref_run("edge", "default", bad_w, store=store)
                dU, dV = dist(bad.W, ref.W), dist(bad.H, ref.H)
                print(f"defect one weight as 1, {side} L={L} {np.dtype(store).name}: U {dU:.2e} V {dV:.2e}")
                smallest = min(smallest, max(dU, dV))
                assert dU >= 100 * bU or dV >= 100 * bV, (side, L, dU, dV)
    print(f"smallest defect distance {smallest:.2e}")
    for store, ref in ((np.float64, s["ref64"]), (np.float32, s["ref32"])):
        bad = wref_run("edge", "default", w, store=store, defect="count_reg")
        dU, dV = dist(bad.W, ref.W), dist(bad.H, ref.H)
        print(f"defect count regulariser {np.dtype(store).name}: U {dU:.2e} V {dV:.2e}")
        assert dU >= 100 * bU and dV >= 100 * bV
        bad = wref_run("edge", "default", w, store=store, defect="plain_loss")
        assert np.array_equal(bad.W, ref.W) and np.array_equal(bad.H, ref.H) and counts(bad) == counts(ref)
        dobj = min(abs(x[3] - y[3]) / abs(y[3]) for x, y in zip(bad.recs, ref.recs))
        print(f"defect unweighted loss {np.dtype(store).name}: obj moves by {dobj:.2e} at least")
        assert dobj > bs


def csr_order_weights(ds, user, item, w):
    idx, it, _ = ds.csr()
    d2 = ds.dims()[1]
    rows = np.repeat(np.arange(idx.shape[0] - 1, dtype=np.int64), np.diff(idx))
    key = user.astype(np.int64) * d2 + item
    o = np.argsort(key)
    pos = np.searchsorted(key[o], rows * d2 + it)
    assert np.array_equal(key[o][pos], rows * d2 + it)
    return w[o][pos]


def test_match_weights_orders_triplets_and_names_the_offender():
    import primalcr_amd as pcr
    R = ratings("synth3")
    ds = pcr.Dataset.from_ratings(R)
    rng = np.random.default_rng(5)
    w = rng.uniform(0.1, 9.0, R.nnz)
    want = csr_order_weights(ds, R.user, R.item, w)
    p = rng.permutation(R.nnz)
    u, j, ww = R.user[p].copy(), R.item[p].copy(), w[p].copy()
    assert np.array_equal(pcr.match_weights(ds, u, j, ww), want)
    assert np.array_equal(pcr.match_weights(ds, R.user, R.item, w), want)
    have = set((R.user.astype(np.int64) * R.d2 + R.item).tolist())
    free = next(x for x in range(R.d1 * R.d2) if x not in have)
    q = 17
    bu, bj = u.copy(), j.copy()
    bu[q], bj[q] = free // R.d2, free % R.d2
    with pytest.raises(pcr.PcrError, match=rf"error -1: .*triplet {q} \(user {free // R.d2}, item {free % R.d2}\) is not a training rating"):
        pcr.match_weights(ds, bu, bj, ww)
    for bad_u, bad_j in ((R.d1, 0), (0, R.d2), (-1, 0)):
        bu, bj = u.copy(), j.copy()
        bu[q], bj[q] = bad_u, bad_j
        with pytest.raises(pcr.PcrError, match=rf"error -1: .*triplet {q} .*is not a training rating"):
            pcr.match_weights(ds, bu, bj, ww)
    bu, bj = u.copy(), j.copy()
    bu[40], bj[40] = u[3], j[3]
    with pytest.raises(pcr.PcrError, match=rf"error -1: .*triplet 40 \(user {u[3]}, item {j[3]}\) names a training rating a second time"):
        pcr.match_weights(ds, bu, bj, ww)
    with pytest.raises(pcr.PcrError, match=rf"error -1: .*\(user {u[-1]}, item {j[-1]}\) is left without a weight"):
        pcr.match_weights(ds, u[:-1], j[:-1], ww[:-1])


def test_popularity_weights_against_numpy():
    import primalcr_amd as pcr
    R = ratings("synth3")
    ds = pcr.Dataset.from_ratings(R)
    _, it, _ = ds.csr()
    ni = np.bincount(it, minlength=R.d2)
    assert np.array_equal(pcr.rating_weights_popularity(ds, 0.0), np.ones(R.nnz))
    assert np.array_equal(pcr.rating_weights_popularity(ds, 1.0), ni.max() / ni[it])
    for gamma in (0.5, -0.75, 2.5):
        got, want = pcr.rating_weights_popularity(ds, gamma), (ni.max() / ni[it]) ** gamma
        assert np.all(np.abs(got - want) <= 2 * np.spacing(want))       # (two pow()s, each within an ulp of the true value)
        assert got.min() > 0 and len(np.unique(got)) > 5
    for gamma in (math.nan, math.inf, -math.inf):
        with pytest.raises(pcr.PcrError, match="error -1: .*gamma"):
            pcr.rating_weights_popularity(ds, gamma)


def run(cmd, cwd):
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=600)


@pytest.mark.parametrize("args,words", [
    (["-s", "0", "--rating-weights", "w", "--popularity-weights", "0.5"], ("--rating-weights", "--popularity-weights")),
    (["-s", "0", "--rating-weights", "w", "--user-weights", "u"], ("--rating-weights", "--user-weights")),
    (["-s", "0", "--popularity-weights", "0.5", "--normalize", "pairs"], ("--popularity-weights", "--normalize")),
    (["-s", "2", "--rating-weights", "w", "--normalize", "pairs"], ("--rating-weights", "--normalize")),
    (["-s", "2", "--rating-weights", "w"], ("--rating-weights", "-s 0")),
    (["-s", "1", "--popularity-weights", "0.5"], ("--popularity-weights", "-s 0")),
    (["--popularity-weights", "0.5"], ("--popularity-weights", "-s 0")),                  # (the default solver is -s 2)
    (["-s", "0", "--popularity-weights", "nan"], ("--popularity-weights", "finite")),
    (["-s", "0", "--popularity-weights", "0.5x"], ("--popularity-weights", "finite")),
])
def test_cli_refuses_before_any_device_work(args, words, tmp_path):
    """Exit 1 and one line, before the model file is opened, a data set read or a device touched (the data directory does not exist)."""
    model = tmp_path / "m.model"
    r = run([TRAIN] + args + [str(tmp_path / "no_data"), str(model)], tmp_path)
    assert r.returncode == 1 and len(r.stderr.strip().splitlines()) == 1, r.stderr
    assert all(x in r.stderr for x in words), r.stderr
    assert "can't open" not in r.stderr and not model.exists()


def test_usage_text_and_exports(tmp_path):
    import primalcr_amd as pcr
    r = run([TRAIN], tmp_path)
    assert r.returncode == 1 and "--rating-weights file" in r.stdout and "--popularity-weights gamma" in r.stdout
    for name in ("pcr_solver_set_rating_weights", "pcr_dataset_match_weights", "pcr_rating_weights_popularity"):
        assert hasattr(pcr.lib(), name), name
    header = open(os.path.join(ROOT, "include", "primalcr.h")).read()
    stubs = open(os.path.join(ROOT, "primalcr_amd", "csrc", "sanitize", "device_absent.cpp")).read()
    assert "int pcr_solver_set_rating_weights(pcr_solver *s, const double *w" in header
    assert "NO_SOLVER(pcr_solver_set_rating_weights, pcr_solver*, const double*)" in stubs
    assert "pcr_dataset_match_weights" not in stubs and "pcr_rating_weights_popularity" not in stubs       # ([host]: the real ones)


# ---------------------------------------------------------------------------------------------------------------- GPU
def wsolver(name, row, f64, w, maxiter=MAXITER, U0=None, profile=False, **kw):
    R = data(name)[0]
    p = params(row)
    s = solver(dataset(name), initial(R.d1, p["k"]) if U0 is None else U0, p["k"], f64, maxiter, p["T"], eps=p["eps"], nmf=p["nmf"], **kw)
    if profile:
        s.profile(True)
    if w is not None:
        s.set_rating_weights(w)
    assert s.counter("ccd_rating_weights") == (0 if w is None else 1)
    return s


def finish(s, close=True):
    recs, lines = s.train()
    assert s.counter("ccd_residual_mismatch") == 0
    U, V = s.get_factors()
    if close:
        s.close()
    return U, V, recs, [re.sub(r"time \S+ ", "", ln) for ln in lines]


def same_bits(a, b):
    return np.array_equal(bits(a, True), bits(b, True))


def figures(recs):
    return [(r["obj"], r["cg_v"], r["cg_u"]) for r in recs[1:]]


def assert_within(got, want, bound, lengths, what):
    """Largest distance relative to the reference's maximum, as dist(); a failure names the first wrong column and its length."""
    m = np.abs(want).max()
    d = np.abs(got - want).max(axis=1) / (m if m > 0 else 1.0)
    bad = np.flatnonzero(~(d <= bound))
    assert bad.size == 0, (f"{what}: {bad.size} columns beyond {bound:.2e}, first column {bad[0]} with {lengths[bad[0]]} ratings: "
                           f"{got[bad[0]]!r} instead of {want[bad[0]]!r} ({d[bad[0]]:.2e})")


@pytest.mark.gpu
@pytest.mark.parametrize("f64", [True, False], ids=["f64", "f32"])
@pytest.mark.parametrize("row", ["default", "nmf"])
def test_all_ones_weights_take_the_weighted_kernels_and_give_the_unweighted_bits(row, f64):
    R = data("edge")[0]
    plain = wsolver("edge", row, f64, None, profile=True, verbose=1)
    U0, V0, recs0, lines0 = finish(plain, close=False)
    prof0 = plain.profile_all()
    plain.close()
    ones = wsolver("edge", row, f64, np.ones(R.nnz), profile=True, verbose=1)
    U1, V1, recs1, lines1 = finish(ones, close=False)
    prof1 = ones.profile_all()
    ones.close()
    assert same_bits(U1, U0) and same_bits(V1, V0)
    assert figures(recs1) == figures(recs0) and lines1 == lines0 and len(lines0) == 3 * MAXITER
    for slot in ("ccd/vsweep", "ccd/usweep", "ccd/resid", "ccd/init"):
        assert prof1.get(slot + ".w", (0, 0))[1] > 0 and prof1.get(slot, (0, 0))[1] == 0, prof1
        assert prof0.get(slot, (0, 0))[1] > 0 and prof0.get(slot + ".w", (0, 0))[1] == 0, prof0
        assert prof1[slot + ".w"][1] == prof0[slot][1]
    assert prof1["ccd/vsweep.w"][1] == 3 * 3 * MAXITER and prof1["ccd/resid.w"][1] == 3 * MAXITER      # 3 T + 3 launches per rank


@pytest.mark.gpu
@pytest.mark.parametrize("f64", [True, False], ids=["f64", "f32"])
@pytest.mark.parametrize("c", [2.0, 0.25])
def test_a_common_power_of_two_scales_the_device_objective_exactly(c, f64):
    R = data("edge")[0]
    for row in ("default", "nmf"):
        U0, V0, recs0, _ = finish(wsolver("edge", row, f64, None))
        U1, V1, recs1, _ = finish(wsolver("edge", row, f64, np.full(R.nnz, c)))
        assert same_bits(U1, U0) and same_bits(V1, V0)
        assert figures(recs1) == [(c * o, a, b) for o, a, b in figures(recs0)]


def weighted_parity(name, row, f64):
    p = params(row)
    s = wstudy(name, row) if name == "edge" else wstudy(name, row, False)
    ref, (bU, bV, bs) = (s["ref64"], s["b64"]) if f64 else (s["ref32"], s["b32"])
    R = data(name)[0]
    U, V, recs, lines = finish(wsolver(name, row, f64, parity_weights(name), verbose=1, do_predict=1 if name == "edge" else 0))
    dU, dV = dist(U, ref.W), dist(V, ref.H)
    last = [[r for r in ref.recs if r[0] == oi][-1] for oi in range(1, MAXITER + 1)]
    dobj = max(abs(recs[oi]["obj"] - last[oi - 1][3]) / abs(last[oi - 1][3]) for oi in range(1, MAXITER + 1))
    diff_bits = int((bits(U, f64) != bits(ref.W, f64)).sum() + (bits(V, f64) != bits(ref.H, f64)).sum())
    print(f"weighted {name}/{row} {'f64' if f64 else 'f32'}: U {dU:.2e} / bound {bU:.2e}, V {dV:.2e} / bound {bV:.2e}, obj {dobj:.2e} / bound {bs:.2e}, "
          f"{diff_bits} of {U.size + V.size} entries not bit-equal")
    assert [recs[oi]["cg_v"] for oi in range(1, MAXITER + 1)] == [r[7] for r in last]
    assert [recs[oi]["cg_u"] for oi in range(1, MAXITER + 1)] == [sum(1 for r in ref.recs if r[0] <= oi) for oi in range(1, MAXITER + 1)]
    assert_within(V, ref.H, bV, np.bincount(R.item, minlength=R.d2), "V")
    assert_within(U, ref.W, bU, np.bincount(R.user, minlength=R.d1), "U")
    assert dobj <= bs
    printed = parse_lines([re.sub(r"^(iter \d+ rank \d+ )", r"\1time 0 ", ln) for ln in lines])
    assert_lines(printed, ref.recs, bs, rmse=f64 and name == "edge")
    assert p["k"] * MAXITER >= len(printed) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("f64", [True, False], ids=["f64", "f32"])
@pytest.mark.parametrize("row", W_ROWS)
def test_parity_with_the_weighted_reference_on_the_edge_set(row, f64):
    weighted_parity("edge", row, f64)


@pytest.mark.gpu
def test_weighted_sums_over_many_partials_on_the_big_set():
    """fp64, k = 2, T = 2: the W arrays and the weighted loss partials above 256 blocks and at the cap of parts()."""
    weighted_parity("big", "big", True)


@pytest.mark.gpu
def test_life_cycle_of_the_weights():
    import primalcr_amd as pcr
    R = data("edge")[0]
    w = parity_weights("edge")
    U0 = initial(R.d1, 3)
    Uw, Vw, recsw, _ = finish(wsolver("edge", "default", True, w))
    Up, Vp, recsp, _ = finish(wsolver("edge", "default", True, None))
    assert not same_bits(Uw, Up)
    # None after weights: the unweighted bits
    s = wsolver("edge", "default", True, w)
    finish(s, close=False)
    s.set_rating_weights(None)
    assert s.counter("ccd_rating_weights") == 0
    s.set_factors(U0, None)
    U, V, recs, _ = finish(s, close=False)
    assert same_bits(U, Up) and same_bits(V, Vp) and figures(recs) == figures(recsp)
    # weights on a solver that has trained, then train(): a fresh weighted solver from the same U
    s.set_rating_weights(w)
    assert s.counter("ccd_rating_weights") == 1
    U, V, recs, _ = finish(s, close=False)
    Uf, Vf, recsf, _ = finish(wsolver("edge", "default", True, w, U0=Up))
    assert same_bits(U, Uf) and same_bits(V, Vf) and figures(recs) == figures(recsf)
    # weights survive set_factors and set_ccd_params
    s.set_factors(U0, None)
    s.set_ccd_params(maxinneriter=3, eps=1e-3, do_nmf=0)
    assert s.counter("ccd_rating_weights") == 1
    U, V, recs, _ = finish(s, close=False)
    assert same_bits(U, Uw) and same_bits(V, Vw) and figures(recs) == figures(recsw)
    # a vector with one bad weight: PCR_ERR_ARG, and the former weights stay
    for bad in (0.0, -1.0, math.nan, math.inf, -math.inf):
        bw = np.full(R.nnz, 3.0)
        bw[R.nnz // 2] = bad
        with pytest.raises(pcr.PcrError, match=rf"error -1: .*rating {R.nnz // 2} "):
            s.set_rating_weights(bw)
        assert s.counter("ccd_rating_weights") == 1
    with pytest.raises(ValueError):
        s.set_rating_weights(np.ones(R.nnz - 1))
    s.set_factors(U0, None)
    U, V, recs, _ = finish(s)
    assert same_bits(U, Uw) and same_bits(V, Vw) and figures(recs) == figures(recsw)
    # train() then iterate(2) is a three-iteration train() under weights
    U3, V3, recs3, _ = finish(wsolver("edge", "default", True, w, maxiter=3))
    s = wsolver("edge", "default", True, w, maxiter=1)
    recs1, _ = s.train()
    it = s.iterate(2)
    assert s.counter("ccd_residual_mismatch") == 0
    U, V = s.get_factors()
    s.close()
    assert same_bits(U, U3) and same_bits(V, V3)
    assert [(recs1[1]["obj"], recs1[1]["cg_v"])] + [(r["obj"], r["cg_v"]) for r in it] == [(r["obj"], r["cg_v"]) for r in recs3[1:]]


@pytest.mark.gpu
def test_fp32_weights_that_do_not_survive_rounding_are_refused():
    """The weights are stored in the solver's precision: one that is finite and > 0 in fp64 but 0 or infinite in fp32 is refused
    on an fp32 solver and taken on an fp64 one."""
    import primalcr_amd as pcr
    R = data("edge")[0]
    for bad in (1e-60, 1e60):
        bw = np.ones(R.nnz)
        bw[5] = bad
        s = wsolver("edge", "default", False, None)
        with pytest.raises(pcr.PcrError, match="error -1: .*rating 5 "):
            s.set_rating_weights(bw)
        assert s.counter("ccd_rating_weights") == 0
        s.close()
    s = wsolver("edge", "default", True, None)
    bw = np.ones(R.nnz)
    bw[5] = 1e-60
    s.set_rating_weights(bw)
    assert s.counter("ccd_rating_weights") == 1
    s.close()


@pytest.mark.gpu
def test_a_ranking_solver_refuses_rating_weights_with_the_reason():
    import primalcr_amd as pcr
    R = ratings("synth3")
    ds = pcr.Dataset.from_ratings(R)
    s = pcr.Solver(ds, pcr.Parameter(solver_type=pcr.PCR_SOLVER_PCRPP, k=4))
    with pytest.raises(pcr.PcrError, match="error -7: .*pcr_solver_set_user_weights"):
        s.set_rating_weights(np.ones(R.nnz))
    with pytest.raises(pcr.PcrError, match="error -7: .*pcr_solver_set_user_weights"):
        s.set_rating_weights(None)
    with pytest.raises(pcr.PcrError, match="error -6: .*ccd_rating_weights"):
        s.counter("ccd_rating_weights")
    s.close()
    c = pcr.Solver(ds, pcr.Parameter(solver_type=pcr.PCR_SOLVER_CCDR1, k=4))
    with pytest.raises(pcr.PcrError, match="error -7"):                  # (per-user weights stay refused on CCDR1)
        c.set_user_weights(np.ones(R.d1))
    c.close()


def binding_run(R, k, f64, weights, lam=0.05, maxiter=3, T=3):
    import primalcr_amd as pcr
    ds = pcr.Dataset.from_ratings(R)
    p = pcr.Parameter(solver_type=pcr.PCR_SOLVER_CCDR1, k=k, precision=pcr.PCR_F64 if f64 else pcr.PCR_F32, maxiter=maxiter, do_predict=1,
                      verbose=1, **{"lambda": lam})
    s = pcr.Solver(ds, p)
    s.set_ccd_params(maxinneriter=T, eps=1e-3, do_nmf=0)
    s.set_factors(pcr.initial_col(R.d1, k), None)
    s.set_rating_weights(weights(ds) if callable(weights) else weights)
    return finish(s)


@pytest.mark.gpu
@pytest.mark.parametrize("f64", [True, False], ids=["f64", "f32"])
def test_cli_rating_weights_and_popularity_weights_equal_the_binding(f64, tmp_path):
    import primalcr_amd as pcr
    R = ratings("synth3")
    assert (R.d1, R.d2, R.nnz) == (200, 120, 4000)
    d = synth.write_dir(R, str(tmp_path / "data"))
    rng = np.random.default_rng(8)
    w = rng.choice(DRAWS, R.nnz) * rng.uniform(0.5, 1.5, R.nnz)
    p = rng.permutation(R.nnz)
    wfile = tmp_path / "weights.ratings"
    wfile.write_text("".join(f"{u + 1} {j + 1} {x:.17g}\n" for u, j, x in zip(R.user[p].tolist(), R.item[p].tolist(), w[p].tolist())))
    common = ["-s", "0", "-k", "4", "-l", "0.05", "-t", "3", "-T", "3"] + (["--f64"] if f64 else [])
    for extra, weights in ((["--rating-weights", str(wfile)], (R.user, R.item, w)),
                           (["--popularity-weights", "0.5"], lambda ds: pcr.rating_weights_popularity(ds, 0.5))):
        model = tmp_path / "cli.model"
        r = run([TRAIN] + common + extra + [d, str(model)], tmp_path)
        assert r.returncode == 0, r.stderr
        out = r.stdout.rstrip("\n").split("\n")
        assert out[0] == "starts!" and out[-1].startswith("Wall-time: ")
        U, V, _, lines = binding_run(R, 4, f64, weights)
        assert [re.sub(r"time \S+ ", "", ln) for ln in out[1:-1]] == lines and len(lines) == 4 * 3
        mine = tmp_path / "binding.model"
        pcr.model_save(str(mine), U, V)
        assert model.read_bytes() == mine.read_bytes()
    # the weights changed the model: the unweighted run writes other bytes
    r = run([TRAIN] + common + [d, str(tmp_path / "plain.model")], tmp_path)
    assert r.returncode == 0 and (tmp_path / "plain.model").read_bytes() != (tmp_path / "cli.model").read_bytes()
