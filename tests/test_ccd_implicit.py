"""Implicit-feedback CCDR1 (pcr_solver_set_implicit) against the numpy reference of tests/ccd_implicit_ref.py (written from
the definition: a dense prediction masked to the unrated cells) on the small sets of tests/ccd_implicit_data.py.

CPU part: in fp64 the implicit reference on the sparse set equals tests/ccd_weight_ref.py on the COMPLETED set (every unrated cell a
rating 0 of weight alpha) within 16 x that reference's own spread over summation orders and a long-double run; on a fully rated set
it is ccd_weight_ref bit for bit; a common power of two on (c, alpha) leaves the factors and scales the scalars exactly; the bounds
of the GPU part are computed from the reference alone (fp64: 16 x the order spread; fp32: 4 x the spread of a one-ulp nudge of one
stored u; scalars with the 64 x 2^-53 floor) -- no tolerance is a literal; four seeded defects land at least 100 x outside them; the
CLI's refusals, the export, the sanitizer targets.
GPU part (-m gpu): the Python binding and omp-pmf-train against that reference, against the weighted solver on the completed set
and against the explicit solver.
"""
import functools
import math
import os
import re
import subprocess

import numpy as np
import pytest

from ccd_data import ratings
from ccd_implicit_data import LONG_DEGREES, completed, full_set, long_set, wide_set
from ccd_implicit_ref import ccd_implicit_ref
from ccd_weight_ref import ccd_weight_ref
from conftest import BIN_DIR, ROOT
from primalcr_amd import synth
from test_ccd_reference import LAM, ROWS, SUM_FLOOR, assert_lines, bits, counts, dist, half_ulp10, initial, parse_lines, scalar_dist

TRAIN = os.path.join(BIN_DIR, "omp-pmf-train")
ALPHA = 0.3                                  # (not a power of two: it rounds in fp32 storage)
# the parameter rows: those of tests/test_ccd_reference.py that the issue names (two outer iterations each) and the two large ranks
# (k = 65: more columns than lanes, ragged ld; k = 100: the workload's rank; one outer iteration of T = 2 keeps the dense reference
# cheap).  eps of the large ranks was picked on the CPU so that no stopping ratio sits near its threshold: at 1e-4 every rank runs (the
# nearest ratio is a factor e^0.9 away), at 1e-2 ("k65stop") ranks break at inner iteration 1 and the rest are skipped (e^0.05 away).
IROWS = {r: dict(ROWS[r], maxiter=2) for r in ("default", "nmf", "T0", "T1", "k1")}
IROWS["k65"] = dict(k=65, T=2, eps=1e-4, nmf=0, maxiter=1)
IROWS["k65stop"] = dict(k=65, T=2, eps=1e-2, nmf=0, maxiter=1)
IROWS["k100"] = dict(k=100, T=2, eps=1e-4, nmf=0, maxiter=1)
TIES = [(r, False) for r in ("default", "nmf", "T0", "T1", "k1")] + [("default", True), ("nmf", True)]
# (row, with rating weights) of the GPU parity tests
PARITY = [(r, False) for r in IROWS] + [("default", True), ("nmf", True), ("k100", True)]
DRAWS = np.array([0.25, 0.5, 1.0, 2.0, 4.0])
DEFECTS = ("no_obs_correction", "obs_reg", "empty_zero", "stale_gram")


# ------------------------------------------------------------------------------------------------------------ helpers
def data(name):
    return {"long": long_set, "wide": wide_set, "full": full_set}[name]()


def rset(name):
    d = data(name)
    return d if name == "full" else d[0]


@functools.lru_cache(maxsize=None)
def weights(name):
    """Seeded rating weights in the order of the set's ratings (the training CSR's): a draw from {1/4 .. 4} times uniform(0.5, 1.5)."""
    R = rset(name)
    rng = np.random.default_rng(43)
    w = rng.choice(DRAWS, R.nnz) * rng.uniform(0.5, 1.5, R.nnz)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def start(name, k, heavy=False):
    """The initial U: initial_col's; `heavy`: with the rows of the EMPTY users multiplied by 1024.  An empty column's minimiser is exactly 0
    from the first sweep on (training starts from V = 0, so its p^ is 0 in every rank), whatever the data: what the update of an empty
    column does shows in its fundec alone, h (old - 0)^2 at the first inner iteration of every rank of outer iteration 1.  With heavy
    rows that term is large enough to decide where the ranks stop."""
    U0 = initial(rset(name).d1, k).copy()
    if heavy:
        U0[data(name)[2]] *= 1024.0
    U0.setflags(write=False)
    return U0


def iref_run(name, row, weighted=False, alpha=ALPHA, w=None, heavy=False, **kw):
    R = rset(name)
    p = IROWS[row]
    if w is None and weighted:
        w = weights(name)
    return ccd_implicit_ref(R.d1, R.d2, R.user, R.item, R.val, w, alpha, start(name, p["k"], heavy), p["k"], LAM, p["maxiter"], T=p["T"],
                            eps=p["eps"], nmf=p["nmf"], test=(R.tuser, R.titem, R.tval), **kw)


def wref_run(R, row, w, **kw):
    p = IROWS[row]
    return ccd_weight_ref(R.d1, R.d2, R.user, R.item, R.val, w, initial(R.d1, p["k"]), p["k"], LAM, p["maxiter"], T=p["T"], eps=p["eps"],
                          nmf=p["nmf"], test=(R.tuser, R.titem, R.tval), **kw)


def spread(ref, others, factor):
    return (factor * max(dist(o.W, ref.W) for o in others), factor * max(dist(o.H, ref.H) for o in others),
            max(SUM_FLOOR, factor * max(scalar_dist(o, ref) for o in others)))


@functools.lru_cache(maxsize=None)
def completed_study(name, row, weighted):
    """ccd_weight_ref on the completed set, and 16 x its spread over three orders of the ratings and a long-double run."""
    R = rset(name)
    C, cw = completed(R, weights(name) if weighted else None, ALPHA)
    rng = np.random.default_rng(103)
    ref = wref_run(C, row, cw)
    others = [wref_run(C, row, cw, perm=rng.permutation(C.nnz)) for _ in range(3)] + [wref_run(C, row, cw, acc=np.longdouble)]
    for o in others:
        assert counts(o) == counts(ref), (name, row)
    return dict(ref=ref, bound=spread(ref, others, 16))


@functools.lru_cache(maxsize=None)
def istudy(name, row, weighted=False, heavy=False):
    """test_ccd_weights.wstudy for the implicit reference: dict(ref64, b64, ref32, b32, bit_identical, nudged_counts).  The fp32
    allowance is for one rounding flip in ONE stored u and its spread: the u of a user of the median length, moved by one fp32 ulp at
    (outer 1, rank 1)."""
    R = rset(name)
    rng = np.random.default_rng(101)
    ref64 = iref_run(name, row, weighted, heavy=heavy)
    others = [iref_run(name, row, weighted, heavy=heavy, perm=rng.permutation(R.nnz)) for _ in range(3)] + [iref_run(name, row, weighted, heavy=heavy, acc=np.longdouble)]
    for o in others:
        assert counts(o) == counts(ref64), (name, row)              # the same inner iterations and ranks in every order
    out = dict(ref64=ref64, b64=spread(ref64, others, 16))
    ref32 = iref_run(name, row, weighted, heavy=heavy, store=np.float32)
    same = [iref_run(name, row, weighted, heavy=heavy, store=np.float32, perm=rng.permutation(R.nnz)), iref_run(name, row, weighted, heavy=heavy, store=np.float32, acc=np.longdouble)]
    out["order32"] = spread(ref32, same, 1)
    out["counts32"] = all(counts(o) == counts(ref32) for o in same)
    cnt = np.bincount(R.user, minlength=R.d1)
    typical = np.sort(cnt[cnt > 0])[(cnt > 0).sum() // 2]
    users = np.array([int(np.flatnonzero(cnt == typical)[0])])

    def hook(oi, t, us, vs):
        if oi == 1 and t == 0:
            us[users] = np.nextafter(us[users].astype(np.float32), np.float32(np.inf)).astype(us.dtype)
    nudged = [iref_run(name, row, weighted, heavy=heavy, store=np.float32, hook=hook)]
    out.update(ref32=ref32, b32=spread(ref32, nudged, 4), nudged_counts=[counts(o) == counts(ref32) for o in nudged])
    return out


def same_result(a, b):
    return (np.array_equal(a.W.view(np.uint64), b.W.view(np.uint64)) and np.array_equal(a.H.view(np.uint64), b.H.view(np.uint64))
            and a.recs == b.recs and a.inner == b.inner and a.ranks == b.ranks and a.ratios == b.ratios)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_the_sets_hold_what_they_claim():
    R, item_of, empty_users, empty_items, full_user = data("long")
    cu, ci = np.bincount(R.user, minlength=R.d1), np.bincount(R.item, minlength=R.d2)
    assert R.d1 * R.d2 <= 4200 * 40 and [ci[item_of[L]] for L in LONG_DEGREES] == list(LONG_DEGREES)
    assert len(empty_users) >= 3 and len(empty_items) >= 3 and np.all(cu[empty_users] == 0) and np.all(ci[empty_items] == 0)
    assert (cu == 0).sum() == len(empty_users) and (ci == 0).sum() == len(empty_items)
    assert cu[full_user] == R.d2 - len(empty_items) == cu.max()              # (no row can be fuller while items are empty)
    assert np.all(np.diff(R.user.astype(np.int64) * R.d2 + R.item) > 0)      # the set's order is the training CSR's
    assert 0 < len(R.tuser) <= 64 and np.all(np.diff(R.tuser) >= 0)
    W, user_of, wempty_users, wempty_items, _ = data("wide")
    assert (W.d1, W.d2, W.nnz) == (R.d2, R.d1, R.nnz) and np.all(np.diff(W.user.astype(np.int64) * W.d2 + W.item) > 0)
    A, B = np.zeros((R.d1, R.d2)), np.zeros((W.d1, W.d2))
    A[R.user, R.item] = R.val; B[W.user, W.item] = W.val
    assert np.array_equal(A.T, B) and np.array_equal(wempty_users, empty_items) and np.array_equal(wempty_items, empty_users)
    F = data("full")
    assert (F.d1, F.d2, F.nnz) == (12, 9, 108) and np.unique(F.user.astype(np.int64) * F.d2 + F.item).shape[0] == 108
    C, cw = completed(R, weights("long"), ALPHA)
    assert C.nnz == R.d1 * R.d2 and (cw == ALPHA).sum() == C.nnz - R.nnz and (C.val == 0).sum() == C.nnz - R.nnz


@pytest.mark.parametrize("row,weighted", TIES, ids=[r + ("-w" if w else "") for r, w in TIES])
@pytest.mark.parametrize("name", ["long", "wide"])
def test_the_implicit_reference_is_the_weighted_reference_on_the_completed_set(name, row, weighted):
    """The tie to the held reference: factors, loss, obj, reg, rmse and the counts, inside 16 x the completed reference's own spread."""
    c = completed_study(name, row, weighted)
    got = iref_run(name, row, weighted)
    bU, bV, bs = c["bound"]
    dU, dV, ds = dist(got.W, c["ref"].W), dist(got.H, c["ref"].H), scalar_dist(got, c["ref"])
    print(f"tie {name}/{row}/{'w' if weighted else 'plain'}: U {dU:.2e} / {bU:.2e}, V {dV:.2e} / {bV:.2e}, scalars {ds:.2e} / {bs:.2e}")
    assert counts(got) == counts(c["ref"])
    assert dU <= bU and dV <= bV and ds <= bs


@pytest.mark.parametrize("store", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("alpha", [ALPHA, 7.0])
def test_on_a_fully_rated_set_the_implicit_reference_is_the_weighted_one_bit_for_bit(alpha, store):
    F = data("full")
    for row in ("default", "nmf"):
        for w in (None, weights("full")):
            a = iref_run("full", row, alpha=alpha, w=w, store=store)
            b = wref_run(F, row, np.ones(F.nnz) if w is None else w, store=store)
            assert same_result(a, b) and len(a.recs) == 3 * 2


@pytest.mark.parametrize("store", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("c", [2.0, 0.25])
def test_a_common_power_of_two_on_weights_and_alpha_scales_exactly(c, store):
    for name in ("long", "wide"):
        for row in ("default", "nmf"):
            b = iref_run(name, row, True, store=store)
            a = iref_run(name, row, alpha=c * ALPHA, w=c * weights(name), store=store)
            assert np.array_equal(a.W.view(np.uint64), b.W.view(np.uint64)) and np.array_equal(a.H.view(np.uint64), b.H.view(np.uint64))
            assert counts(a) == counts(b) and a.ratios == b.ratios
            for x, y in zip(a.recs, b.recs):
                assert (x[2], x[3], x[4], x[5]) == (c * y[2], c * y[3], c * y[4], c * y[5]) and x[6] == y[6]     # loss, obj, diff, reg; rmse


def test_bounds_of_every_row_and_their_preconditions():
    """The bounds of the GPU part (printed for NOTES.md) and what they rest on: every stopping ratio is at least 1 % from its
    threshold, the counts are the same in every order (asserted inside istudy) and in both storage types."""
    for name in ("long", "wide"):
        for row, weighted in PARITY:
            s = istudy(name, row, weighted)
            print(f"{name}/{row}/{'w' if weighted else 'plain'}: fp64 bound U {s['b64'][0]:.2e} V {s['b64'][1]:.2e} s {s['b64'][2]:.2e}; fp32 bound U "
                  f"{s['b32'][0]:.2e} V {s['b32'][1]:.2e} s {s['b32'][2]:.2e}; fp32 order spread U {s['order32'][0]:.2e} V {s['order32'][1]:.2e}; "
                  f"inner {s['ref64'].inner} ranks {s['ref64'].ranks}")
            for res in (s["ref64"], s["ref32"]):
                assert all(abs(math.log(x)) > 0.01 for x in res.ratios), (name, row, sorted(res.ratios, key=lambda x: abs(math.log(x)))[:3])
            assert counts(s["ref32"]) == counts(s["ref64"]) and all(s["nudged_counts"]) and s["counts32"], (name, row)
            assert all(math.isfinite(b) for b in s["b64"] + s["b32"]), (name, row)
            p = IROWS[row]
            assert (s["ref64"].ranks < p["k"] * p["maxiter"] and s["ref64"].inner < 2 * s["ref64"].ranks) if row == "k65stop" else \
                   (s["ref64"].ranks == p["k"] * p["maxiter"] and s["ref64"].inner == p["T"] * s["ref64"].ranks)
    # empty columns: updated like every other, and their minimiser is exactly 0 (see start()); without a sweep they keep U0
    R, _, empty_users, empty_items, _ = data("long")
    ref = istudy("long", "default")["ref64"]
    assert not ref.W[empty_users].any() and not ref.H[empty_items].any() and np.all(start("long", 3)[empty_users] != 0)
    assert np.array_equal(istudy("long", "T0")["ref64"].W[empty_users], start("long", 3)[empty_users])
    for name in ("long", "wide"):
        s = istudy(name, "default", heavy=True)
        print(f"{name}/default/heavy empty users: fp64 bound U {s['b64'][0]:.2e} V {s['b64'][1]:.2e} s {s['b64'][2]:.2e}; fp32 bound U "
              f"{s['b32'][0]:.2e} V {s['b32'][1]:.2e} s {s['b32'][2]:.2e}; inner {s['ref64'].inner} ranks {s['ref64'].ranks}")
        for res in (s["ref64"], s["ref32"]):
            assert all(abs(math.log(x)) > 0.01 for x in res.ratios), name
        assert counts(s["ref32"]) == counts(s["ref64"]) and all(s["nudged_counts"]) and s["counts32"], name
        assert s["ref64"].inner < 3 * 3 * 2                                                   # ranks stop early
    nmf = istudy("long", "nmf")["ref64"]
    assert nmf.W.min() >= 0 and nmf.H.min() >= 0 and (ref.W.min() < 0 or ref.H.min() < 0)


def test_seeded_defects_land_far_outside_both_bounds():
    """Each of the four defects at least 100 x outside the fp64 and the fp32 bound, in the factors, on at least one set.  "empty_zero"
    is measured from the heavy start (see start()): from initial_col's U it moves no factor and no count on any data."""
    for defect in DEFECTS:
        best = 0.0
        heavy = defect == "empty_zero"
        for name in ("long", "wide"):
            s = istudy(name, "default", heavy=heavy)
            bU, bV = max(s["b64"][0], s["b32"][0]), max(s["b64"][1], s["b32"][1])
            worst = math.inf
            for store, ref in ((np.float64, s["ref64"]), (np.float32, s["ref32"])):
                bad = iref_run(name, "default", store=store, defect=defect, heavy=heavy)
                dU, dV = dist(bad.W, ref.W), dist(bad.H, ref.H)
                print(f"defect {defect} {name} {np.dtype(store).name}: U {dU:.2e} ({dU / bU:.1e} x bound) V {dV:.2e} ({dV / bV:.1e} x bound)")
                worst = min(worst, max(dU / bU, dV / bV))
            best = max(best, worst)
        assert best >= 100, (defect, best)


def run(cmd, cwd):
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=600)


@pytest.mark.parametrize("args,words", [
    (["-s", "2", "--implicit", "0.5"], ("--implicit", "-s 0")),
    (["-s", "1", "--implicit", "0.5"], ("--implicit", "-s 0")),
    (["--implicit", "0.5"], ("--implicit", "-s 0")),                                        # (the default solver is -s 2)
    (["-s", "0", "--implicit", "nan"], ("--implicit", "finite")),
    (["-s", "0", "--implicit", "inf"], ("--implicit", "finite")),
    (["-s", "0", "--implicit", "-1"], ("--implicit", "finite")),
    (["-s", "0", "--implicit", "0.5x"], ("--implicit", "finite")),
    (["-s", "0", "--implicit", "1e-60"], ("--implicit", "finite", "fp32")),               # (0 as stored without --f64)
    (["-s", "0", "--implicit", "1e60"], ("--implicit", "finite", "fp32")),
    (["-s", "0", "--implicit", "0.5", "--user-weights", "u"], ("--user-weights", "-s 0")),
])
def test_cli_refuses_before_any_device_work(args, words, tmp_path):
    """Exit 1 and one line, before the model file is opened, a data set read or a device touched (the data directory does not exist)."""
    model = tmp_path / "m.model"
    r = run([TRAIN] + args + [str(tmp_path / "no_data"), str(model)], tmp_path)
    assert r.returncode == 1 and len(r.stderr.strip().splitlines()) == 1, r.stderr
    assert all(x in r.stderr for x in words), r.stderr
    assert "can't open" not in r.stderr and not model.exists()


def test_usage_text_and_export():
    import primalcr_amd as pcr
    r = run([TRAIN], ROOT)
    assert r.returncode == 1 and "--implicit alpha" in r.stdout
    assert hasattr(pcr.lib(), "pcr_solver_set_implicit")
    header = open(os.path.join(ROOT, "include", "primalcr.h")).read()
    stubs = open(os.path.join(ROOT, "primalcr_amd", "csrc", "sanitize", "device_absent.cpp")).read()
    assert "int pcr_solver_set_implicit(pcr_solver *s, double alpha);" in header
    assert "NO_SOLVER(pcr_solver_set_implicit, pcr_solver*, double)" in stubs


def test_sanitizer_host_targets_still_build():
    """make asan / make tsan (host code only): the new entry point resolves in the device-absent library and the CLI links against it."""
    r = run(["make", "-s", "-C", os.path.join(ROOT, "primalcr_amd", "csrc"), "asan", "tsan"], ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    san = os.path.join(ROOT, "build_san", "asan")
    sym = run(["nm", "-D", "--defined-only", os.path.join(san, "libprimalcr.so")], ROOT)
    assert " T pcr_solver_set_implicit" in sym.stdout
    r = run([os.path.join(san, "omp-pmf-train"), "-s", "2", "--implicit", "1", "no_data", "m"], ROOT)
    assert r.returncode == 1 and "--implicit" in r.stderr and "ERROR" not in r.stderr            # (refused; no sanitizer report)


# ---------------------------------------------------------------------------------------------------------------- GPU
@functools.lru_cache(maxsize=None)
def dataset(name):
    import primalcr_amd as pcr
    return pcr.Dataset.from_ratings(rset(name))


def make_solver(ds, d1, row, f64, alpha=ALPHA, w=None, U0=None, maxiter=None, verbose=0, do_predict=0, profile=False):
    import primalcr_amd as pcr
    p = IROWS[row]
    prm = pcr.Parameter(solver_type=pcr.PCR_SOLVER_CCDR1, k=p["k"], precision=pcr.PCR_F64 if f64 else pcr.PCR_F32,
                        maxiter=p["maxiter"] if maxiter is None else maxiter, do_predict=do_predict, verbose=verbose, **{"lambda": LAM})
    s = pcr.Solver(ds, prm)
    s.set_ccd_params(maxinneriter=p["T"], eps=p["eps"], do_nmf=p["nmf"])
    s.set_factors(initial(d1, p["k"]) if U0 is None else U0, None)
    if profile:
        s.profile(True)
    if w is not None:
        s.set_rating_weights(w)
    if alpha is not None:
        s.set_implicit(alpha)
    return s


def isolver(name, row, f64, weighted=False, heavy=False, **kw):
    return make_solver(dataset(name), rset(name).d1, row, f64, w=weights(name) if weighted else None, U0=start(name, IROWS[row]["k"], heavy), **kw)


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
    m = np.abs(want).max()
    d = np.abs(got - want).max(axis=1) / (m if m > 0 else 1.0)
    bad = np.flatnonzero(~(d <= bound))
    assert bad.size == 0, (f"{what}: {bad.size} columns beyond {bound:.2e}, first column {bad[0]} with {lengths[bad[0]]} ratings: "
                           f"{got[bad[0]]!r} instead of {want[bad[0]]!r} ({d[bad[0]]:.2e})")


def assert_run_within(U, V, recs, lines, ref, bounds, R, maxiter, tag, rmse):
    """Factors, the counts, obj per outer iteration and the printed per-rank lines (loss, obj, diff, reg, and with `rmse` the test rmse:
    in both precisions, the test residuals being fp64 on the device and in the emulated reference alike) against a reference run,
    inside `bounds`."""
    bU, bV, bs = bounds
    dU, dV = dist(U, ref.W), dist(V, ref.H)
    last = [[r for r in ref.recs if r[0] == oi][-1] for oi in range(1, maxiter + 1)]
    dobj = max(abs(recs[oi]["obj"] - last[oi - 1][3]) / abs(last[oi - 1][3]) for oi in range(1, maxiter + 1))
    print(f"{tag}: U {dU:.2e} / bound {bU:.2e}, V {dV:.2e} / bound {bV:.2e}, obj {dobj:.2e} / bound {bs:.2e}")
    assert [recs[oi]["cg_v"] for oi in range(1, maxiter + 1)] == [r[7] for r in last]
    assert [recs[oi]["cg_u"] for oi in range(1, maxiter + 1)] == [sum(1 for r in ref.recs if r[0] <= oi) for oi in range(1, maxiter + 1)]
    assert_within(V, ref.H, bV, np.bincount(R.item, minlength=R.d2), tag + " V")
    assert_within(U, ref.W, bU, np.bincount(R.user, minlength=R.d1), tag + " U")
    assert dobj <= bs
    printed = parse_lines([re.sub(r"^(iter \d+ rank \d+ )", r"\1time 0 ", ln) for ln in lines])
    assert_lines(printed, ref.recs, bs, rmse=rmse)


@pytest.mark.gpu
@pytest.mark.parametrize("f64", [True, False], ids=["f64", "f32"])
@pytest.mark.parametrize("row,weighted", PARITY, ids=[r + ("-w" if w else "") for r, w in PARITY])
@pytest.mark.parametrize("name", ["long", "wide"])
def test_parity_with_the_implicit_reference(name, row, weighted, f64):
    """Factors and the per-rank loss / obj / reg / rmse lines inside the CPU-computed bounds; the counts equal; empty users and
    items carry the reference's values; the residual copies agree (finish).

    In fp32 the device is expected to equal the emulated reference bit for bit (measured: it does, on every case): the rated cells
    leave the all-cells sums through an fp64 prediction kept per rating, not through the stored fp32 residual, whose rounding would
    show at one to twenty times these bounds."""
    s = istudy(name, row, weighted)
    ref, bounds = (s["ref64"], s["b64"]) if f64 else (s["ref32"], s["b32"])
    R = rset(name)
    U, V, recs, lines = finish(isolver(name, row, f64, weighted, verbose=1, do_predict=1))
    assert_run_within(U, V, recs, lines, ref, bounds, R, IROWS[row]["maxiter"], f"implicit {name}/{row}{'/w' if weighted else ''} {'f64' if f64 else 'f32'}", True)
    _, _, empty_users, empty_items, _ = data(name)                    # empty users and items carry the reference's values, bit for bit
    assert same_bits(U[empty_users], ref.W[empty_users]) and same_bits(V[empty_items], ref.H[empty_items])


@pytest.mark.gpu
@pytest.mark.parametrize("f64", [True, False], ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["long", "wide"])
def test_the_fundec_of_empty_columns_decides_where_ranks_stop(name, f64):
    """From the heavy start the update of the empty users (old -> 0, fundec h old^2) decides the stopping of outer iteration 1: an
    implementation that skipped empty columns would run other counts (the CPU defect test: 100 x outside these bounds)."""
    s = istudy(name, "default", heavy=True)
    ref, bounds = (s["ref64"], s["b64"]) if f64 else (s["ref32"], s["b32"])
    U, V, recs, lines = finish(isolver(name, "default", f64, heavy=True, verbose=1, do_predict=1))
    assert_run_within(U, V, recs, lines, ref, bounds, rset(name), 2, f"implicit {name}/heavy {'f64' if f64 else 'f32'}", True)


@pytest.mark.gpu
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weights"])
@pytest.mark.parametrize("row", ["default", "nmf"])
@pytest.mark.parametrize("name", ["long", "wide"])
def test_device_against_device_on_the_completed_set(name, row, weighted):
    """The implicit solver on the sparse set against the existing weighted solver on the completed set (the loader keeps ratings of
    0: asserted), both fp64 on the GPU, inside the completed reference's own bound (CPU test 1)."""
    import primalcr_amd as pcr
    R = rset(name)
    C, cw = completed(R, weights(name) if weighted else None, ALPHA)
    cds = pcr.Dataset.from_ratings(C)
    assert cds.dims()[2] == R.d1 * R.d2 and np.array_equal(cds.csr()[2], C.val)
    Ui, Vi, recsi, linesi = finish(isolver(name, row, True, weighted, verbose=1, do_predict=1))
    Uc, Vc, recsc, linesc = finish(make_solver(cds, R.d1, row, True, alpha=None, w=cw, verbose=1, do_predict=1))
    bU, bV, bs = completed_study(name, row, weighted)["bound"]
    dU, dV = dist(Ui, Uc), dist(Vi, Vc)
    a, b = parse_lines([re.sub(r"^(iter \d+ rank \d+ )", r"\1time 0 ", ln) for ln in linesi]), parse_lines([re.sub(r"^(iter \d+ rank \d+ )", r"\1time 0 ", ln) for ln in linesc])
    print(f"device / device {name}/{row}/{'w' if weighted else 'plain'}: U {dU:.2e} / {bU:.2e}, V {dV:.2e} / {bV:.2e}")
    assert dU <= bU and dV <= bV
    assert [(r["cg_v"], r["cg_u"]) for r in recsi[1:]] == [(r["cg_v"], r["cg_u"]) for r in recsc[1:]]
    assert max(abs(x["obj"] - y["obj"]) / abs(y["obj"]) for x, y in zip(recsi[1:], recsc[1:])) <= bs
    # the printed loss, obj, reg and rmse of every rank: both sides are rounded to their print resolution
    assert [q[:2] for q in a] == [q[:2] for q in b]
    for x, y in zip(a, b):
        for i, digits in ((3, 10), (4, 10), (7, 7), (8, 10)):
            assert abs(x[i] - y[i]) <= half_ulp10(x[i], digits) + half_ulp10(y[i], digits) + bs * abs(y[i]), (x, y, i)


@pytest.mark.gpu
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weights"])
def test_on_a_fully_rated_set_the_implicit_solver_is_the_explicit_one(weighted):
    """No unrated cell: every all-cells sum is taken back out in full.  Inside the fp64 bound of the explicit reference's spread."""
    F = data("full")
    w = weights("full") if weighted else None
    for row in ("default", "nmf", "k1"):
        rng = np.random.default_rng(105)
        ref = wref_run(F, row, np.ones(F.nnz) if w is None else w)
        others = [wref_run(F, row, np.ones(F.nnz) if w is None else w, perm=rng.permutation(F.nnz)) for _ in range(3)]
        others.append(wref_run(F, row, np.ones(F.nnz) if w is None else w, acc=np.longdouble))
        assert all(counts(o) == counts(ref) for o in others)
        bounds = spread(ref, others, 16)
        Ue, Ve, recse, _ = finish(make_solver(dataset("full"), F.d1, row, True, alpha=None, w=w))
        U, V, recs, lines = finish(make_solver(dataset("full"), F.d1, row, True, alpha=ALPHA, w=w, verbose=1, do_predict=1))
        assert_run_within(U, V, recs, lines, ref, bounds, F, 2, f"full/{row}", True)
        assert dist(U, Ue) <= bounds[0] and dist(V, Ve) <= bounds[1]
        assert [(r["cg_v"], r["cg_u"]) for r in recs[1:]] == [(r["cg_v"], r["cg_u"]) for r in recse[1:]]


@pytest.mark.gpu
@pytest.mark.parametrize("f64", [True, False], ids=["f64", "f32"])
@pytest.mark.parametrize("c", [2.0, 0.25])
def test_a_common_power_of_two_on_the_device(c, f64):
    """Factors bit-identical, obj scaled exactly, the same counts."""
    for name, row in (("long", "default"), ("wide", "nmf"), ("long", "k100")):
        U0, V0, recs0, _ = finish(isolver(name, row, f64, True))
        U1, V1, recs1, _ = finish(make_solver(dataset(name), rset(name).d1, row, f64, alpha=c * ALPHA, w=c * weights(name)))
        assert same_bits(U1, U0) and same_bits(V1, V0)
        assert figures(recs1) == [(c * o, a, b) for o, a, b in figures(recs0)]


@pytest.mark.gpu
@pytest.mark.parametrize("f64", [True, False], ids=["f64", "f32"])
def test_switching_back_and_the_profiler_slots(f64):
    """set_implicit(0) after an implicit run gives the run of a solver that never saw the call, bit for bit; the .i slots and
    ccd/gramcol are non-empty in implicit runs only; the setting survives set_factors, set_ccd_params and set_rating_weights."""
    import primalcr_amd as pcr
    R = rset("long")
    U0 = start("long", 3)
    islots = ("ccd/gramcol", "ccd/vsweep.i", "ccd/usweep.i", "ccd/resid.i", "ccd/final.i", "ccd/init.i")
    for weighted in (False, True):
        w = weights("long") if weighted else None
        never = make_solver(dataset("long"), R.d1, "default", f64, alpha=None, w=w, profile=True)
        Ue, Ve, recse, _ = finish(never, close=False)
        prof = never.profile_all()
        never.close()
        assert all(prof.get(x, (0, 0))[1] == 0 for x in islots), prof
        s = isolver("long", "default", f64, weighted, profile=True)
        assert s.counter("ccd_implicit") == (ALPHA if f64 else float(np.float32(ALPHA)))
        Ui, Vi, recsi, _ = finish(s, close=False)
        prof = s.profile_all()
        assert all(prof.get(x, (0, 0))[1] > 0 for x in islots), prof
        assert all(prof.get(x + sfx, (0, 0))[1] == 0 for x in ("ccd/vsweep", "ccd/usweep", "ccd/resid", "ccd/init") for sfx in ("", ".w")), prof
        assert not same_bits(Ui, Ue)
        s.set_implicit(0)
        assert s.counter("ccd_implicit") == 0
        s.set_factors(U0, None)
        U, V, recs, _ = finish(s, close=False)
        assert same_bits(U, Ue) and same_bits(V, Ve) and figures(recs) == figures(recse)
        # on again; survives set_factors, set_ccd_params and a change of the rating weights (W is rebuilt)
        s.set_implicit(ALPHA)
        s.set_factors(U0, None)
        s.set_ccd_params(maxinneriter=3, eps=1e-3, do_nmf=0)
        U, V, recs, _ = finish(s, close=False)
        assert same_bits(U, Ui) and same_bits(V, Vi) and figures(recs) == figures(recsi)
        s.set_rating_weights(None if weighted else weights("long"))
        assert s.counter("ccd_implicit") > 0
        s.set_factors(U0, None)
        Uo, Vo, recso, _ = finish(s, close=False)
        Uf, Vf, recsf, _ = finish(isolver("long", "default", f64, not weighted))
        assert same_bits(Uo, Uf) and same_bits(Vo, Vf) and figures(recso) == figures(recsf)
        for bad in (-1.0, math.nan, math.inf, -math.inf) + (() if f64 else (1e-60, 1e60)):     # (fp32: 0 or infinite as stored)
            before = s.counter("ccd_implicit")
            with pytest.raises(pcr.PcrError, match="error -1: .*alpha"):
                s.set_implicit(bad)
            assert s.counter("ccd_implicit") == before
        s.close()


@pytest.mark.gpu
def test_training_again_and_iterate():
    """Two train() calls from the same U are bit-identical; train() then iterate(2) is a three-iteration train()."""
    U0 = start("wide", 3)
    s = isolver("wide", "default", True, True)
    U1, V1, recs1, _ = finish(s, close=False)
    s.set_factors(U0, None)
    U2, V2, recs2, _ = finish(s)
    assert same_bits(U1, U2) and same_bits(V1, V2) and figures(recs1) == figures(recs2)
    U3, V3, recs3, _ = finish(isolver("wide", "default", True, True, maxiter=3))
    s = isolver("wide", "default", True, True, maxiter=1)
    r1, _ = s.train()
    it = s.iterate(2)
    assert s.counter("ccd_residual_mismatch") == 0
    U, V = s.get_factors()
    s.close()
    assert same_bits(U, U3) and same_bits(V, V3)
    assert [(r1[1]["obj"], r1[1]["cg_v"])] + [(r["obj"], r["cg_v"]) for r in it] == [(r["obj"], r["cg_v"]) for r in recs3[1:]]


@pytest.mark.gpu
def test_a_ranking_solver_refuses_implicit_feedback_with_the_reason():
    import primalcr_amd as pcr
    ds = pcr.Dataset.from_ratings(ratings("synth3"))
    s = pcr.Solver(ds, pcr.Parameter(solver_type=pcr.PCR_SOLVER_PCRPP, k=4))
    with pytest.raises(pcr.PcrError, match="error -7: .*CCDR1"):
        s.set_implicit(0.5)
    with pytest.raises(pcr.PcrError, match="error -6: .*ccd_implicit"):
        s.counter("ccd_implicit")
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("f64", [True, False], ids=["f64", "f32"])
def test_cli_implicit_prints_the_lines_of_the_binding(f64, tmp_path):
    import primalcr_amd as pcr
    R = ratings("synth3")
    d = synth.write_dir(R, str(tmp_path / "data"))
    common = ["-s", "0", "-k", "4", "-l", "0.05", "-t", "2", "-T", "3", "--implicit", "0.3"] + (["--f64"] if f64 else [])
    ds = pcr.Dataset.from_ratings(R)
    for extra, w in (([], None), (["--popularity-weights", "0.5"], pcr.rating_weights_popularity(ds, 0.5))):
        model = tmp_path / "cli.model"
        r = run([TRAIN] + common + extra + [d, str(model)], tmp_path)
        assert r.returncode == 0, r.stderr
        out = r.stdout.rstrip("\n").split("\n")
        assert out[0] == "starts!" and out[-1].startswith("Wall-time: ")
        p = pcr.Parameter(solver_type=pcr.PCR_SOLVER_CCDR1, k=4, precision=pcr.PCR_F64 if f64 else pcr.PCR_F32, maxiter=2, do_predict=1, verbose=1,
                          **{"lambda": 0.05})
        s = pcr.Solver(ds, p)
        s.set_ccd_params(maxinneriter=3, eps=1e-3, do_nmf=0)
        s.set_factors(pcr.initial_col(R.d1, 4), None)
        if w is not None:
            s.set_rating_weights(w)
        s.set_implicit(0.3)
        U, V, _, lines = finish(s)
        assert [re.sub(r"time \S+ ", "", ln) for ln in out[1:-1]] == lines and len(lines) == 4 * 2
        mine = tmp_path / "binding.model"
        pcr.model_save(str(mine), U, V)
        assert model.read_bytes() == mine.read_bytes()
    r = run([TRAIN] + [x for x in common if x not in ("--implicit", "0.3")] + [d, str(tmp_path / "plain.model")], tmp_path)
    assert r.returncode == 0 and (tmp_path / "plain.model").read_bytes() != (tmp_path / "cli.model").read_bytes()
