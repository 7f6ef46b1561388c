"""Per-user loss weights in PrimalCR / PrimalCR++ training (pcr_solver_set_user_weights):

    min  sum_u c_u L_u(U, V) + lambda/2 (|U|^2 + |V|^2)

Part 1 (CPU) holds the host entries (user_pairs, user_weights), the definitional numpy reference of tests/user_weight_ref.py
(against the oracle at c = 1 and against the oracle on the data set in which user u appears c_u times) and the precondition
of the exact GPU cells, and checks the CLI's argument handling.  Part 2 (GPU) holds the kernels: all-ones weights change no
bit; on dyadic inputs objective / obtain_g / compute_Ha equal the reference exactly under the launch variants; user u's Newton
step is the unweighted step at lambda / c_u bit for bit; a uniform weight is a rescaled lambda over the whole trajectory;
general weights meet the tolerances the unweighted entries meet against the oracle; shards add up; weights may be set mid-run;
what is unsupported is refused.

Exact cells: weights are dealt from {1/2, 1, 2} round-robin inside every user-length class.  Every (solver, rank) cell fits
fp32's 24 bits with these weights (test_exact_cells_fit_fp32 computes, in int64, the largest stored sweep coefficient and, for
every (item, column), the sum of the ABSOLUTE values of all terms of g and Ha -- a bound on every partial sum in any order);
a cell that did not would fall back to {1, 2} (exact_values), and none does."""
import os
import struct
import subprocess

import numpy as np
import pytest

import exact_data as ed
import primalcr_amd as pcr
import user_weight_ref as uw
from conftest import BIN_DIR, load_golden
from primalcr_amd import synth
from test_gpu_parity import TOL, rel

TRAIN = os.path.join(BIN_DIR, "omp-pmf-train")
PREC = {"F64": pcr.PCR_F64, "F32": pcr.PCR_F32}
RANKS = (1, 7, 100)
CELLS = [(p, s, r) for p in ("F64", "F32") for s in (2, 1) for r in RANKS]
CELL_IDS = [f"{p}-s{s}-r{r}" for p, s, r in CELLS]
# the launch variants of test_gpu_parity.VARIANTS the exact cells run under
EXACT_VARIANTS = [{}, {"window_cache": "0"}, {"prepare_merged": "0"}, {"ustep_mode": "1"}, {"ustep_mode": "2"}, {"cluster_k": "1"},
                  {"lanes": "1"}, {"sddmm_csc": "1"}]
BUDGET = 2 ** 24                         # fp32's exact integers, in the unit of the quantity (exact_data.py)


def vid(v):
    return ",".join(f"{k}={v[k]}" for k in v) if v else "default"


def run(cmd, cwd):
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=300)


_CASE = {}


def case(r, solver, real=False):
    """The dyadic case with its CSR, data set and the reference's per-user terms (computed once per module and never changed)."""
    key = (r, solver, real)
    if key not in _CASE:
        c = ed.dyadic_case(r, solver, real=real)
        o = np.lexsort((c.item, c.user))
        c.idx = np.concatenate([[0], np.cumsum(np.bincount(c.user, minlength=c.d1))]).astype(np.int64)
        c.citem, c.cval = c.item[o].astype(np.int64), c.val[o]
        c.lens = np.diff(c.idx)
        c.terms = uw.user_terms(c.U, c.V, c.idx, c.citem, c.cval, solver, c.a)
        c.ds = pcr.Dataset.from_triplets(c.d1, c.d2, c.user, c.item, c.val)
        c.budget = {}
        _CASE[key] = c
    return _CASE[key]


def budget(c, values):
    if values not in c.budget:
        w, _ = uw.class_weights(c.lens, values)
        c.budget[values] = uw.integer_budget(c, c.idx, c.citem, c.cval, w, c.a)
    return c.budget[values]


def fits_fp32(b):
    return all(b[k]["coef"] < BUDGET and b[k]["abssum"] < BUDGET for k in ("g", "Ha"))


def exact_values(c, pname):
    """{1/2, 1, 2}; an fp32 cell whose partial sums would leave the 24-bit budget with them takes {1, 2}."""
    if pname == "F64" or fits_fp32(budget(c, (0.5, 1.0, 2.0))):
        return (0.5, 1.0, 2.0)
    return (1.0, 2.0)


def make(c, pname, lam=None, variant=None, ds=None):
    with pcr.tuned(**(variant or {})):
        return pcr.Solver(ds or c.ds, pcr.Parameter(k=c.r, solver_type=c.solver, precision=PREC[pname], **{"lambda": c.lam if lam is None else lam}))


# ------------------------------------------------------------------------------------------------------------------------------
# 1. CPU: host entries, the reference, the preconditions, the CLI's arguments
# ------------------------------------------------------------------------------------------------------------------------------

def _small_real_set():
    """40 users over 60 items, ratings off the integers: user 0 has no rating, user 1 one, user 2 seven ratings of ONE value,
    user 3 six different values inside one lround bucket (PrimalCR++: one level, PrimalCR: fifteen pairs)."""
    rng = np.random.default_rng(5)
    lens = np.concatenate([[0, 1, 7, 6], rng.integers(2, 40, 36)])
    user = np.repeat(np.arange(40), lens)
    item = np.concatenate([rng.choice(60, n, replace=False) for n in lens])
    val = rng.integers(1, 6, user.shape[0]) + rng.uniform(-0.49, 0.49, user.shape[0])
    val[user == 2] = 3.25
    val[user == 3] = 4.0 + np.linspace(-0.4, 0.4, 6)
    return 40, 60, user, item, val


def _all_pairs(d1, user, val, solver):
    lev = ed.levels_of(val, solver)
    return np.array([int((lev[user == u][:, None] > lev[user == u][None, :]).sum()) for u in range(d1)], np.int64)


def test_user_pairs_equal_an_all_pairs_count():
    d1, d2, user, item, val = _small_real_set()
    ds = pcr.Dataset.from_triplets(d1, d2, user, item, val)
    got = {}
    for solver in (pcr.PCR_SOLVER_PCR, pcr.PCR_SOLVER_PCRPP):
        got[solver] = ds.user_pairs(solver)
        assert got[solver].dtype == np.int64 and np.array_equal(got[solver], _all_pairs(d1, user, val, solver))
        assert int(got[solver].sum()) == ds.count_pairs(solver)
        assert got[solver][0] == got[solver][1] == got[solver][2] == 0
    assert got[pcr.PCR_SOLVER_PCRPP][3] == 0 and got[pcr.PCR_SOLVER_PCR][3] == 15
    assert not np.array_equal(got[pcr.PCR_SOLVER_PCR], got[pcr.PCR_SOLVER_PCRPP])
    with pytest.raises(pcr.PcrError, match="error -1"):
        ds.user_pairs(0)


def test_user_weights_schemes():
    d1, d2, user, item, val = _small_real_set()
    ds = pcr.Dataset.from_triplets(d1, d2, user, item, val)
    n = np.bincount(user, minlength=d1)
    for solver in (pcr.PCR_SOLVER_PCR, pcr.PCR_SOLVER_PCRPP):
        P = ds.user_pairs(solver)
        assert np.array_equal(pcr.user_weights(ds, pcr.PCR_WEIGHT_UNIFORM, solver), np.ones(d1))
        wp = pcr.user_weights(ds, pcr.PCR_WEIGHT_PAIRS, solver)
        want = np.where(P > 0, (P.sum() / (P > 0).sum()) / np.maximum(P, 1), 1.0)
        assert np.array_equal(wp, want) and np.all(wp[P == 0] == 1.0)
        assert abs(float((wp * P).sum()) / P.sum() - 1) < 1e-12
        wr = pcr.user_weights(ds, pcr.PCR_WEIGHT_RATINGS, solver)
        want = np.where(n > 0, (n.sum() / (n > 0).sum()) / np.maximum(n, 1), 1.0)
        assert np.array_equal(wr, want) and wr[0] == 1.0
        assert abs(float((wr * n).sum()) / n.sum() - 1) < 1e-12
    for bad in (-1, 3, 17):
        with pytest.raises(pcr.PcrError, match="error -1"):
            pcr.user_weights(ds, bad)
    with pytest.raises(pcr.PcrError, match="error -1"):
        pcr.user_weights(ds, pcr.PCR_WEIGHT_PAIRS, 0)


REF_CASES = [(7, 2, False), (7, 1, False), (1, 2, False), (7, 1, True), (100, 2, True)]


@pytest.mark.parametrize("r,solver,real", REF_CASES, ids=[f"r{r}-s{s}-{'real' if x else 'int'}" for r, s, x in REF_CASES])
def test_reference_with_unit_weights_is_the_oracle(oracle, r, solver, real):
    """The reference is itself held to something: with c = 1 it equals the oracle's objective / obtain_g / compute_Ha on the
    dyadic case, exactly (every number involved is a small dyadic rational)."""
    c = case(r, solver, real)
    X = oracle.build_csr(c.d1, c.d2, c.user, c.item, c.val)
    assert np.array_equal(X.idx, c.idx) and np.array_equal(X.item, c.citem) and np.array_equal(X.val, c.cval)
    m = oracle.comp_m(c.U, c.V, X)
    obj, g, Ha, _, _, _ = uw.combine(c.terms, np.ones(c.d1), c.lam)
    assert np.array_equal(c.terms.m, m)
    assert obj == oracle.objective_new(m, c.U, c.V, X, c.lam, solver=solver)
    assert np.array_equal(g, oracle.obtain_g_new(c.U, c.V, X, m, c.lam, solver=solver))
    assert np.array_equal(Ha, oracle.compute_Ha_new(c.a, m, c.U, X, c.lam, solver=solver))
    assert int(c.terms.pairs.sum()) == c.ds.count_pairs(solver) and np.array_equal(c.terms.pairs, c.ds.user_pairs(solver))


@pytest.mark.parametrize("solver", [2, 1])
def test_integer_weights_are_duplicated_users(oracle, solver):
    """With weights in {1, 2, 3} the weighted loss and the item side's gradient / Hessian-vector product WITHOUT their lambda
    terms are those of the data set in which user u appears c_u times with the same row of U -- computed by the oracle, which
    knows nothing of weights.  Exact on the dyadic case.  A mutant reference that ignores one user's weight lands outside."""
    c = case(7, solver)
    w = np.asarray(uw.class_weights(c.lens, (1.0, 2.0, 3.0))[0])
    rep = np.repeat(np.arange(c.d1), w.astype(np.int64))                       # new user -> old user
    new_of = np.concatenate([[0], np.cumsum(w.astype(np.int64))])
    du, di, dv = [], [], []
    for copy in range(3):
        keep = w[c.user] > copy
        du.append(new_of[c.user[keep]] + copy); di.append(c.item[keep]); dv.append(c.val[keep])
    du, di, dv = np.concatenate(du), np.concatenate(di), np.concatenate(dv)
    Ud = c.U[rep]
    X = oracle.build_csr(len(rep), c.d2, du, di, dv)
    m = oracle.comp_m(Ud, c.V, X)
    loss_d = oracle.objective_new(m, Ud, c.V, X, c.lam, solver=solver) - c.lam / 2.0 * float((Ud ** 2).sum() + (c.V ** 2).sum())
    g_d = oracle.obtain_g_new(Ud, c.V, X, m, c.lam, solver=solver) - c.lam * c.V
    Ha_d = oracle.compute_Ha_new(c.a, m, Ud, X, c.lam, solver=solver) - c.lam * c.a
    _, _, _, loss, g0, h0 = uw.combine(c.terms, w, c.lam)
    assert loss == loss_d and np.array_equal(g0, g_d) and np.array_equal(h0, Ha_d)
    victim = int(np.flatnonzero((w == 3.0) & (c.terms.loss > 0) & (c.lens > 100))[0])
    _, _, _, loss_m, g_m, h_m = uw.combine(c.terms, w, c.lam, ignore_user=victim)
    assert loss_m != loss_d and not np.array_equal(g_m, g_d) and not np.array_equal(h_m, Ha_d)


@pytest.mark.parametrize("solver,r", [(s, r) for s in (2, 1) for r in RANKS], ids=[f"s{s}-r{r}" for s in (2, 1) for r in RANKS])
def test_exact_cells_fit_fp32(solver, r):
    """The precondition of the exact GPU cells, in int64 (user_weight_ref.integer_budget, as
    test_dyadic_preconditions_and_integer_brute_force does for the unweighted case): with the weights the fp32 cell uses, the
    sweep coefficient stored per rating (quarter units) and the sum of the absolute values of all terms of every entry of g and
    Ha (eighth units: a bound on every partial sum, in any order and any split) stay below 2^24; the objective is a whole
    number of 1/32 far inside fp64; the integer results are the float reference's; every length class that has three users
    holds every weight value."""
    c = case(r, solver)
    values = exact_values(c, "F32")
    b = budget(c, values)
    print(f"[user-weights] s{solver} r={r}: weights {values}; max stored coefficient {b['g']['coef']} / {b['Ha']['coef']} quarter units, "
          f"max sum of |terms| {b['g']['abssum']} / {b['Ha']['abssum']} eighth units (budget {BUDGET})")
    assert fits_fp32(b), (values, {k: (b[k]["coef"], b[k]["abssum"]) for k in ("g", "Ha")})
    assert values == (0.5, 1.0, 2.0)             # no cell needs the fall-back; the module docstring says so
    assert b["obj32"] < 2 ** 50
    w, cls = uw.class_weights(c.lens, values)
    assert set(ed.CLASS_EDGES) <= set(c.lens.tolist())
    for k in np.unique(cls):
        if (cls == k).sum() >= len(values):
            assert set(w[cls == k]) == set(values), k
    obj, g, Ha, _, _, _ = uw.combine(c.terms, w, c.lam)
    assert obj * 32 == b["obj32"] and np.array_equal(g * 8, b["g"]["val8"]) and np.array_equal(Ha * 8, b["Ha"]["val8"])
    for x in (g, Ha):
        assert np.array_equal(x, x.astype(np.float32).astype(np.float64))


def test_cli_arguments(tmp_path):
    """Usage text, the mutual exclusion, the refusal with -s 0 and the weights file's checks: all before any GPU work."""
    R = synth.generate("tiny")
    d = synth.write_dir(R, str(tmp_path / "data"))
    r = run([TRAIN], tmp_path)
    assert r.returncode == 1 and "--user-weights file" in r.stdout and "--normalize pairs|ratings" in r.stdout
    good = tmp_path / "w.txt"
    good.write_text("".join("1.5\n" for _ in range(R.d1)))
    r = run([TRAIN, "--user-weights", str(good), "--normalize", "pairs", d, "m.model"], tmp_path)
    assert r.returncode == 1 and "mutually exclusive" in r.stderr
    r = run([TRAIN, "--normalize", "stars", d, "m.model"], tmp_path)
    assert r.returncode == 1 and "pairs or ratings" in r.stderr
    for opt in (["--user-weights", str(good)], ["--normalize", "pairs"]):
        r = run([TRAIN, "-s", "0"] + opt + [d, "m.model"], tmp_path)
        assert r.returncode == 1 and opt[0] + " is not supported with -s 0" in r.stderr
    short = tmp_path / "short.txt"
    short.write_text("".join("1\n" for _ in range(R.d1 - 1)))
    r = run([TRAIN, "--user-weights", str(short), d, "m.model"], tmp_path)
    assert r.returncode == 1 and f"holds {R.d1 - 1} weights, meta has {R.d1} users" in r.stderr
    long = tmp_path / "long.txt"
    long.write_text("".join("1\n" for _ in range(R.d1 + 1)))
    r = run([TRAIN, "--user-weights", str(long), d, "m.model"], tmp_path)
    assert r.returncode == 1 and "more than" in r.stderr
    for bad, what in (("0", "not a finite number > 0"), ("-2.5", "not a finite number > 0"), ("inf", "not a finite number > 0"),
                      ("nan", "not a finite number > 0"), ("heavy", "is not a number"), ("1.5x", "is not a number")):
        f = tmp_path / "bad.txt"
        f.write_text("".join("1\n" for _ in range(R.d1 - 1)) + bad + "\n")
        r = run([TRAIN, "--user-weights", str(f), d, "m.model"], tmp_path)
        assert r.returncode == 1 and what in r.stderr and f"bad.txt:{R.d1}" in r.stderr, (bad, r.stderr)
    r = run([TRAIN, "--user-weights", str(tmp_path / "missing.txt"), d, "m.model"], tmp_path)
    assert r.returncode == 1 and "can't open" in r.stderr


# ------------------------------------------------------------------------------------------------------------------------------
# 2. GPU
# ------------------------------------------------------------------------------------------------------------------------------

def first_order(s, c):
    s.comp_m(want=False)
    return s.objective(), s.obtain_g(), s.compute_Ha(c.a)


def two_steps(s):
    recs = s.iterate(2)
    U, V = s.get_factors()
    return U.tobytes(), V.tobytes(), [(x["obj"], x["cg_v"], x["ls_v"], x["cg_u"], x["ls_u"]) for x in recs]


@pytest.mark.gpu
@pytest.mark.parametrize("pname,solver,r", CELLS, ids=CELL_IDS)
def test_all_ones_change_nothing(pname, solver, r):
    """set_user_weights(ones) takes the weighted kernels and must leave every bit where the unweighted solver puts it: objective,
    obtain_g, compute_Ha, two iterate steps (U, V, objectives, counts).  set_user_weights(None) after non-trivial weights is
    the unweighted solver again."""
    c = case(r, solver)
    plain = make(c, pname)
    ones = make(c, pname)
    back = make(c, pname)
    try:
        for s in (plain, ones, back):
            s.set_factors(c.U, c.V)
        ones.set_user_weights(np.ones(c.d1))
        back.set_user_weights(uw.class_weights(c.lens, (0.5, 3.0, 7.0))[0])
        ref = first_order(plain, c)
        other = first_order(back, c)
        assert other[0] != ref[0] and not np.array_equal(other[1], ref[1])             # the weights were live
        back.set_user_weights(None)
        for s, tag in ((ones, "all ones"), (back, "None after weights")):
            got = first_order(s, c)
            assert got[0] == ref[0], (tag, got[0], ref[0])
            assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]), tag
        want = two_steps(plain)
        for s, tag in ((ones, "all ones"), (back, "None after weights")):
            assert two_steps(s) == want, tag
    finally:
        for s in (plain, ones, back):
            s.close()


EXACT = [(p, s, r, v) for (p, s, r) in CELLS for v in EXACT_VARIANTS]


@pytest.mark.gpu
@pytest.mark.parametrize("pname,solver,r,variant", EXACT, ids=[f"{p}-s{s}-r{r}-{vid(v)}" for p, s, r, v in EXACT])
def test_weighted_first_order_entries_are_exact(pname, solver, r, variant):
    """Weights in {1/2, 1, 2}, every length class holding every value: objective, obtain_g and compute_Ha == the reference, under
    the launch variants (the same again after the probe: the state survives)."""
    c = case(r, solver)
    w, _ = uw.class_weights(c.lens, exact_values(c, pname))
    obj, g, Ha, _, _, _ = uw.combine(c.terms, w, c.lam)
    s = make(c, pname, variant=variant)
    try:
        s.set_factors(c.U, c.V)
        s.set_user_weights(w)
        for _ in range(2):
            o, gg, hh = first_order(s, c)
            assert o == obj, (o, obj, (o - obj) * 32)
            for name, got, want in (("g", gg, g), ("Ha", hh, Ha)):
                bad = np.flatnonzero(got.ravel() != want.ravel())
                assert bad.size == 0, f"{name}: {bad.size} of {got.size} entries differ; first at item {bad[0] // c.r}, column {bad[0] % c.r}: " \
                                      f"{got.ravel()[bad[0]]!r} against {want.ravel()[bad[0]]!r}"
    finally:
        s.close()


USTEP_CELLS = [("F64", 2, 7), ("F32", 2, 7), ("F64", 1, 7), ("F32", 2, 100), ("F64", 2, 100)]


@pytest.mark.gpu
@pytest.mark.parametrize("pname,solver,r", USTEP_CELLS, ids=[f"{p}-s{s}-r{r}" for p, s, r in USTEP_CELLS])
def test_u_step_is_the_unweighted_step_at_lambda_over_c(pname, solver, r):
    """V fixed, one update_U under weights from {1/2, 1, 2, 3} (lambda / 3 is not dyadic: the identity still holds bitwise, both
    sides are handed the same double).  For every value w the rows of the users carrying w are, byte for byte, the rows of an
    UNWEIGHTED solver created with lambda / w.
    Counts and objective: the per-user counts are not observable, so every value's cohort runs alone -- an unweighted solver at
    lambda / w on the data set in which every OTHER user is inert: its ratings keep their items (the rating counts, hence the
    length classes and every user's workgroup form, stay those of the full set) but all take one value, and its row of U is
    zero -- no comparable pair, a zero gradient, the skip test of pcrpp.cpp:787-790 holds: no CG iteration, no line-search
    evaluation, nothing added to the objective.  The weighted run's CG and line-search totals are the sums of the cohorts',
    and its now_obj is sum_u c_u obj_u + lambda/2 |V|^2."""
    c = case(r, solver)
    values = (0.5, 1.0, 2.0, 3.0)
    w, _ = uw.class_weights(c.lens, values)

    def ustep(s, weights=None, U=None):
        s.set_factors(c.U if U is None else U, c.V)
        if weights is not None:
            s.set_user_weights(weights)
        s.comp_m(want=False)
        obj, info = s.update_U()
        Un, _ = s.get_factors()
        s.close()
        return Un, obj, info

    Uw, objw, infow = ustep(make(c, pname), w)
    for v in values:
        Uv, _, _ = ustep(make(c, pname, lam=c.lam / v))
        who = np.flatnonzero(w == v)
        assert who.size > 100
        bad = [int(u) for u in who if Uw[u].tobytes() != Uv[u].tobytes()]
        assert not bad, f"weight {v}: {len(bad)} of {who.size} rows differ from the unweighted step at lambda / {v}; first user {bad[0]}, " \
                        f"{ed.class_of(int(c.lens[bad[0]]))}: {Uw[bad[0]][:4]} against {Uv[bad[0]][:4]}"
    v2 = c.lam / 2.0 * float((c.V ** 2).sum())
    cg = ls = 0
    total = 0.0
    for v in values:
        ds = pcr.Dataset.from_triplets(c.d1, c.d2, c.user, c.item, np.where(w[c.user] == v, c.val, 3.0))
        Uc, obj, info = ustep(make(c, pname, lam=c.lam / v, ds=ds), U=c.U * (w == v)[:, None])
        who = np.flatnonzero(w == v)
        assert Uc[who].tobytes() == Uw[who].tobytes() and not Uc[w != v].any(), v
        cg += info["cg"]; ls += info["ls"]
        total += v * (obj - v2 / v)
    assert (infow["cg"], infow["ls"]) == (cg, ls) and cg > 0 and ls > 0
    assert abs(objw / (total + v2) - 1) < TOL[PREC[pname]]["obj"], (objw, total + v2)


@pytest.mark.gpu
@pytest.mark.parametrize("pname,solver,r", USTEP_CELLS, ids=[f"{p}-s{s}-r{r}" for p, s, r in USTEP_CELLS])
def test_uniform_weight_is_a_rescaled_lambda(pname, solver, r):
    """Weights = 4 with lambda = 128 against no weights with lambda = 32 over two full iterations: U and V bit-identical, every
    pcr_iter_stats.obj exactly 4 x, the counts equal -- through the V step's CG stop, its line search and the pipelined hand-off
    with weights present (every quantity of the weighted run is the unweighted one times a power of two)."""
    c = case(r, solver)
    a = make(c, pname, lam=32.0)
    b = make(c, pname, lam=128.0)
    try:
        for s in (a, b):
            s.set_factors(c.U, c.V)
        b.set_user_weights(np.full(c.d1, 4.0))
        Ua, Va, ra = two_steps(a)
        Ub, Vb, rb = two_steps(b)
        assert Ua == Ub and Va == Vb
        assert [x[1:] for x in ra] == [x[1:] for x in rb]
        assert [4.0 * x[0] for x in ra] == [x[0] for x in rb], (ra, rb)
    finally:
        a.close(); b.close()


GENERAL = [("F64", 2, 7), ("F32", 2, 7), ("F64", 1, 7), ("F32", 1, 7), ("F64", 2, 100), ("F32", 2, 100)]


@pytest.mark.gpu
@pytest.mark.parametrize("pname,solver,r", GENERAL, ids=[f"{p}-s{s}-r{r}" for p, s, r in GENERAL])
def test_general_weights_against_the_reference(pname, solver, r):
    """Weights log-uniform in [0.1, 10] on the real-valued case: objective, g and Ha against the numpy reference at the tolerances
    the unweighted entries meet against the oracle (weighting adds one multiplication and no summation); three iterations give
    a non-increasing objective."""
    c = case(r, solver, real=True)
    t = TOL[PREC[pname]]
    w = np.exp(np.random.default_rng(r + solver).uniform(np.log(0.1), np.log(10.0), c.d1))
    obj, g, Ha, _, _, _ = uw.combine(c.terms, w, c.lam)
    s = make(c, pname)
    try:
        s.set_factors(c.U, c.V)
        s.set_user_weights(w)
        o, gg, hh = first_order(s, c)
        print(f"[user-weights] general {pname} s{solver} r={r}: obj rel {abs(o / obj - 1):.2e}, g rel {rel(gg, g):.2e}, Ha rel {rel(hh, Ha):.2e}")
        assert abs(o / obj - 1) < t["obj"]
        assert rel(gg, g) < t["vec"] and rel(hh, Ha) < t["vec"]
        objs = [o] + [x["obj"] for x in s.iterate(3)]
        assert all(b <= a for a, b in zip(objs, objs[1:])), objs
    finally:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pname", ["F64", "F32"])
@pytest.mark.parametrize("solver", [2, 1])
def test_pairs_weights_keep_the_total_mass(pname, solver):
    """At U = V = 0 every comparable pair costs 1, so the objective under PCR_WEIGHT_PAIRS is sum_u w_u |Omega_u| = |Omega|."""
    c = case(7, solver, real=True)
    w = pcr.user_weights(c.ds, pcr.PCR_WEIGHT_PAIRS, solver)
    P = c.ds.user_pairs(solver)
    s = make(c, pname)
    try:
        s.set_factors(np.zeros_like(c.U), np.zeros_like(c.V))
        s.set_user_weights(w)
        s.comp_m(want=False)
        o = s.objective()
        assert abs(o / float((w * P).sum()) - 1) < 1e-12 and abs(o / float(P.sum()) - 1) < 1e-12
    finally:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pname", ["F64", "F32"])
@pytest.mark.parametrize("nranks", [2, 3])
def test_weighted_shards_add_up_exactly(pname, nranks):
    """Local-only shards of the weighted dyadic case, every rank reading its own range of the job's weight vector (rank 0 of the
    3-rank job through set_user_weights_local): the partial g and Ha, summed on the host, and the objective with the replicated
    lambda/2 |V|^2 counted once equal the one-rank result and the reference exactly."""
    for solver, r in ((2, 7), (1, 7), (2, 100)):
        c = case(r, solver)
        w, _ = uw.class_weights(c.lens, exact_values(c, pname))
        obj, g, Ha, _, _, _ = uw.combine(c.terms, w, c.lam)
        par = dict(k=r, solver_type=solver, precision=PREC[pname], **{"lambda": c.lam})
        g_sum, Ha_sum, obj_sum = 0.0, 0.0, 0.0
        for q in range(nranks):
            s = pcr.Solver(c.ds, pcr.Parameter(**par), rank=q, nranks=nranks)
            s.set_local_only(True)
            s.set_factors(c.U, c.V)
            if q == 0 and nranks == 3:
                s.set_user_weights(w[s.first_user:s.first_user + s.n_users], local=True)
            else:
                s.set_user_weights(w)
            o, gg, hh = first_order(s, c)
            obj_sum += o; g_sum = g_sum + gg; Ha_sum = Ha_sum + hh
            s.close()
        obj_sum -= (nranks - 1) * c.lam / 2.0 * float((c.V ** 2).sum())
        full = make(c, pname)
        full.set_factors(c.U, c.V)
        full.set_user_weights(w)
        of, gf, hf = first_order(full, c)
        full.close()
        assert obj_sum == of == obj, (solver, r, obj_sum, of, obj)
        assert np.array_equal(g_sum, gf) and np.array_equal(gf, g), (solver, r)
        assert np.array_equal(Ha_sum, hf) and np.array_equal(hf, Ha), (solver, r)


def _golden_dir(name, tmp_path):
    g, meta = load_golden(name)
    R = synth.Ratings(int(g["d1"]), int(g["d2"]), g["user"], g["item"], g["val"], g["tuser"], g["titem"], g["tval"])
    return g, synth.write_dir(R, str(tmp_path / "data")), R


def _write_weights(path, w):
    with open(path, "w") as f:
        f.write("".join(repr(float(x)) + "\n" for x in w))


@pytest.mark.gpu
def test_cli_two_ranks_with_weights_equal_one_rank(tmp_path):
    """omp-pmf-train --gpus 2 --comm p2p --user-weights f on one device: every worker reads its own range of the file's weights
    and the job writes the model of the one-rank run, to the tolerance of test_gpus_option_two_ranks_on_one_gpu_equal_one_rank;
    and the weights matter: the unweighted model is another one."""
    g, d, R = _golden_dir("mid5", tmp_path)
    w = np.exp(np.random.default_rng(8).uniform(np.log(0.2), np.log(5.0), R.d1))
    _write_weights(tmp_path / "w.txt", w)
    base = [TRAIN, "-k", str(int(g["r"])), "-l", repr(float(g["lam"])), "-t", "3", "--f64", "-p", "0"]
    one = run(base + ["--user-weights", "w.txt", d, "one.model"], tmp_path)
    assert one.returncode == 0, one.stderr
    two = run(base + ["--user-weights", "w.txt", "--gpus", "2", "--devices", "0,0", "--comm", "p2p", d, "two.model"], tmp_path)
    assert two.returncode == 0, two.stderr
    plain = run(base + [d, "plain.model"], tmp_path)
    assert plain.returncode == 0, plain.stderr
    a, b, p = (np.frombuffer(open(tmp_path / n, "rb").read(), np.float64) for n in ("one.model", "two.model", "plain.model"))
    assert a.shape == b.shape and np.nanmax(np.abs(a[2:] - b[2:])) < 1e-9 * np.nanmax(np.abs(a[2:]))
    assert np.nanmax(np.abs(a[2:] - p[2:])) > 1e-3 * np.nanmax(np.abs(a[2:]))
    la = [l for l in one.stdout.split("\n") if l.startswith("Iter")]
    lb = [l for l in two.stdout.split("\n") if l.startswith("Iter")]
    lp = [l for l in plain.stdout.split("\n") if l.startswith("Iter")]
    assert len(la) == len(lb) == 4 and [l.split()[-1] for l in la] == [l.split()[-1] for l in lb] and la[0].split()[-1] != lp[0].split()[-1]


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["pairs", "ratings"])
def test_cli_normalize_is_the_weights_file_of_user_weights(scheme, tmp_path):
    """--normalize pairs writes the model of --user-weights with the file written from user_weights(..., PCR_WEIGHT_PAIRS), byte
    for byte (and --normalize ratings that of PCR_WEIGHT_RATINGS)."""
    g, d, R = _golden_dir("mid5", tmp_path)
    ds = pcr.Dataset.from_ratings(R)
    w = pcr.user_weights(ds, pcr.PCR_WEIGHT_PAIRS if scheme == "pairs" else pcr.PCR_WEIGHT_RATINGS, pcr.PCR_SOLVER_PCRPP)
    assert w.min() < 0.9 and w.max() > 1.1
    _write_weights(tmp_path / "w.txt", w)
    base = [TRAIN, "-k", str(int(g["r"])), "-l", repr(float(g["lam"])), "-t", "2", "-p", "0"]
    a = run(base + ["--normalize", scheme, d, "a.model"], tmp_path)
    b = run(base + ["--user-weights", "w.txt", d, "b.model"], tmp_path)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    raw = open(tmp_path / "a.model", "rb").read()
    assert raw == open(tmp_path / "b.model", "rb").read() and struct.unpack("l", raw[:8])[0] == R.d1
    objs = [[l.split()[-1] for l in x.stdout.split("\n") if l.startswith("Iter")] for x in (a, b)]       # (the lines' times differ)
    assert objs[0] == objs[1] and len(objs[0]) == 3


@pytest.mark.gpu
@pytest.mark.parametrize("pname,solver,r", [("F64", 2, 7), ("F32", 2, 7), ("F64", 1, 7), ("F32", 2, 100)])
def test_weights_set_mid_run(pname, solver, r):
    """After iterate(1): set_user_weights(w), then objective() is the reference's at the current factors (the sorted state the U
    step left stays valid, the queued sums are dropped), and the next iterate(1) is that of a solver given the same factors and
    weights from the start -- to the tolerance the project holds a step to against the oracle: the one continues from the state
    k_ustep left, the other from a k_prepare of its own, and in fp32 their scores differ in the last bit."""
    c = case(r, solver, real=True)
    t = TOL[PREC[pname]]
    w = np.exp(np.random.default_rng(3 * r + solver).uniform(np.log(0.1), np.log(10.0), c.d1))
    s = make(c, pname)
    fresh = make(c, pname)
    try:
        s.set_factors(c.U, c.V)
        s.iterate(1)
        s.set_user_weights(w)
        o = s.objective()
        U1, V1 = s.get_factors()
        terms = uw.user_terms(U1, V1, c.idx, c.citem, c.cval, solver, c.a)
        obj = uw.combine(terms, w, c.lam)[0]
        assert abs(o / obj - 1) < t["obj"], (o, obj)
        fresh.set_factors(U1, V1)
        fresh.set_user_weights(w)
        ra, rb = s.iterate(1)[0], fresh.iterate(1)[0]
        Ua, Va = s.get_factors(); Ub, Vb = fresh.get_factors()
        assert rel(Ua, Ub) < t["fac"] and rel(Va, Vb) < t["fac"] and abs(ra["obj"] / rb["obj"] - 1) < t["fac"]
        assert ra["obj"] <= o
    finally:
        s.close(); fresh.close()


@pytest.mark.gpu
def test_refusals():
    """CCDR1 and the three optional kernel families are PCR_ERR_UNSUPPORTED with the reason; a weight that is 0, negative, NaN or
    infinite is PCR_ERR_ARG and leaves the solver usable and as it was (here: unweighted)."""
    c = case(7, 2)
    s = pcr.Solver(c.ds, pcr.Parameter(k=7, solver_type=pcr.PCR_SOLVER_CCDR1, **{"lambda": 1.0}))
    with pytest.raises(pcr.PcrError, match=r"error -7.*CCDR1"):
        s.set_user_weights(np.ones(c.d1))
    s.close()
    for knob in ({"ustep_newton": "1"}, {"ustep_gram": "64"}, {"vblock_users": "8"}):
        s = make(c, "F32", variant=knob)
        with pytest.raises(pcr.PcrError, match="error -7.*" + list(knob)[0]):
            s.set_user_weights(np.ones(c.d1))
        with pytest.raises(pcr.PcrError, match="error -7"):
            s.set_user_weights(None)
        s.close()
    s = make(c, "F64")
    plain = make(c, "F64")
    try:
        for x in (s, plain):
            x.set_factors(c.U, c.V)
        ref = first_order(plain, c)
        for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
            w = np.ones(c.d1); w[c.d1 // 2] = bad
            with pytest.raises(pcr.PcrError, match=f"error -1.*user {c.d1 // 2}"):
                s.set_user_weights(w)
            got = first_order(s, c)
            assert got[0] == ref[0] and np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]), bad
        with pytest.raises(ValueError):
            s.set_user_weights(np.ones(c.d1 - 1))
    finally:
        s.close(); plain.close()
