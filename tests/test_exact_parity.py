"""Exact parity on dyadic inputs: fp32 and fp64, both solvers, every rank class, every launch variant.

With factors and probe vectors in {-1, -1/2, 0, 1/2, 1} and lambda = 32 (tests/exact_data.py) every product and every sum inside
comp_m, objective, obtain_g and compute_Ha is exact in fp32 and in fp64, whatever the summation order, tiling, split or stream
placement, and the results are representable in fp32.  So the device must return the oracle's numbers BIT FOR BIT -- one dropped
or doubled rating, one off-by-one hinge window at a class edge, changes an integer count of quarter units and fails the test,
where the relative tolerances of tests/test_gpu_parity.py (2e-4 of the matrix maximum in fp32) cannot see it.

Part 1 (CPU) proves the precondition with the oracle alone and holds the oracle to a definitional brute force in numpy integer
arithmetic.  Parts 2 and 3 (GPU) are the exact checks, one solver and across user shards.  Part 4 holds what cannot be exact (the
U step's CG and line search, the trajectory) to the project's own fp32 numbers, per user and under every variant.
"""
import numpy as np
import pytest

import exact_data as ed
import primalcr_amd as pcr
from test_gpu_parity import TOL, VARIANTS

PREC = {"F64": pcr.PCR_F64, "F32": pcr.PCR_F32}

# ---- launch variants: the list of test_launch_variants_agree plus the forms it does not reach
EXTRA_VARIANTS = [
    {"win16": 0, "ustep_win_lds": 0},                                  # 32-bit window rows from global memory
    {"count_rows": 1},                                                 # the counting instantiation of k_ustep: same results
    # fp32 users in the 512-thread throughput class (two classes above 1024 ratings, 80 KB of LDS) under other class layouts,
    # with and without the clusters that would take the longest users out of it
    {"ustep_mode": 2, "cluster_k": 1},
    {"ustep_mode": 2, "ubins": "64:64:0,512:256:0"},
    {"ustep_mode": 2, "ubins": "16:64:1,48:64:1,200:256:0,700:256:0", "cluster_k": 1},
    {"ustep_mode": 2, "cluster_k": 1, "window_cache": 0},
]
R100_VARIANTS = [{"vblock_users": 24}, {"vblock_users": 64}]          # the dense MFMA V step at the headline rank (k = 100)
ALL_VARIANTS = VARIANTS + EXTRA_VARIANTS
# the fixed subset for the cells that do not take the full list: default, throughput and latency forms, no clusters, a coarse
# class layout, many SpMM tiles, one stream, searching sweeps, item ranges over the CSC plan, the blocked-user V step
SUBSET = [{}, {"ustep_mode": "2"}, {"ustep_mode": "1"}, {"cluster_k": "1"}, {"ubins": "64:64:0,512:256:0"}, {"spmm_tiles": "64"},
          {"lanes": "1"}, {"window_cache": "0"}, {"allreduce_chunks": "4", "sddmm_csc": "1"}, {"vblock_users": "8"},
          {"win16": 0, "ustep_win_lds": 0}, {"ustep_mode": 2, "cluster_k": 1}]
FULL_CELLS = {("F32", 2, 12), ("F32", 2, 100), ("F64", 2, 12)}       # cells that run every variant


def vid(v):
    return ",".join(f"{k}={v[k]}" for k in v) if v else "default"


def _cells():
    out = []
    for pname in ("F64", "F32"):
        for solver in (2, 1):
            for r in ed.RANKS:
                vs = list(ALL_VARIANTS if (pname, solver, r) in FULL_CELLS else SUBSET)
                if r == 100:
                    vs += R100_VARIANTS
                for v in vs:
                    out.append(pytest.param(pname, solver, r, v, id=f"{pname}-s{solver}-r{r}-{vid(v)}"))
    return out


assert all(v in ALL_VARIANTS for v in SUBSET)

_REF = {}


def reference(oracle, r, solver, real=False):
    """The dyadic case and the oracle's m, objective, g and Ha for both probes (cached: the oracle runs once per case)."""
    key = (r, solver, real)
    if key not in _REF:
        c = ed.dyadic_case(r, solver, real=real)
        c.X = X = oracle.build_csr(c.d1, c.d2, c.user, c.item, c.val)
        c.m = oracle.comp_m(c.U, c.V, X)
        c.obj = oracle.objective_new(c.m, c.U, c.V, X, c.lam, solver=solver)
        c.g = oracle.obtain_g_new(c.U, c.V, X, c.m, c.lam, solver=solver)
        c.Ha = oracle.compute_Ha_new(c.a, c.m, c.U, X, c.lam, solver=solver)
        c.Ha2 = oracle.compute_Ha_new(c.a2, c.m, c.U, X, c.lam, solver=solver)
        c.lens = np.diff(X.idx)
        c.ds = pcr.Dataset.from_triplets(c.d1, c.d2, c.user, c.item, c.val)
        _REF[key] = c
    return _REF[key]


def is_f32(x):
    x = np.asarray(x, np.float64)
    return np.array_equal(x, x.astype(np.float32).astype(np.float64))


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the precondition, on the CPU
# ------------------------------------------------------------------------------------------------------------------------------

CPU_CASES = [(r, s, False) for s in (2, 1) for r in ed.RANKS] + [(7, 2, True), (12, 1, True), (100, 2, True)]


@pytest.mark.parametrize("r,solver,real", CPU_CASES, ids=[f"r{r}-s{s}-{'real' if x else 'int'}" for r, s, x in CPU_CASES])
def test_dyadic_preconditions_and_integer_brute_force(oracle, r, solver, real):
    """What makes "exact" legitimate, with the oracle alone: m, g, Ha are their own float32 round trip; max |.| in units of 1/4
    stays below 2^22 (two spare bits under fp32's 24: the partial sums of a split reduction stay exact too); the objective is a
    whole number of sixteenths far inside fp64; both sides of the hinge window are populated; every user-length class boundary
    is present; feeding the ratings in another order changes no bit.  Then the oracle against the definition itself, in numpy
    INTEGER arithmetic scaled to the unit (exact_data.brute_force): objective and gradient must be equal -- that is the plain
    high-precision reference; Ha is held to its own integer definition (item_edge_data.brute_force_Ha) on this fixture by
    tests/test_item_edges.py::test_Ha_equals_its_integer_definition_on_the_user_edge_fixture."""
    c = reference(oracle, r, solver, real)
    X = c.X
    assert set(ed.CLASS_EDGES) <= set(c.lens.tolist()) and c.lens.max() > 4097
    assert c.lam == 32.0 and set(np.unique(np.abs(np.concatenate([c.U.ravel(), c.V.ravel(), c.a.ravel(), c.a2.ravel()])))) <= {0.0, 0.5, 1.0}
    if real:
        lv = ed.levels_of(X.val, 1)
        assert not np.array_equal(lv, np.rint(lv)) and set(np.rint(X.val)) == {1.0, 2.0, 3.0, 4.0, 5.0}
    for name, x in (("m", c.m), ("g", c.g), ("Ha", c.Ha), ("Ha2", c.Ha2)):
        assert is_f32(x), name
        assert np.array_equal(x * ed.UNIT, np.rint(x * ed.UNIT)), name
        assert np.abs(x).max() * ed.UNIT < 2 ** 22, (name, np.abs(x).max())
    assert c.obj * 16 == np.rint(c.obj * 16) and c.obj * 16 < 2 ** 50
    # order independence: the triplets shuffled (the CSR builder sorts them back), and a CSR whose users list their ratings in
    # another order (every per-user sum inside the oracle then runs in another order)
    rng = np.random.default_rng(r + solver)
    p = rng.permutation(len(c.user))
    Xs = oracle.build_csr(c.d1, c.d2, c.user[p], c.item[p], c.val[p])
    q = np.concatenate([X.idx[u] + rng.permutation(int(n)) for u, n in enumerate(c.lens)]).astype(np.int64)
    from oracle.oracle_py import CSR
    Xq = CSR(c.d1, c.d2, X.idx, X.item[q], X.val[q])
    assert np.array_equal(Xs.idx, X.idx) and np.array_equal(Xs.item, X.item) and np.array_equal(Xs.val, X.val)
    mq = oracle.comp_m(c.U, c.V, Xq)
    assert np.array_equal(mq, c.m[q])
    assert oracle.objective_new(mq, c.U, c.V, Xq, c.lam, solver=solver) == c.obj
    assert np.array_equal(oracle.obtain_g_new(c.U, c.V, Xq, mq, c.lam, solver=solver), c.g)
    assert np.array_equal(oracle.compute_Ha_new(c.a, mq, c.U, Xq, c.lam, solver=solver), c.Ha)
    # the definition, in integers
    obj16, g4, m4, active, comparable = ed.brute_force(c, X.idx, X.item, X.val)
    assert np.array_equal(c.m * ed.UNIT, m4)
    assert c.obj * 16 == obj16, (c.obj * 16, obj16)
    assert np.array_equal(c.g * ed.UNIT, g4)
    share = active / comparable
    # [0.2, 0.9] where the scores span several hinge widths (r >= 12).  Below, they do not: at r = 1 every score lies in [-1, 1]
    # and a difference of a whole unit is rarer; what matters there -- pairs on both sides of the window in every long user --
    # still holds with a twentieth of them outside
    assert 0.2 <= share <= (0.9 if r >= 12 else 0.95), share
    if solver == 1 and real:
        assert comparable == int((c.lens * (c.lens - 1) // 2).sum())            # every pair of a user is comparable


# ------------------------------------------------------------------------------------------------------------------------------
# 2. exact first-order parity on the GPU
# ------------------------------------------------------------------------------------------------------------------------------

def where_m(c, z):
    u = int(np.searchsorted(c.X.idx, z, side="right") - 1)
    return f"rating {z}: user {u}, item {int(c.X.item[z])}, {ed.class_of(int(c.lens[u]))}"


def where_item(c, flat):
    it, col = divmod(int(flat), c.r)
    raters = np.flatnonzero(c.X.item == it)
    users = np.searchsorted(c.X.idx, raters, side="right") - 1
    who = "; ".join(f"user {int(u)} {ed.class_of(int(c.lens[u]))}" for u in users[:12])
    return f"item {it}, column {col}, rated by {len(users)} users: {who}{' ...' if len(users) > 12 else ''}"


def assert_same(tag, name, got, ref, c, where):
    """np.array_equal with a message the next kernel author can read the cause from."""
    got = np.asarray(got); ref = np.asarray(ref)
    assert got.shape == ref.shape, (tag, name, got.shape, ref.shape)
    bad = np.flatnonzero(got.ravel() != ref.ravel())
    if bad.size:
        z = int(bad[0])
        pytest.fail(f"{tag}: {name} differs from the oracle in {bad.size} of {got.size} entries; first at {where(c, z)}: "
                    f"got {got.ravel()[z]!r}, expected {ref.ravel()[z]!r} (difference {(got.ravel()[z] - ref.ravel()[z]) * ed.UNIT:g} quarter units)")


def check_first_order(s, c, tag):
    assert_same(tag, "m", s.comp_m(), c.m, c, where_m)
    obj = s.objective()
    assert obj == c.obj, f"{tag}: objective {obj!r}, oracle {c.obj!r} ({(obj - c.obj) * 16:g} sixteenths)"
    assert_same(tag, "g", s.obtain_g(), c.g, c, where_item)
    assert_same(tag, "Ha", s.compute_Ha(c.a), c.Ha, c, where_item)
    assert_same(tag, "Ha (second probe)", s.compute_Ha(c.a2), c.Ha2, c, where_item)
    assert_same(tag, "g after the probes", s.obtain_g(), c.g, c, where_item)            # state survives compute_Ha
    assert s.objective() == c.obj, tag


@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize("pname,solver,r,variant", _cells())
def test_first_order_entry_points_are_exact(oracle, pname, solver, r, variant):
    """comp_m, objective, obtain_g and compute_Ha (two probes, then obtain_g again) equal the oracle bit for bit, in both
    precisions, both solvers, ranks 1 / 7 / 12 / 100 / 132, under every launch variant: the whole list for (F32, solver 2,
    r = 12 and 100) and (F64, solver 2, r = 12), the fixed SUBSET for the other cells, the blocked-user V step with larger blocks
    at r = 100.  A failure names the variant, precision, solver, rank, the first differing (user or item, column) and the
    length class of the users involved."""
    c = reference(oracle, r, solver)
    with pcr.tuned(**variant):
        s = pcr.Solver(c.ds, pcr.Parameter(k=r, solver_type=solver, precision=PREC[pname], **{"lambda": c.lam}))
    try:
        s.set_factors(c.U, c.V)
        check_first_order(s, c, f"variant {vid(variant)}, {pname}, solver {solver}, r = {r}")
    finally:
        s.close()


REAL_CELLS = [(p, s, r, v) for p in ("F64", "F32") for (s, r) in ((2, 7), (1, 12), (2, 100))
              for v in ({}, {"ustep_mode": "2"}, {"window_cache": "0"}, {"spmm_tiles": "16"}, {"vblock_users": "8"})]


@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize("pname,solver,r,variant", REAL_CELLS, ids=[f"{p}-s{s}-r{r}-{vid(v)}" for p, s, r, v in REAL_CELLS])
def test_first_order_entry_points_are_exact_on_real_valued_ratings(oracle, pname, solver, r, variant):
    """The same with ratings off the integers: PrimalCR++ buckets them by lround (5 levels), PrimalCR compares the raw doubles
    (a level per rating: no window cache, the level-count-sized scratch of the long classes)."""
    c = reference(oracle, r, solver, real=True)
    with pcr.tuned(**variant):
        s = pcr.Solver(c.ds, pcr.Parameter(k=r, solver_type=solver, precision=PREC[pname], **{"lambda": c.lam}))
    try:
        s.set_factors(c.U, c.V)
        check_first_order(s, c, f"variant {vid(variant)}, {pname}, solver {solver}, r = {r}, real-valued ratings")
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 3. exact sharding
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize("pname", ["F64", "F32"])
@pytest.mark.parametrize("nranks", [2, 3, 5])
def test_user_shards_add_up_exactly(oracle, nranks, pname):
    """Shard-local mode on one GPU: the shards' partial g and Ha, summed on the host, equal the one-rank result (and the
    oracle) exactly; so does the objective once the replicated lambda/2 |V|^2 is counted once; the concatenated m is
    identical.  (test_user_sharding_on_one_gpu holds this to 1e-12, in fp64 only.)"""
    for solver, r in ((2, 12), (2, 100), (1, 12)):
        c = reference(oracle, r, solver)
        tag = f"{nranks} ranks, {pname}, solver {solver}, r = {r}"
        par = dict(k=r, solver_type=solver, precision=PREC[pname], **{"lambda": c.lam})
        bounds = pcr.partition_users(c.X.idx, nranks)
        m_parts, g_sum, Ha_sum, obj_sum = [], 0.0, 0.0, 0.0
        for q in range(nranks):
            s = pcr.Solver(c.ds, pcr.Parameter(**par), rank=q, nranks=nranks)
            assert (s.first_user, s.n_users) == (bounds[q], bounds[q + 1] - bounds[q])
            s.set_local_only(True)
            s.set_factors(c.U, c.V)
            m_parts.append(s.comp_m())
            obj_sum += s.objective()
            g_sum = g_sum + s.obtain_g()
            Ha_sum = Ha_sum + s.compute_Ha(c.a)
            s.close()
        full = pcr.Solver(c.ds, pcr.Parameter(**par))
        full.set_factors(c.U, c.V)
        m_full = full.comp_m(); obj_full = full.objective(); g_full = full.obtain_g(); Ha_full = full.compute_Ha(c.a)
        full.close()
        # replicated terms: every shard adds lambda/2 |V|^2 to its local objective (count it once); lambda V and lambda a ride on
        # rank 0's partial alone (Solver::obtain_g / compute_Ha), so the partial g and Ha add up as they are
        obj_sum -= (nranks - 1) * c.lam / 2.0 * float((c.V ** 2).sum())
        assert_same(tag, "concatenated m", np.concatenate(m_parts), m_full, c, where_m)
        assert_same(tag, "sum of shard g (against one rank)", g_sum, g_full, c, where_item)
        assert_same(tag, "sum of shard Ha (against one rank)", Ha_sum, Ha_full, c, where_item)
        assert obj_sum == obj_full, (tag, obj_sum, obj_full)
        assert_same(tag, "sum of shard g", g_sum, c.g, c, where_item)
        assert_same(tag, "sum of shard Ha", Ha_sum, c.Ha, c, where_item)
        assert obj_sum == c.obj, (tag, obj_sum, c.obj)


# ------------------------------------------------------------------------------------------------------------------------------
# 4. what cannot be exact: the U step and the trajectory
# ------------------------------------------------------------------------------------------------------------------------------

_STEP = {}


def oracle_steps(oracle, r):
    """From the dyadic start: the oracle's first U step (no V step before it) and two outer iterations half step by half step."""
    if r not in _STEP:
        c = reference(oracle, r, 2)
        U1, objU, iu = oracle.update_U_new(c.X, c.m, c.lam, 1.0, c.V, c.U)
        U, V, half, cg_v = c.U, c.V, [], []
        for _ in range(2):
            V, m, oV, iv = oracle.update_V_new(c.X, c.lam, 1.0, U, V)
            U, oU, _ = oracle.update_U_new(c.X, m, c.lam, 1.0, V, U)
            half += [oV, oU]; cg_v.append(iv["cg"])
        _, _, recs = oracle.train(c.X, c.U, c.V, c.lam, 2, do_predict=0)
        assert [x["obj"] for x in recs[1:]] == half[1::2] and [x["cg_v"] for x in recs[1:]] == cg_v      # the same trajectory
        _STEP[r] = (U1, objU, iu, half, cg_v)
    return _STEP[r]


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("r", [12, 100])
@pytest.mark.parametrize("pname", ["F32", "F64"])
def test_first_u_step_per_user_under_every_variant(oracle, pname, r):
    """set_factors; comp_m(); update_U() from the dyadic start (V and m still exact: only the U step's own arithmetic is under
    test), every user's row against oracle.update_U_new under every launch variant:
        max |dU[u]| <= TOL[precision]["fac"] * max(|U_o[u]|_inf, 1e-3 |U_o|_inf)
    -- the project's own number (5e-3 in fp32, 1e-7 in fp64), applied per row instead of over the whole matrix; the floor is
    there because users without comparable pairs are driven to ~1e-17.  fp64: the inner counts equal the oracle's.  The largest
    ratio to the bound is printed (NOTES.md records it)."""
    c = reference(oracle, r, 2)
    Uo, objUo, iu, _, _ = oracle_steps(oracle, r)
    fac = TOL[PREC[pname]]["fac"]
    bound = fac * np.maximum(np.abs(Uo).max(1), 1e-3 * np.abs(Uo).max())
    failures, worst = [], (0.0, None)
    for v in ALL_VARIANTS:
        with pcr.tuned(**v):
            s = pcr.Solver(c.ds, pcr.Parameter(k=r, precision=PREC[pname], **{"lambda": c.lam}))
        s.set_factors(c.U, c.V)
        s.comp_m()
        objU, info = s.update_U()
        Ug, _ = s.get_factors()
        s.close()
        ratio = np.abs(Ug - Uo).max(1) / bound
        u = int(ratio.argmax())
        if ratio[u] > worst[0]:
            worst = (float(ratio[u]), f"{vid(v)}: user {u}, {ed.class_of(int(c.lens[u]))}")
        if not ratio[u] <= 1.0:
            failures.append(f"variant {vid(v)}, {pname}, r = {r}: {int((ratio > 1).sum())} users beyond the bound; worst user {u}, "
                            f"{ed.class_of(int(c.lens[u]))}: max |dU| = {np.abs(Ug[u] - Uo[u]).max():.3e}, bound {bound[u]:.3e}")
        if pname == "F64" and (info["cg"], info["ls"]) != (iu["cg"], iu["ls"]):
            failures.append(f"variant {vid(v)}, F64, r = {r}: inner counts {info} against the oracle's {iu}")
    print(f"[exact-parity] first U step {pname} r={r}: largest per-row |dU| / bound = {worst[0]:.3e} ({worst[1]})")
    assert not failures, "\n".join(failures)


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("r", [12, 100])
def test_two_fp32_iterations_under_every_variant(oracle, r):
    """Two outer iterations in fp32 from the dyadic start under every launch variant: the objective after each half step within
    1e-3 relative of the oracle's trajectory (the fp32 contract of README.md and test_fp32_training_matches_reference_quality)
    and the V side's CG counts equal to the oracle's, as that test asserts."""
    c = reference(oracle, r, 2)
    _, _, _, half, cg_v = oracle_steps(oracle, r)
    failures, worst = [], 0.0
    for v in ALL_VARIANTS:
        with pcr.tuned(**v):
            s = pcr.Solver(c.ds, pcr.Parameter(k=r, precision=pcr.PCR_F32, **{"lambda": c.lam}))
        s.set_factors(c.U, c.V)
        objs, cgs = [], []
        for _ in range(2):
            oV, iv = s.update_V(); oU, _ = s.update_U()
            objs += [oV, oU]; cgs.append(iv["cg"])
        s.close()
        err = [abs(a / b - 1) for a, b in zip(objs, half)]
        worst = max(worst, max(err))
        if not max(err) < 1e-3:
            failures.append(f"variant {vid(v)}, r = {r}: objectives {objs} against the oracle's {half} (relative {err})")
        if cgs != cg_v:
            failures.append(f"variant {vid(v)}, r = {r}: cg_v {cgs} against the oracle's {cg_v}")
    print(f"[exact-parity] two fp32 iterations r={r}: largest relative objective difference {worst:.3e}")
    assert not failures, "\n".join(failures)
