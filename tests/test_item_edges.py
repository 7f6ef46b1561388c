"""The V step at the item-degree edges of the SpMM plan: exact parity on a rating set designed by item.

tests/test_exact_parity.py pins the user side down (a user of every length-class boundary, bit for bit), but every fixture that
feeds the V step draws each user's items uniformly: item degrees of 3 .. 29, no empty item, never a chunk inside one column.
The kernels that turn a per-rating vector into an item-major result -- k_spmm / k_spmm_fin, the tile-major CSC of k_sddmm,
k_vblock_b / k_vblock_hp and the device-side plan builder (pcr_plan_dev.h) -- are written around item structure.  The fixture
of tests/item_edge_data.py has a hot item rated by everyone, empty items (the second, the last, a run that empties whole item
ranges), a ladder of degrees around every power of two up to d1 - 1, a block of 320 single-rating items and two dense users, with
the dyadic factors of tests/exact_data.py: comp_m, objective, obtain_g and compute_Ha must equal the oracle BIT FOR BIT under
every tiling, chunk length, item-range count, CSC form, key width and dense block -- one dropped or doubled (chunk, item)
incidence changes an integer count of quarter units.

Part 1 (CPU): the fixture reaches the edges it is meant to (plan_shape: conditions, not measurements), the exactness
precondition, the oracle against the integer definition -- now for the Hessian-vector product too, here and on the user-edge
fixture.  Parts 2-3 (GPU): the exact cells, one rank and user shards.  Parts 4-5: what cannot be exact (a whole V step, two outer
iterations) to the project's own tolerances, with equal inner counts in fp64.
"""
import numpy as np
import pytest

import exact_data as ed
import item_edge_data as ie
import primalcr_amd as pcr
from test_exact_parity import assert_same, check_first_order, is_f32, vid, where_item, where_m
from test_exact_parity import reference as user_edge_reference
from test_gpu_parity import TOL, rel

PREC = {"F64": pcr.PCR_F64, "F32": pcr.PCR_F32}

# ---- the V-side launch list: every form of the plan, and what each means for the cutting rule (tiles, chunk, item ranges).
# Not forced: 2 tiles (640 users: nu / 256 = 2) and chunks of 64 (7409 ratings fit the chip in one round: the floor of
# plan_pick_chunk); the dense block (vblock_users) takes users 5 and 633 out of the chunks and runs one item range.
VSIDE = [
    {},
    {"spmm_tiles": 1, "spmm_chunk": 8}, {"spmm_tiles": 1, "spmm_chunk": 32}, {"spmm_tiles": 1, "spmm_chunk": 64},
    {"spmm_tiles": 1, "spmm_chunk": 128},
    {"spmm_tiles": 2}, {"spmm_tiles": 4}, {"spmm_tiles": 5, "spmm_chunk": 32}, {"spmm_tiles": 8}, {"spmm_tiles": 16, "spmm_chunk": 32},
    {"spmm_tiles": 64, "spmm_chunk": 8},
    {"allreduce_chunks": 3}, {"allreduce_chunks": 64, "spmm_tiles": 16}, {"allreduce_chunks": 4, "sddmm_csc": 1},
    {"sddmm_csc": 1, "spmm_tiles": 16},
    {"plan_key64": 1}, {"plan_key64": 1, "allreduce_chunks": 3, "spmm_tiles": 16},
    {"vblock_users": 2}, {"vblock_users": 8}, {"vblock_users": 33, "spmm_tiles": 4},
]
R100_VSIDE = [{"vblock_users": 64}]
# the fixed subset for the cells that do not take the full list: default, the shortest and the longest chunk on one tile, a tile
# per XCD, more tiles than XCDs, 64 item ranges (whole ranges empty), ranges over the CSC form, the dense block
SUBSET = [{}, {"spmm_tiles": 1, "spmm_chunk": 8}, {"spmm_tiles": 1, "spmm_chunk": 128}, {"spmm_tiles": 8},
          {"spmm_tiles": 64, "spmm_chunk": 8}, {"allreduce_chunks": 64, "spmm_tiles": 16}, {"allreduce_chunks": 4, "sddmm_csc": 1},
          {"vblock_users": 8}]
assert all(v in VSIDE for v in SUBSET)
FULL_CELLS = {("F32", 2, 12), ("F32", 2, 100), ("F64", 2, 12)}
CELLS = [(2, r, False) for r in ed.RANKS] + [(1, 12, False)]
REAL = [(2, 7, True), (1, 12, True)]


def plan_config(v):
    """(tiles, chunk, item ranges, users left out of the chunks) of a launch variant on the whole fixture."""
    block = "vblock_users" in v
    return (int(v.get("spmm_tiles", 2)), int(v.get("spmm_chunk", 64)), 1 if block else int(v.get("allreduce_chunks", 1)),
            ie.DENSE if block else ())


_REF = {}


def reference(oracle, r, solver, real=False):
    """The item-edge case and the oracle's m, objective, g and Ha for both probes (cached: the oracle runs once per case)."""
    key = (r, solver, real)
    if key not in _REF:
        c = ie.item_edge_case(r, solver, real=real)
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


# ------------------------------------------------------------------------------------------------------------------------------
# 1. on the CPU: the structure, the precondition, the definition
# ------------------------------------------------------------------------------------------------------------------------------

def test_fixture_reaches_every_item_edge():
    """Conditions on the generator (if one fails, change the generator): the degree set holds every rung of the ladder, 0, 1 and
    d1; the table starts with the full item and ends with an empty one behind a rated one; a run of >= 40 empty items; and under
    the plan's cutting rule (item_edge_data.plan_shape) the launch list reaches, taken together, every edge of k_spmm /
    k_spmm_fin / launch_spmm_range -- the one-tile, chunk-64 plan alone already a chunk wholly inside a column, an all-new chunk,
    an item without a slot and one with more than eight."""
    c = ie.item_edge_case(12, 2)
    deg = c.deg
    assert np.array_equal(deg, ie.item_degrees()) and (c.d1, c.d2) == (ie.D1, ie.D2) == (640, 1031)
    assert set(ie.LADDER) | {0, 1, c.d1} <= set(deg.tolist()) and ie.LADDER[-1] == c.d1 - 1
    assert [int(deg[j]) for j in ie.LADDER_ITEMS] == list(ie.LADDER)
    assert deg[0] == c.d1 and deg[1] == 0 and deg[c.d2 - 1] == 0 and deg[c.d2 - 2] == 1
    assert c.user[c.item == c.d2 - 2].tolist() == [c.d1 - 1]
    empty = np.flatnonzero(deg == 0)
    runs = np.split(empty, np.flatnonzero(np.diff(empty) != 1) + 1)
    assert max(len(x) for x in runs) >= 40
    lo, hi = ie.SINGLES
    assert hi - lo >= 300 and (deg[lo:hi] == 1).all() and not np.isin(c.user[(c.item >= lo) & (c.item < hi)], ie.DENSE).any()
    assert len(set(zip(c.user.tolist(), c.item.tolist()))) == len(c.user)          # no pair twice (the dense block's table)
    lens = np.bincount(c.user, minlength=c.d1)
    idx = np.concatenate([[0], np.cumsum(lens)])
    assert np.all(np.diff(c.user) >= 0)
    # the dense users: every rated item outside the singles (user 5; user 633 from degree 2 on), the only users that qualify for
    # the dense block (a sixteenth of the catalogue) and the only ones near 512 ratings: the user side stays small
    rated = np.flatnonzero((deg > 0) & ~((np.arange(c.d2) >= lo) & (np.arange(c.d2) < hi)) & (np.arange(c.d2) != c.d2 - 2))
    assert np.array_equal(np.sort(c.item[c.user == ie.DENSE[0]]), rated)
    assert np.array_equal(np.sort(c.item[c.user == ie.DENSE[1]]), rated[deg[rated] >= 2])
    assert lens[ie.DENSE[0]] > 512 and set(np.flatnonzero(lens * 16 >= c.d2).tolist()) == set(ie.DENSE)
    assert np.delete(lens, ie.DENSE).max() <= 64
    # item ranges of allreduce_chunks = 64: at least one whole range without any rating
    b = np.array([c.d2 * q // 64 for q in range(65)])
    assert any(deg[b[q]:b[q + 1]].sum() == 0 for q in range(64))

    shapes = {vid(v): ie.plan_shape(idx, c.item, c.d2, *plan_config(v)) for v in VSIDE + R100_VSIDE}
    one = shapes["spmm_tiles=1,spmm_chunk=64"]
    assert one["inside"] > 0 and one["all_new"] > 0 and 0 in one["slot_counts"] and max(one["slot_counts"]) >= 9, one
    slots = set().union(*(s["slot_counts"] for s in shapes.values()))
    assert {0, 1, 7, 8, 9, 15, 16, 17} <= slots and max(slots) > 64, sorted(slots)
    for edge in ("inside", "all_new", "flag_on_32", "flag_on_64", "flag_on_last", "empty_tile_range", "empty_range"):
        assert any(s[edge] for s in shapes.values()), edge
    assert all(s["inside"] > 0 for k, s in shapes.items() if k.startswith("spmm_tiles=1,"))
    assert {1, 2, 7} <= set().union(*(s["short_last"] for s in shapes.values()))     # ragged last chunks, shorter than one unroll
    assert shapes["allreduce_chunks=64,spmm_tiles=16"]["empty_range"]
    assert shapes["vblock_users=8"]["slab_rows"] < shapes["default"]["slab_rows"]


CPU_CASES = CELLS + REAL


@pytest.mark.parametrize("solver,r,real", CPU_CASES, ids=[f"r{r}-s{s}-{'real' if x else 'int'}" for s, r, x in CPU_CASES])
def test_item_edge_preconditions_and_integer_brute_force(oracle, solver, r, real):
    """As test_dyadic_preconditions_and_integer_brute_force, for every case the GPU part uses: m, g, Ha are their own float32
    round trip and whole quarter units below 2^22, the objective whole sixteenths below 2^50, both sides of the hinge window
    populated; the oracle's m, objective and g equal the integer definition (exact_data.brute_force) and its Ha for BOTH probes
    the integer definition of the Hessian-vector product (item_edge_data.brute_force_Ha)."""
    c = reference(oracle, r, solver, real)
    X = c.X
    assert c.lam == 32.0 and set(np.unique(np.abs(np.concatenate([c.U.ravel(), c.V.ravel(), c.a.ravel(), c.a2.ravel()])))) <= {0.0, 0.5, 1.0}
    assert np.array_equal(X.item, c.item) and np.array_equal(X.val, c.val)          # the fixture is in CSR order already
    if real:
        lv = ed.levels_of(X.val, 1)
        assert not np.array_equal(lv, np.rint(lv)) and set(np.rint(X.val)) == {1.0, 2.0, 3.0, 4.0, 5.0}
    else:
        assert set(X.val) == {1.0, 2.0, 3.0, 4.0, 5.0}
    for name, x in (("m", c.m), ("g", c.g), ("Ha", c.Ha), ("Ha2", c.Ha2)):
        assert is_f32(x), name
        assert np.array_equal(x * ed.UNIT, np.rint(x * ed.UNIT)), name
        assert np.abs(x).max() * ed.UNIT < 2 ** 22, (name, np.abs(x).max())
    assert c.obj * 16 == np.rint(c.obj * 16) and c.obj * 16 < 2 ** 50
    obj16, g4, m4, active, comparable = ed.brute_force(c, X.idx, X.item, X.val)
    assert np.array_equal(c.m * ed.UNIT, m4)
    assert c.obj * 16 == obj16, (c.obj * 16, obj16)
    assert np.array_equal(c.g * ed.UNIT, g4)
    assert 0.2 <= active / comparable <= (0.9 if r >= 12 else 0.95), active / comparable
    assert np.array_equal(c.Ha * ed.UNIT, ie.brute_force_Ha(c, X.idx, X.item, X.val, c.a))
    assert np.array_equal(c.Ha2 * ed.UNIT, ie.brute_force_Ha(c, X.idx, X.item, X.val, c.a2))
    # an empty item's rows are the lambda terms alone
    nil = np.flatnonzero(c.deg == 0)
    assert np.array_equal(c.g[nil], c.lam * c.V[nil]) and np.array_equal(c.Ha[nil], c.lam * c.a[nil])


@pytest.mark.parametrize("r,solver,real", [(12, 2, False), (100, 2, False), (12, 1, True)], ids=["r12-s2-int", "r100-s2-int", "r12-s1-real"])
def test_Ha_equals_its_integer_definition_on_the_user_edge_fixture(oracle, r, solver, real):
    """The oracle's compute_Ha_new / compute_Ha on exact_data.dyadic_case (users of 0 .. 5000 ratings) against the definition in
    integers, both probes: the Hessian-vector product is held to its definition like the objective and the gradient, not trusted
    through the oracle's sweep form."""
    c = user_edge_reference(oracle, r, solver, real)
    assert np.array_equal(c.Ha * ed.UNIT, ie.brute_force_Ha(c, c.X.idx, c.X.item, c.X.val, c.a))
    assert np.array_equal(c.Ha2 * ed.UNIT, ie.brute_force_Ha(c, c.X.idx, c.X.item, c.X.val, c.a2))


# ------------------------------------------------------------------------------------------------------------------------------
# 2. exact first-order parity on the GPU
# ------------------------------------------------------------------------------------------------------------------------------

def _cells():
    out = []
    for pname in ("F64", "F32"):
        for solver, r, real in CELLS + REAL:
            vs = list(VSIDE if (pname, solver, r) in FULL_CELLS and not real else SUBSET)
            if r == 100:
                vs += R100_VSIDE
            for v in vs:
                out.append(pytest.param(pname, solver, r, real, v, id=f"{pname}-s{solver}-r{r}{'-real' if real else ''}-{vid(v)}"))
    return out


@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize("pname,solver,r,real,variant", _cells())
def test_first_order_entry_points_are_exact_at_item_edges(oracle, pname, solver, r, real, variant):
    """comp_m, objective, obtain_g, compute_Ha (two probes), obtain_g again: the oracle's numbers bit for bit on the item-edge
    fixture, in both precisions, under every form of the V-side plan (the whole list for (F32, solver 2, r = 12 and 100) and
    (F64, solver 2, r = 12), the fixed SUBSET elsewhere).  A failure names the variant, the first differing item, its degree and
    its raters; item_edge_data.plan_shape(idx, item, d2, *plan_config(variant)) tells which chunk and slot that is."""
    c = reference(oracle, r, solver, real)
    with pcr.tuned(**variant):
        s = pcr.Solver(c.ds, pcr.Parameter(k=r, solver_type=solver, precision=PREC[pname], **{"lambda": c.lam}))
    try:
        s.set_factors(c.U, c.V)
        check_first_order(s, c, f"variant {vid(variant)}, {pname}, solver {solver}, r = {r}{', real-valued ratings' if real else ''}, item-edge fixture")
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 3. exact sharding
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize("pname", ["F64", "F32"])
@pytest.mark.parametrize("nranks", [2, 3, 5, 7])
def test_user_shards_add_up_exactly_at_item_edges(oracle, nranks, pname):
    """test_user_shards_add_up_exactly on the item-edge fixture: the hot item and the random-rater rungs get a partial row from
    every shard, the contiguous-rater rungs from one, the singles from the shard of their one rater, the empty items from none
    (rank 0's lambda term alone).  The shards' partial g and Ha, summed on the host, equal the one-rank result and the oracle
    exactly; so does the objective once the replicated lambda/2 |V|^2 is counted once; the concatenated m is identical."""
    for solver, r in ((2, 12), (2, 100)):
        c = reference(oracle, r, solver)
        tag = f"{nranks} ranks, {pname}, solver {solver}, r = {r}, item-edge fixture"
        par = dict(k=r, solver_type=solver, precision=PREC[pname], **{"lambda": c.lam})
        bounds = pcr.partition_users(c.X.idx, nranks)
        m_parts, g_sum, Ha_sum, obj_sum = [], 0.0, 0.0, 0.0
        for q in range(nranks):
            s = pcr.Solver(c.ds, pcr.Parameter(**par), rank=q, nranks=nranks)
            try:
                assert (s.first_user, s.n_users) == (bounds[q], bounds[q + 1] - bounds[q])
                s.set_local_only(True)
                s.set_factors(c.U, c.V)
                m_parts.append(s.comp_m())
                obj_sum += s.objective()
                g_sum = g_sum + s.obtain_g()
                Ha_sum = Ha_sum + s.compute_Ha(c.a)
            finally:
                s.close()
        full = pcr.Solver(c.ds, pcr.Parameter(**par))
        try:
            full.set_factors(c.U, c.V)
            m_full = full.comp_m(); obj_full = full.objective(); g_full = full.obtain_g(); Ha_full = full.compute_Ha(c.a)
        finally:
            full.close()
        obj_sum -= (nranks - 1) * c.lam / 2.0 * float((c.V ** 2).sum())          # every shard counted lambda/2 |V|^2
        assert_same(tag, "concatenated m", np.concatenate(m_parts), m_full, c, where_m)
        assert_same(tag, "sum of shard g (against one rank)", g_sum, g_full, c, where_item)
        assert_same(tag, "sum of shard Ha (against one rank)", Ha_sum, Ha_full, c, where_item)
        assert obj_sum == obj_full, (tag, obj_sum, obj_full)
        assert_same(tag, "sum of shard g", g_sum, c.g, c, where_item)
        assert_same(tag, "sum of shard Ha", Ha_sum, c.Ha, c, where_item)
        assert obj_sum == c.obj, (tag, obj_sum, c.obj)


# ------------------------------------------------------------------------------------------------------------------------------
# 4. the whole V step
# ------------------------------------------------------------------------------------------------------------------------------

_VSTEP = {}
_WORST = {"F64": (0.0, None), "F32": (0.0, None)}


def oracle_v_step(oracle, r):
    if r not in _VSTEP:
        c = reference(oracle, r, 2)
        _VSTEP[r] = oracle.update_V_new(c.X, c.lam, 1.0, c.U, c.V)
    return _VSTEP[r]


def _vstep_cells():
    return [pytest.param(p, r, v, id=f"{p}-r{r}-{vid(v)}") for p in ("F64", "F32") for r in (12, 100)
            for v in VSIDE + (R100_VSIDE if r == 100 else [])]


@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize("pname,r,variant", _vstep_cells())
def test_v_step_from_the_dyadic_point_at_item_edges(oracle, pname, r, variant):
    """update_V() from the dyadic point (gradient, up to ten CG iterations through k_sddmm / the sweeps / k_spmm + k_spmm_fin with
    its fused dot products, the line search) against oracle.update_V_new under every form of the V-side plan, within the project's
    own numbers (test_v_side_vs_golden): the objective to max(TOL obj, 1e-2 TOL cg), V to TOL fac; the state handed to the U step
    -- the sorted scores the line search left -- through objective() read from it, to the same bound, and the scores of the new V
    to TOL fac (they are U V^T: the factors' bound).  fp64: the CG and line-search counts equal the oracle's.  The largest ratio
    to its bound so far is printed per precision (NOTES.md records it)."""
    c = reference(oracle, r, 2)
    Vo, mo, objo, io = oracle_v_step(oracle, r)
    t = TOL[PREC[pname]]
    with pcr.tuned(**variant):
        s = pcr.Solver(c.ds, pcr.Parameter(k=r, precision=PREC[pname], **{"lambda": c.lam}))
    try:
        s.set_factors(c.U, c.V)
        objV, info = s.update_V()
        obj_state = s.objective()
        _, Vg = s.get_factors()
        mg = s.comp_m()
    finally:
        s.close()
    obj_bound = max(t["obj"], t["cg"] * 1e-2)
    ratios = {"objective": abs(objV / objo - 1) / obj_bound, "objective of the handed-over state": abs(obj_state / objo - 1) / obj_bound,
              "V": rel(Vg, Vo) / t["fac"], "m": rel(mg, mo) / t["fac"]}
    worst = max(ratios, key=ratios.get)
    tag = f"variant {vid(variant)}, {pname}, r = {r}"
    if ratios[worst] > _WORST[pname][0]:
        _WORST[pname] = (ratios[worst], f"{worst}, {tag}")
    print(f"[item-edges] V step {tag}: " + ", ".join(f"{k} {v:.3e}" for k, v in ratios.items()) + f" of the bound; counts {info}, oracle {io}; "
          f"largest so far in {pname}: {_WORST[pname][0]:.3e} ({_WORST[pname][1]})")
    assert info["accepted"] == io["accepted"] == 1, (tag, info, io)
    if ratios["V"] > 1:
        j = int(np.abs(Vg - Vo).max(1).argmax())
        pytest.fail(f"{tag}: V differs by {rel(Vg, Vo):.3e} of its scale (bound {t['fac']:.1e}), most at item {j} of degree {int(c.deg[j])}")
    assert all(v <= 1 for v in ratios.values()), (tag, ratios)
    if pname == "F64":
        assert (info["cg"], info["ls"]) == (io["cg"], io["ls"]), (tag, info, io)


# ------------------------------------------------------------------------------------------------------------------------------
# 5. two outer iterations
# ------------------------------------------------------------------------------------------------------------------------------

_TRAIN = {}


@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize("variant", [{}, {"spmm_tiles": 1, "spmm_chunk": 8}, {"vblock_users": 8}], ids=vid)
@pytest.mark.parametrize("r", [12, 100])
def test_two_fp64_iterations_at_item_edges(oracle, r, variant):
    """iterate(2) in fp64 from the dyadic point against oracle.train, as test_fuzz_small_shapes_against_oracle demands:
    objectives to 1e-8, every inner count equal, factors to 1e-7 of their scale."""
    c = reference(oracle, r, 2)
    if r not in _TRAIN:
        _TRAIN[r] = oracle.train(c.X, c.U, c.V, c.lam, 2, solver=2, do_predict=0)
    Uo, Vo, recs = _TRAIN[r]
    with pcr.tuned(**variant):
        s = pcr.Solver(c.ds, pcr.Parameter(k=r, precision=pcr.PCR_F64, **{"lambda": c.lam}))
    try:
        s.set_factors(c.U, c.V)
        got = s.iterate(2)
        Ug, Vg = s.get_factors()
    finally:
        s.close()
    tag = f"variant {vid(variant)}, r = {r}"
    for g, o in zip(got, recs[1:]):
        assert abs(g["obj"] - o["obj"]) <= 1e-8 * max(abs(o["obj"]), 1.0), (tag, g["obj"], o["obj"])
        assert (g["cg_v"], g["ls_v"], g["cg_u"], g["ls_u"]) == (o["cg_v"], o["ls_v"], o["cg_u"], o["ls_u"]), (tag, g, o)
    scale = max(np.abs(Uo).max(), np.abs(Vo).max(), 1e-3)
    assert np.abs(Ug - Uo).max() < 1e-7 * scale and np.abs(Vg - Vo).max() < 1e-7 * scale, tag
