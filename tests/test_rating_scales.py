"""Exact parity across rating scales and level counts.

The number of distinct rating levels per user selects the code path of training: on the host the route of pcr_build_levels
(64-bit presence mask / insertion into at most 64 keys / sort + unique / refusal above 65535), in the sweeps the window cache
(ws = max_levels - 1 slots per rating for a shard maximum of 2..9 levels, the unrolled sweep_coeff_win4 / sweep_out4 at exactly
ws = 4, the generic sweep_coeff_win for the other counts, searching sweeps from 10 levels on), in the class layout every LDS size
(rs_cap = levels + 2) and the Gram cut (> 64 levels).  Every other exact test runs integers 1..5.  This file runs the dyadic
exact-parity method of tests/test_exact_parity.py over the scales of tests/scale_data.py:

    scale      values                        levels (++ / PrimalCR)   what it reaches
    five       1..5                          5 / 5      the control cell: ws = 4, the unrolled path
    one        all 3                         1 / 1      no comparable pair, ws = 0, g = lambda V exactly
    binary     {0, 1}                        2 / 2      ws = 1, a rating of 0
    three      {1, 3, 5}                     3 / 3      ws = 2, gaps in the mask
    four       1..4                          4 / 4      ws = 3, just below the unrolled path
    six        1..6                          6 / 6      ws = 5, just above it
    nine       1..9                          9 / 9      ws = 8, the last cached count
    ten        1..10                         10 / 10    the first searching count
    halfstar   0.5..5.0 by 0.5               5 / 10     ++: the half-away rule decides the level; PrimalCR: non-integer, insertion route
    signed     -2.5..2.5 by 0.5              7 / 11     negative halves (-0.5 -> -1, -1.5 -> -2)
    jester     integers -10..10              21 / 21    a negative mask base
    l64, l65   1..64, 1..65                  64, 65     the last bit of the mask route / the first set off it (sort route), Gram cut
    wide6      {0, 20, .., 100}              6 / 6      a range >= 64: insertion route with ws = 5
    percent    0..100                        101 / 101  sort route, searching sweeps, no Gram class
    mixed      by user index mod 4: one, binary, five, nine    9 / 9   shard ws = 8 with users of 1, 2, 5 and 9 levels side by side

Which form ran: the profile slots name the U step's class form (gram, g = global scratch) and those are asserted; the window form
(ws, win4 or generic, searching) has no slot of its own -- there the evidence is the level count checked on the CPU (part 1) and
the ws the host-only class layout prints for it (test_window_slots_of_the_class_layout).
"""
import re

import numpy as np
import pytest

import exact_data as ed
import item_edge_data as ie
import primalcr_amd as pcr
import scale_data as sd
from test_exact_parity import PREC, assert_same, check_first_order, is_f32, vid, where_item, where_m
from test_gpu_parity import TOL, _oracle_update_U_solver1

R = 12
VARIANTS = [{}, {"ustep_mode": 2}, {"ustep_mode": 1}, {"window_cache": 0}, {"win16": 0, "ustep_win_lds": 0}, {"ustep_win_lds": 0},
            {"lanes": 1}, {"cluster_k": 1}, {"vblock_users": 8}, {"allreduce_chunks": 4, "sddmm_csc": 1}]
GRAM = {"ustep_gram": 64}
RANK_SCALES = ("four", "nine", "ten", "percent", "mixed")       # the scales that also run at r = 1, 100, 132
OTHER_RANKS = (1, 100, 132)
RANK_VARIANTS = [{}, {"ustep_mode": 2}]
TWO_LEVELS = tuple(s for s in sd.ALL_SCALES if s != "one")
# the shard cells: (shards, scale of the shards after the first); the first shard's users rate 1..5
SPLITS = tuple((n, later) for later in ("ten", "nine") for n in (2, 3))
SPLIT_CELLS = ((2, 12), (2, 100), (1, 12))                       # (solver, r) of the shard cells


def split_name(n, later):
    return f"split{n}-{later}"


def variants_of(scale):
    return VARIANTS + ([GRAM] if scale in ("l64", "l65") else [])


_REF = {}


def reference(oracle, scale, solver, r=R):
    """The case of a scale and the oracle's m, objective, g and Ha for both probes (cached: the oracle runs once per case)."""
    key = (scale, solver, r)
    if key not in _REF:
        val = None
        if scale.startswith("split"):
            n, later = scale[5:].split("-")
            bounds = pcr.partition_users(sd.structure()[1], int(n))
            val = sd.split_values(bounds, later)
        c = sd.scale_case(scale, solver, r, val)
        if val is not None:
            c.bounds = bounds
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


def reordered(c, seed):
    """The case's CSR with every user's ratings listed in another (seeded) order, and the permutation."""
    from oracle.oracle_py import CSR
    rng = np.random.default_rng(seed)
    q = np.concatenate([c.X.idx[u] + rng.permutation(int(n)) for u, n in enumerate(c.lens)]).astype(np.int64)
    return CSR(c.d1, c.d2, c.X.idx, c.X.item[q], c.X.val[q]), q


# ------------------------------------------------------------------------------------------------------------------------------
# 1 + 2. the precondition and the oracle against the definition, on the CPU
# ------------------------------------------------------------------------------------------------------------------------------

CPU_CELLS = ([(sc, s, R) for sc in sd.ALL_SCALES for s in (2, 1)] + [(sc, s, r) for sc in RANK_SCALES for s in (2, 1) for r in OTHER_RANKS] +
             [(split_name(n, later), s, r) for n, later in SPLITS for s, r in SPLIT_CELLS])


def max_levels_of(scale, solver):
    return sd.MAX_LEVELS[scale[scale.index("-") + 1:] if scale.startswith("split") else scale][0 if solver == 2 else 1]


@pytest.mark.parametrize("scale,solver,r", CPU_CELLS, ids=[f"{sc}-s{s}-r{r}" for sc, s, r in CPU_CELLS])
def test_preconditions_and_integer_brute_force_on_every_scale(oracle, scale, solver, r):
    """Every (scale, solver, r) the GPU part runs, with the oracle alone: m, g, Ha, Ha2 are their own float32 round trip and whole
    quarter units with max |.| * 4 < 2^22; the objective is a whole number of sixteenths below 2^50; the per-user level counts,
    in numpy, are the table's (the shard maximum exactly; every user of 1024 ratings or more holds every level of its scale up to
    21, and the user of 5000 ratings all of them; for `mixed` users of 1, 2, 5 and 9 levels stand side by side, for the split
    cells the first shard stays at 5); shuffling the triplets and listing every user's ratings in another order changes no bit.
    Then the oracle against the definition in integers with scale_data.levels_of (half away from zero for PrimalCR++, which holds
    the oracle's lround to that rule on halfstar and signed): objective and g through exact_data.brute_force, and at r = 12 Ha for
    both probes through item_edge_data.brute_force_Ha (the level partition does not depend on r; the rank classes of Ha are held
    by tests/test_item_edges.py).  Both sides of the hinge are populated for every scale with two levels or more."""
    c = reference(oracle, scale, solver, r)
    X = c.X
    assert set(ed.CLASS_EDGES) <= set(c.lens.tolist()) and c.lens.max() == 5000 and c.d1 == 65 and 24000 < X.nnz < 28000
    assert c.lam == 32.0 and set(np.unique(np.abs(np.concatenate([c.U.ravel(), c.V.ravel(), c.a.ravel(), c.a2.ravel()])))) <= {0.0, 0.5, 1.0}
    for name, x in (("m", c.m), ("g", c.g), ("Ha", c.Ha), ("Ha2", c.Ha2)):
        assert is_f32(x), name
        assert np.array_equal(x * ed.UNIT, np.rint(x * ed.UNIT)), name
        assert np.abs(x).max() * ed.UNIT < 2 ** 22, (name, np.abs(x).max())
    assert c.obj * 16 == np.rint(c.obj * 16) and c.obj * 16 < 2 ** 50
    # level counts
    cnt = sd.level_counts(X.idx, X.val, solver)
    top = max_levels_of(scale, solver)
    assert cnt.max() == top, (cnt.max(), top)
    if scale == "mixed":
        per_user = np.array([sd.MAX_LEVELS[sd.MIXED[u % 4]][0] for u in range(c.d1)])
        assert (cnt <= per_user).all() and np.array_equal(cnt[c.lens >= 128], per_user[c.lens >= 128])
        assert {1, 2, 5, 9} <= set(cnt[c.lens >= 128].tolist())
        assert cnt[c.lens == 2049] == 1 and cnt[c.lens == 4096] == 2 and cnt[c.lens == 4097] == 5 and cnt[c.lens == 200].max(initial=9) == 9
    elif scale.startswith("split"):
        first = np.arange(c.d1) < c.bounds[1]
        assert 0 < c.bounds[1] < c.d1 and cnt[first].max() == 5 and cnt[~first].max() == top
        assert (np.diff(c.bounds) > 0).all() and c.lens[first].max() >= 1024 and c.lens[~first].min() < 64
    else:
        assert (cnt[c.lens >= 1024] == top).all() if top <= 21 else cnt[c.lens == 5000] == top
    # order independence
    rng = np.random.default_rng(r + solver)
    p = rng.permutation(len(c.user))
    Xs = oracle.build_csr(c.d1, c.d2, c.user[p], c.item[p], c.val[p])
    assert np.array_equal(Xs.idx, X.idx) and np.array_equal(Xs.item, X.item) and np.array_equal(Xs.val, X.val)
    Xq, q = reordered(c, 7 * r + solver)
    mq = oracle.comp_m(c.U, c.V, Xq)
    assert np.array_equal(mq, c.m[q])
    assert oracle.objective_new(mq, c.U, c.V, Xq, c.lam, solver=solver) == c.obj
    assert np.array_equal(oracle.obtain_g_new(c.U, c.V, Xq, mq, c.lam, solver=solver), c.g)
    assert np.array_equal(oracle.compute_Ha_new(c.a, mq, c.U, Xq, c.lam, solver=solver), c.Ha)
    # the definition, in integers
    lev = sd.levels_of(X.val, solver)
    obj16, g4, m4, active, comparable = ed.brute_force(c, X.idx, X.item, X.val, levels=lev)
    assert np.array_equal(c.m * ed.UNIT, m4)
    assert c.obj * 16 == obj16, (c.obj * 16, obj16)
    assert np.array_equal(c.g * ed.UNIT, g4)
    if r == R:
        assert comparable == int(sd.all_pairs(X.idx, X.val, solver).sum())
    if top == 1:
        assert comparable == 0 and np.array_equal(c.g, c.lam * c.V) and np.array_equal(c.Ha, c.lam * c.a)
    else:
        # pairs inside and outside the hinge, a twentieth of each at least (test_exact_parity's own band is [0.2, 0.95])
        assert 0.05 <= active / comparable <= 0.95, active / comparable
    if r == R:
        assert np.array_equal(c.Ha * ed.UNIT, ie.brute_force_Ha(c, X.idx, X.item, X.val, c.a, levels=lev))
        if not scale.startswith("split"):                                     # (the shard cells run the first probe only)
            assert np.array_equal(c.Ha2 * ed.UNIT, ie.brute_force_Ha(c, X.idx, X.item, X.val, c.a2, levels=lev))


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the host level builder
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scale", sd.ALL_SCALES)
def test_user_pairs_equal_the_all_pairs_count(oracle, scale):
    """Dataset.user_pairs (pcr_build_levels through the mask, insertion and sort routes) == the all-pairs count in numpy under
    scale_data.levels_of, for both solver types; its sum is count_pairs, and the oracle's own count."""
    c = reference(oracle, scale, 2)
    for solver in (2, 1):
        want = sd.all_pairs(c.X.idx, c.X.val, solver)
        got = c.ds.user_pairs(solver)
        assert np.array_equal(got, want), (scale, solver, np.flatnonzero(got != want)[:8])
        assert int(got.sum()) == c.ds.count_pairs(solver) == oracle.count_pairs(c.X, raw=solver == 1)


HALVES = [0.49999999999999994, 0.5, -0.5, -0.0, 1.5, 2.5, -2.5, 2.5000000000000004]


def test_half_away_rule_on_a_hand_made_row(oracle):
    """The doubles where a rounding rule can go wrong: the largest double below a half (v + .5 rounds up to 1 in binary64; lround
    gives 0), the halves of both signs, a negative zero, 2.5 (to even it would be 2) and its successor.  scale_data.levels_of
    against the rule in rational arithmetic; then the host builder: the whole row as one user, and every value beside the
    integer it must share a level with (no pair) and beside that integer's neighbour (one pair)."""
    want = [0, 1, -1, 0, 2, 3, -3, 3]
    assert [sd.half_away_exact(v) for v in HALVES] == want
    assert sd.levels_of(np.array(HALVES), 2).tolist() == want
    assert np.array_equal(sd.levels_of(np.array(HALVES), 1), np.array(HALVES))
    rows = [HALVES] + [[v, float(k)] for v, k in zip(HALVES, want)] + [[v, float(k) + (1.0 if v >= 0 else -1.0)] for v, k in zip(HALVES, want)]
    lens = np.array([len(x) for x in rows])
    user = np.repeat(np.arange(len(rows)), lens)
    item = np.concatenate([np.arange(n) for n in lens])
    val = np.concatenate(rows)
    ds = pcr.Dataset.from_triplets(len(rows), 8, user, item, val)
    idx = np.concatenate([[0], np.cumsum(lens)])
    pp = ds.user_pairs(2)
    assert pp.tolist() == [26] + [0] * 8 + [1] * 8
    assert np.array_equal(pp, sd.all_pairs(idx, val, 2))
    raw = ds.user_pairs(1)
    assert np.array_equal(raw, sd.all_pairs(idx, val, 1))
    assert raw.tolist() == [28] + [1, 1, 1, 0, 1, 1, 1, 1] + [1] * 8                   # raw doubles: only -0.0 == 0.0 ties
    X = oracle.build_csr(len(rows), 8, user, item, val)
    assert oracle.count_pairs(X) == int(pp.sum()) and oracle.count_pairs(X, raw=True) == int(raw.sum())


def test_level_count_limit():
    """A PrimalCR user of 65535 distinct ratings is accepted (pairs = n (n - 1) / 2); one of 65536 is refused with
    PCR_ERR_UNSUPPORTED (-7) -- count_pairs reports -1, user_pairs raises -- and the message names the user.  PrimalCR++ on the
    same integers refuses too (the sort route: the range is beyond the mask)."""
    for n, ok in ((65535, True), (65536, False)):
        lens = np.array([3, 0, n, 2])
        user = np.repeat(np.arange(4), lens)
        item = np.concatenate([np.arange(k) for k in lens])
        val = np.concatenate([[1.0, 2.0, 2.0], np.random.default_rng(n).permutation(n) * 0.25, [5.0, 4.0]])
        ds = pcr.Dataset.from_triplets(4, n, user, item, val)
        if ok:
            assert ds.user_pairs(1).tolist() == [2, 0, n * (n - 1) // 2, 1] and ds.count_pairs(1) == 3 + n * (n - 1) // 2
            m = np.unique(sd.levels_of(val[3:3 + n], 2)).size                    # PrimalCR++ on the quarter steps: far fewer levels
            assert m < 65535 and ds.count_pairs(2) > 0
        else:
            assert ds.count_pairs(1) == -1
            with pytest.raises(pcr.PcrError, match=r"error -7: .*user 2 has more than 65535 distinct rating levels"):
                ds.user_pairs(1)
            ints = pcr.Dataset.from_triplets(4, n, user, item, np.concatenate([[1.0, 2.0, 2.0], np.arange(n, dtype=np.float64), [5.0, 4.0]]))
            assert ints.count_pairs(2) == -1
            with pytest.raises(pcr.PcrError, match=r"error -7: .*user 2 "):
                ints.user_pairs(2)


def test_window_slots_of_the_class_layout(oracle, tmp_path):
    """What the shard's level count makes of the class layout, from the host-only layout function (csrc/check/classes_dump) fed
    with the fixture's lengths and the numpy level counts: ws = levels - 1 for 2..9 levels and 0 otherwise (1 level, 10 and more)
    or with the window cache off; every class's max_lev is the largest count among its users, so that in `mixed` a class of long
    users sits below the shard's 9; ustep_gram = 64 gives l64 a Gram class and l65 none."""
    import classes_data as cd
    exe = cd.build_dump()

    def dump(cnt, lens, prec, knobs):
        path = tmp_path / "case.txt"
        head = [f"precision={prec}", f"ld={R}", "ncu=256", f"users={len(lens)}"] + [f"{k}={v}" for k, v in knobs.items()]
        path.write_text(" ".join(head) + "\n" + "".join(f"{int(n)} {int(t)}\n" for n, t in zip(lens, cnt)))
        import subprocess
        p = subprocess.run([exe, str(path)], capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
        classes = [dict([x.split("=") for x in line.split()[2:]], name=line.split()[1]) for line in p.stdout.splitlines() if line.startswith("class ")]
        ws = int(re.search(r"\bws=(\d+)", p.stdout).group(1))
        return classes, ws

    for scale in sd.ALL_SCALES:
        for solver in (2, 1):
            c = reference(oracle, scale, solver)
            cnt = sd.level_counts(c.X.idx, c.X.val, solver)
            top = sd.MAX_LEVELS[scale][0 if solver == 2 else 1]
            for prec in ("f32", "f64"):
                classes, ws = dump(cnt, c.lens, prec, {})
                assert ws == sd.window_slots(top) == (top - 1 if top in (2, 3, 4, 5, 6, 7, 8, 9) else 0), (scale, solver, prec, ws)
                assert max(int(x["max_lev"]) for x in classes) == top
                assert dump(cnt, c.lens, prec, {"window_cache": 0})[1] == 0
                if scale == "mixed":
                    assert min(int(x["max_lev"]) for x in classes if int(x["users"]) > 0) < 9
                if scale in ("l64", "l65"):
                    gram = [x for x in dump(cnt, c.lens, prec, GRAM)[0] if int(x["gram"]) and int(x["users"]) > 0]
                    assert bool(gram) == (scale == "l64"), (scale, solver, prec)


# ------------------------------------------------------------------------------------------------------------------------------
# 4. the decisions of the first U step are stable under re-ordering
# ------------------------------------------------------------------------------------------------------------------------------

_USTEP = {}


def oracle_u_step(oracle, c, X=None, m=None):
    """The oracle's first U step from the dyadic start: (U, objective, {cg, ls})."""
    X = c.X if X is None else X
    m = c.m if m is None else m
    if c.solver == 2:
        return oracle.update_U_new(X, m, c.lam, 1.0, c.V, c.U)
    return _oracle_update_U_solver1(oracle, X, m, c.lam, c.V, c.U)


def first_u_step(oracle, scale, solver):
    key = (scale, solver)
    if key not in _USTEP:
        _USTEP[key] = oracle_u_step(oracle, reference(oracle, scale, solver))
    return _USTEP[key]


@pytest.mark.parametrize("solver", [2, 1])
@pytest.mark.parametrize("scale", TWO_LEVELS)
def test_first_u_step_decisions_do_not_depend_on_the_order(oracle, scale, solver):
    """The per-user comparison of part 2 on the GPU counts CG iterations and line-search tries; a user whose CG stops within
    rounding of its tolerance, or whose line search accepts within rounding, would make those counts a property of the summation
    order.  Here, on the CPU: the oracle's first U step on three seeded re-orderings of every user's ratings gives the same CG and
    line-search totals and rows within 1e-10 of the row maximum.  (A scale or seed that fails this is re-seeded in
    scale_data.rating_values; the GPU bound is never widened instead.)"""
    c = reference(oracle, scale, solver)
    U0, _, info0 = first_u_step(oracle, scale, solver)
    assert info0["cg"] > 0 and info0["ls"] > 0
    for seed in (1, 2, 3):
        Xq, q = reordered(c, 1000 * seed + solver)
        Uq, _, info = oracle_u_step(oracle, c, Xq, c.m[q])
        assert (info["cg"], info["ls"]) == (info0["cg"], info0["ls"]), (scale, solver, seed, info, info0)
        d = np.abs(Uq - U0).max(1) / np.maximum(np.abs(U0).max(1), 1e-3 * np.abs(U0).max())
        assert d.max() <= 1e-10, (scale, solver, seed, int(d.argmax()), d.max())


# ------------------------------------------------------------------------------------------------------------------------------
# GPU 1. the first-order entry points, bit for bit
# ------------------------------------------------------------------------------------------------------------------------------

FAILED = (AssertionError, pytest.fail.Exception)


def run_first_order(c, pname, variants, what):
    failures = []
    for v in variants:
        with pcr.tuned(**v):
            s = pcr.Solver(c.ds, pcr.Parameter(k=c.r, solver_type=c.solver, precision=PREC[pname], **{"lambda": c.lam}))
        try:
            s.set_factors(c.U, c.V)
            check_first_order(s, c, f"scale {what}, variant {vid(v)}, {pname}, solver {c.solver}, r = {c.r}")
        except FAILED as e:
            failures.append(str(e))
        finally:
            s.close()
    assert not failures, "\n".join(failures)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", sd.ALL_SCALES)
@pytest.mark.parametrize("solver", [2, 1])
@pytest.mark.parametrize("pname", ["F32", "F64"])
def test_first_order_entry_points_are_exact_on_every_scale(oracle, pname, solver, scale):
    """comp_m, objective, obtain_g, compute_Ha on both probes, then obtain_g and objective again, equal the oracle bit for bit at
    r = 12 on every scale, in both precisions and for both solvers, under: the default, ustep_mode 2 and 1, window_cache = 0,
    32-bit window rows from global memory, ustep_win_lds = 0 alone, one stream, no clusters, the blocked-user V step, item ranges
    over the CSC plan; l64 and l65 also under ustep_gram = 64.  A failure names the scale, the variant, the first differing
    (user or item, column) and the users' length classes, and reads against the `five` cell.  (The window form that ran is not
    named by a profile slot: the level counts of part 1 and test_window_slots_of_the_class_layout are the evidence.)"""
    run_first_order(reference(oracle, scale, solver), pname, variants_of(scale), scale)


@pytest.mark.gpu
@pytest.mark.parametrize("r", OTHER_RANKS)
@pytest.mark.parametrize("scale", RANK_SCALES)
@pytest.mark.parametrize("solver", [2, 1])
@pytest.mark.parametrize("pname", ["F32", "F64"])
def test_first_order_entry_points_are_exact_at_other_ranks(oracle, pname, solver, scale, r):
    """The same at r = 1, 100 and 132 (one chunk, the headline rank, beyond 128) for four, nine, ten, percent and mixed, under the
    default and the throughput forms."""
    run_first_order(reference(oracle, scale, solver, r), pname, RANK_VARIANTS, scale)


# ------------------------------------------------------------------------------------------------------------------------------
# GPU 2. the first U step, per user
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("scale", TWO_LEVELS)
@pytest.mark.parametrize("solver", [2, 1])
@pytest.mark.parametrize("pname", ["F32", "F64"])
def test_first_u_step_per_user_on_every_scale(oracle, pname, solver, scale):
    """set_factors; comp_m(); update_U() from the dyadic start, every user's row against the oracle's U step (PrimalCR through
    its per-user entry point) under the variant list of part 1, by the method and bound of
    test_first_u_step_per_user_under_every_variant:
        max |dU[u]| <= TOL[precision]["fac"] * max(|U_o[u]|_inf, 1e-3 |U_o|_inf)
    fp64: the CG and line-search totals equal the oracle's (their stability is checked on the CPU, part 4).  The profile slots
    name the class forms, and these are asserted: every class the solver laid out ran once; without clusters the users beyond
    4096 ratings run a global-scratch class (.../512g..); under ustep_gram = 64 a ustep/gram* class runs for l64 and none for l65.
    The largest ratio to the bound is printed (NOTES.md records it)."""
    c = reference(oracle, scale, solver)
    Uo, _, iu = first_u_step(oracle, scale, solver)
    fac = TOL[PREC[pname]]["fac"]
    bound = fac * np.maximum(np.abs(Uo).max(1), 1e-3 * np.abs(Uo).max())
    failures, worst = [], (0.0, None)
    for v in variants_of(scale):
        tag = f"scale {scale}, variant {vid(v)}, {pname}, solver {solver}"
        with pcr.tuned(**v):
            s = pcr.Solver(c.ds, pcr.Parameter(k=R, solver_type=solver, precision=PREC[pname], **{"lambda": c.lam}))
        s.profile(True)
        s.set_factors(c.U, c.V)
        s.comp_m()
        _, info = s.update_U()
        Ug, _ = s.get_factors()
        classes = s.ustep_classes()
        ran = {n: s.profile_launches(n) for n in classes}
        s.close()
        if set(ran.values()) != {1}:
            failures.append(f"{tag}: launches per class {ran}")
        if v == {"cluster_k": 1} and not any(re.match(r"ustep/512g", n) for n in classes):
            failures.append(f"{tag}: no global-scratch class among {classes}")
        if v == GRAM and any(n.startswith("ustep/gram") for n in classes) != (scale == "l64"):
            failures.append(f"{tag}: classes {classes}")
        ratio = np.abs(Ug - Uo).max(1) / bound
        u = int(ratio.argmax())
        if ratio[u] > worst[0]:
            worst = (float(ratio[u]), f"{vid(v)}: user {u}, {ed.class_of(int(c.lens[u]))}")
        if not ratio[u] <= 1.0:
            failures.append(f"{tag}: {int((ratio > 1).sum())} users beyond the bound; worst user {u}, {ed.class_of(int(c.lens[u]))}: "
                            f"max |dU| = {np.abs(Ug[u] - Uo[u]).max():.3e}, bound {bound[u]:.3e}")
        if pname == "F64" and (info["cg"], info["ls"]) != (iu["cg"], iu["ls"]):
            failures.append(f"{tag}: inner counts {info} against the oracle's {iu}")
    print(f"[rating-scales] first U step {scale} {pname} solver {solver}: largest per-row |dU| / bound = {worst[0]:.3e} ({worst[1]})")
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------------------------------------
# GPU 3. shards under different window forms
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("pname", ["F64", "F32"])
@pytest.mark.parametrize("nranks,later", SPLITS, ids=[split_name(n, later) for n, later in SPLITS])
def test_shards_under_different_window_forms_add_up_exactly(oracle, nranks, later, pname):
    """Local-only shards as in test_user_shards_add_up_exactly, with the scale chosen by shard: partition_users on the fixture's
    idx first, then the users of shard 0 rate 1..5 (ws = 4, the unrolled path) and the later shards 1..10 (searching sweeps; the
    one-rank solver then searches everywhere) or 1..9 (ws = 8 there and in the one-rank solver).  The concatenated m, the summed g
    and Ha and the objective equal the one-rank result and the oracle exactly.  (The level counts per shard are checked on the
    CPU, part 1; no profile slot names the window form.)"""
    for solver, r in SPLIT_CELLS:
        c = reference(oracle, split_name(nranks, later), solver, r)
        tag = f"{nranks} shards (1..5 | {later}), {pname}, solver {solver}, r = {r}"
        par = dict(k=r, solver_type=solver, precision=PREC[pname], **{"lambda": c.lam})
        m_parts, g_sum, Ha_sum, obj_sum = [], 0.0, 0.0, 0.0
        for q in range(nranks):
            s = pcr.Solver(c.ds, pcr.Parameter(**par), rank=q, nranks=nranks)
            assert (s.first_user, s.n_users) == (c.bounds[q], c.bounds[q + 1] - c.bounds[q])
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
        obj_sum -= (nranks - 1) * c.lam / 2.0 * float((c.V ** 2).sum())          # the replicated lambda/2 |V|^2, counted once
        assert_same(tag, "concatenated m", np.concatenate(m_parts), m_full, c, where_m)
        assert_same(tag, "sum of shard g (against one rank)", g_sum, g_full, c, where_item)
        assert_same(tag, "sum of shard Ha (against one rank)", Ha_sum, Ha_full, c, where_item)
        assert obj_sum == obj_full, (tag, obj_sum, obj_full)
        assert_same(tag, "concatenated m (oracle)", np.concatenate(m_parts), c.m, c, where_m)
        assert_same(tag, "sum of shard g", g_sum, c.g, c, where_item)
        assert_same(tag, "sum of shard Ha", Ha_sum, c.Ha, c, where_item)
        assert obj_sum == c.obj, (tag, obj_sum, c.obj)


# ------------------------------------------------------------------------------------------------------------------------------
# GPU 4. the pre-rounded twin
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("scale", ["halfstar", "signed"])
@pytest.mark.parametrize("pname", ["F64", "F32"])
def test_prerounded_twin_is_bit_identical(oracle, pname, scale):
    """PrimalCR++ sees a rating only through its level: a solver on the half-step ratings and one on the same triplets rounded half
    away from zero on the host (scale_data.levels_of) return the same bits -- objective, obtain_g, compute_Ha, then two iterate
    steps (U, V, objectives, inner counts)."""
    c = reference(oracle, scale, 2)
    twin_val = sd.levels_of(c.val, 2).astype(np.float64)
    assert not np.array_equal(twin_val, c.val)
    out = []
    for val in (c.val, twin_val):
        ds = pcr.Dataset.from_triplets(c.d1, c.d2, c.user, c.item, val)
        s = pcr.Solver(ds, pcr.Parameter(k=R, solver_type=2, precision=PREC[pname], **{"lambda": c.lam}))
        s.set_factors(c.U, c.V)
        s.comp_m()
        first = (s.objective(), s.obtain_g(), s.compute_Ha(c.a))
        recs = [{k: x[k] for k in ("obj", "cg_v", "ls_v", "cg_u", "ls_u")} for x in s.iterate(2)]
        out.append(first + (recs,) + s.get_factors())
        s.close()
    a, b = out
    assert a[0] == b[0] == c.obj and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert np.array_equal(a[1], c.g) and np.array_equal(a[2], c.Ha)
    assert a[3] == b[3], (a[3], b[3])
    assert np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5])


@pytest.mark.gpu
@pytest.mark.parametrize("scale", ["halfstar", "signed"])
@pytest.mark.parametrize("pname", ["F64", "F32"])
def test_prerounded_twin_fold_in_is_bit_identical(oracle, pname, scale):
    """The same for fold_in(steps = 2): a handful of new users with half-step ratings against their pre-rounded twins, rows and
    per-user tables bitwise."""
    c = reference(oracle, scale, 2)
    rng = np.random.default_rng(5 + len(scale))
    lens = np.array([2, 7, 33, 64, 65, 300, 1100])
    idx = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    item = np.concatenate([np.sort(rng.choice(c.d2, int(n), replace=False)) for n in lens]).astype(np.int32)
    pool = sd.SCALES[scale]
    val = pool[rng.integers(0, len(pool), item.shape[0])]
    twin = sd.levels_of(val, 2).astype(np.float64)
    assert not np.array_equal(twin, val)
    U0 = ed.dyadic_matrix(rng, len(lens), R, 1.0)
    res = [pcr.fold_in(c.V, (idx, item, v), c.lam, solver_type=2, U0=U0, steps=2, dtype=PREC[pname], per_user=True) for v in (val, twin)]
    (Ua, sa, pa), (Ub, sb, pb) = res
    assert np.array_equal(Ua, Ub) and sa == sb and np.array_equal(pa, pb, equal_nan=True)
    assert not np.array_equal(Ua, U0)


# ------------------------------------------------------------------------------------------------------------------------------
# GPU 5. the trajectory
# ------------------------------------------------------------------------------------------------------------------------------

_TRAJ = {}


def trajectory(oracle, scale, solver):
    key = (scale, solver)
    if key not in _TRAJ:
        c = reference(oracle, scale, solver)
        U0 = oracle.initial(c.d1, R) * 0.3; V0 = oracle.initial(c.d2, R) * 0.3
        Uo, Vo, recs = oracle.train(c.X, U0, V0, 25.0, 2, solver=solver, do_predict=0)
        _TRAJ[key] = (U0, V0, Uo, Vo, recs[1:])
    return _TRAJ[key]


@pytest.mark.gpu
@pytest.mark.parametrize("scale", sd.ALL_SCALES)
@pytest.mark.parametrize("solver", [2, 1])
@pytest.mark.parametrize("pname", ["F32", "F64"])
def test_two_iterations_follow_the_oracle_on_every_scale(oracle, pname, solver, scale):
    """Two outer iterations from oracle.initial * 0.3 at lambda = 25 against oracle.train, under the default and ustep_mode = 2.
    fp64 by the numbers of test_fuzz_small_shapes_against_oracle: objective 1e-8 relative, the four inner counts equal, factors
    within 1e-7 of the scale; fp32 by those of test_two_fp32_iterations_under_every_variant: objective 1e-3 relative, cg_v equal."""
    c = reference(oracle, scale, solver)
    U0, V0, Uo, Vo, recs = trajectory(oracle, scale, solver)
    failures = []
    for v in RANK_VARIANTS:
        tag = f"scale {scale}, variant {vid(v)}, {pname}, solver {solver}"
        with pcr.tuned(**v):
            s = pcr.Solver(c.ds, pcr.Parameter(k=R, solver_type=solver, precision=PREC[pname], **{"lambda": 25.0}))
        s.set_factors(U0, V0)
        got = s.iterate(2)
        Ug, Vg = s.get_factors()
        s.close()
        for g, o in zip(got, recs):
            if pname == "F64":
                if not abs(g["obj"] - o["obj"]) <= 1e-8 * max(abs(o["obj"]), 1.0):
                    failures.append(f"{tag}: objective {g['obj']!r} against {o['obj']!r}")
                if (g["cg_v"], g["ls_v"], g["cg_u"], g["ls_u"]) != (o["cg_v"], o["ls_v"], o["cg_u"], o["ls_u"]):
                    failures.append(f"{tag}: inner counts {g} against {o}")
            else:
                if not abs(g["obj"] / o["obj"] - 1) < 1e-3:
                    failures.append(f"{tag}: objective {g['obj']!r} against {o['obj']!r}")
                if g["cg_v"] != o["cg_v"]:
                    failures.append(f"{tag}: cg_v {g['cg_v']} against {o['cg_v']}")
        if pname == "F64":
            scale_ = max(np.abs(Uo).max(), np.abs(Vo).max(), 1e-3)
            if not (np.abs(Ug - Uo).max() < 1e-7 * scale_ and np.abs(Vg - Vo).max() < 1e-7 * scale_):
                failures.append(f"{tag}: factors off by {np.abs(Ug - Uo).max():.3e} (U), {np.abs(Vg - Vo).max():.3e} (V) at scale {scale_:.3e}")
    assert not failures, "\n".join(failures)
