"""The exact-Newton U step (pcr_tune("ustep_newton"), k_unewton in primalcr_amd/csrc/pcr_newton.h) held to a plain per-user
reference at every edge of its code.

The fixture (tests/newton_data.py) has a user at every length at which the kernel changes its path, dyadic factors (H, g, the scores
and every window are exact in fp32 and in fp64 in any summation order; pairs exactly on the hinge boundary are frequent) and ratings
from scales of 1, 2, 5, 6, 9, 10 and 21 levels, a mix of them, and real values.  The reference (tests/newton_ref.py) is the definition
in numpy fp64 over all pairs: no sort, no window, no prefix sum.

Paths of k_unewton and the cells that reach them (test_every_listed_path_is_reached proves the table on the CPU):
    levels 6..9 (the unprefetched slots 4..7)      six / nine / mixed at rank 12 (fp64, kept); six / nine at rank 100 in fp32 (kept)
    the 9 | 10 cut, Bnd's min(rs_cap, 10) rows     nine (rs_cap 11: the last kept count), ten (searched; a user with 9 of the 10 levels is
                                                   kept inside rs_cap 12), mixed (9-level users beside 1-, 2- and 5-level ones)
    wbcap = 0 with few levels                      every scale of at most 9 levels at rank 100 in fp64 on the FULL shard (the 80 KiB cut);
                                                   the short shard at rank 100 keeps its bounds
    nt = 1, 3, 4, 5, 7                             ranks 1 / 12 / 16, 48, 64, 65 / 80, 100 (pad) / 112 (no pad); 17 is nt = 2
    n < 8, the chunk, the block, NEWTON_MAX_N      the users of 1, 2, 3, 7 | 15, 16, 17 | 255, 256, 257 | 1023, 1024, 1025 ratings
    boundary pairs under both solvers              every cell with a comparable pair: inclusive (PrimalCR++) and strict (PrimalCR)
    a level per rating                             real under PrimalCR: searched windows with up to 1024 levels
    independence of the shard                      test_a_user_does_not_depend_on_its_shard
    the second iteration                           test_two_outer_iterations_under_the_mode
"""
import os
import re

import numpy as np
import pytest

import newton_data as nd
import newton_ref as nr
import primalcr_amd as pcr
import scale_data as sd
from conftest import ROOT
from test_gpu_parity import TOL, rel

FAC64 = TOL[pcr.PCR_F64]["fac"]                      # the project's fp64 factor bound, applied per row (1e-7)
PRE = 1e-2                                           # cond(H) 2^-52 |delta|_inf may use this share of a user's bound
MARGIN = 1e-3                                        # every line-search decision is at least this far (relative) from a tie
# Largest per-user |U_oracle - U_reference| / bound over the anchor cells, measured (NOTES.md): 5.3e-5, times 10.
ANCHOR = 5.3e-4
assert ANCHOR <= 1e-2                                # the anchor stays at least 100 times below the GPU bound

FP64_CELLS = list(dict.fromkeys([("five", 2, r) for r in nd.RANKS] +
                                [(v, s, r) for v in nd.VARIANTS for r in (12, 100) for s in (2, 1)]))
SHORT_CELLS = [("five", 2, 100), ("five", 1, 100), ("nine", 2, 100), ("mixed", 2, 100), ("real", 1, 100)]
FP32_CELLS = [("five", 2, r) for r in (1, 17, 65, 100, 112)] + [(v, 2, 100) for v in ("six", "nine", "ten")]
ANCHOR_CELLS = [(v, s, r) for v in ("five", "nine", "ten", "real") for r in (12, 100) for s in (2, 1)]
SHARD_CELLS = [(v, r) for v in ("five", "nine", "mixed") for r in (12, 100)]


def cid(cell):
    return "-".join(str(x) if i != 1 else f"s{x}" for i, x in enumerate(cell[:2])) + f"-r{cell[2]}"


# ------------------------------------------------------------------------------------------------------------------------------
# the host's geometry, mirrored: which users k_unewton covers, the shard-wide sizes, the 80 KiB cut
# ------------------------------------------------------------------------------------------------------------------------------

def header_constants():
    with open(os.path.join(ROOT, "primalcr_amd", "csrc", "pcr_newton.h")) as f:
        text = f.read()
    k = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define NEWTON_(\w+) (\d+)\s", text, re.M)}
    assert {"MAX_N", "MAX_LD", "CHUNK", "TP"} <= set(k), k
    assert "(size_t)80 * 1024 ? newton_cap : 0" in open(os.path.join(ROOT, "primalcr_amd", "csrc", "pcr_solver.hip")).read()
    return k


def carve(n, elt):
    return (n * elt + 15) & ~15


def newton_bytes(K, elt, cap, rs_cap, ldp, wbcap):
    """newton_bytes<T> of pcr_newton.h (elt = sizeof(T))."""
    build = (carve(cap, elt) + carve(cap + 1, 8) + carve(cap, 2) + carve(cap, 4) + carve(cap, 4) + carve(max(cap, min(rs_cap, 10) * ldp), 8) +
             carve(rs_cap, 4) + carve(wbcap * 8, 2) + 2 * carve(K["CHUNK"] * ldp, 8))
    nt = ldp // 16
    tiles = carve(nt * (nt + 1) // 2 * 16 * K["TP"], 8)
    return carve(8, 8) + 3 * carve(ldp, 8) + max(build, tiles)


class Geo:
    pass


def geometry(c, nlev, elt):
    """What setup_newton / launch_ustep (pcr_solver.hip) derive from the shard: the covered users, newton_cap, newton_rs, wbcap."""
    K = header_constants()
    g = Geo()
    g.ld = (c.r + 3) & ~3
    g.ldp = (g.ld + 15) & ~15
    g.nt = g.ldp // 16
    g.covered = (c.lens >= 1) & (c.lens <= K["MAX_N"]) & (g.ld <= K["MAX_LD"])
    g.cap = int(c.lens[g.covered].max()) if g.covered.any() else 0
    g.rs_cap = int(nlev.max()) + 2
    g.bytes_with_bounds = newton_bytes(K, elt, g.cap, g.rs_cap, g.ldp, g.cap)
    g.wbcap = g.cap if g.bytes_with_bounds <= 80 * 1024 else 0
    g.kept = g.covered & (g.wbcap > 0) & (nlev <= 9)               # (one level: kept, with no slot)
    return g


def path_of(g, u, nlev):
    if not g.covered[u]:
        return "not covered: converged CG"
    return f"{'kept' if g.kept[u] else 'searched'} windows, wbcap = {g.wbcap}, rs_cap = {g.rs_cap}, nt = {g.nt}, {nlev[u]} levels"


# ------------------------------------------------------------------------------------------------------------------------------
# the reference, once per cell
# ------------------------------------------------------------------------------------------------------------------------------

_REF = {}


def reference(variant, solver, r):
    """The full shard's case with the reference's step: Uref, info (per user), bound (per user), nlev, lev."""
    key = (variant, solver, r)
    if key not in _REF:
        c = nd.case(variant, solver, r)
        c.lev = sd.levels_of(c.val, solver)
        c.nlev = nd.level_counts(c)
        c.g64 = geometry(c, c.nlev, 8)
        c.Uref, c.info = nr.shard_step(c, c.U, c.V, c.lev, c.g64.covered)
        c.Uref.setflags(write=False)
        c.bound = row_bound(c.Uref)
        _REF[key] = c
    return _REF[key]


def row_bound(Uref):
    """The per-row rule of test_first_u_step_per_user_under_every_variant, in fp64."""
    return FAC64 * np.maximum(np.abs(Uref).max(1), 1e-3 * np.abs(Uref).max())


def short_reference(variant, solver, r):
    """The short sub-shard: its users' reference rows ARE the full shard's (a user's step is a function of its own ratings)."""
    c = reference(variant, solver, r)
    s = nd.short_case(c)
    s.lev = sd.levels_of(s.val, solver)
    s.nlev = c.nlev[s.users]
    s.g64 = geometry(s, s.nlev, 8)
    s.Uref = c.Uref[s.users]
    s.info = [c.info[u] for u in s.users]
    s.bound = c.bound[s.users]                                      # the full shard's floor: the same bound for the same user
    return s


# ------------------------------------------------------------------------------------------------------------------------------
# 1. on the CPU: the reference against the oracle, the fixture's preconditions, the cut, the mutants
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cell", ANCHOR_CELLS, ids=cid)
def test_reference_is_anchored_on_the_oracle(oracle, cell):
    """The oracle's per-user U step with its CG run to convergence (6 r + 50 iterations, 1e-13) is the same Newton step by the
    reference implementation's own route (sorted sweeps for PrimalCR++, the pair list for PrimalCR).  Its rows equal newton_ref's
    within ANCHOR of each user's GPU bound -- measured 5.3e-5 at the worst (nine, PrimalCR, rank 100: an iterative solve against a direct one), times 10,
    and 100 times below the bound the device is held to -- and its line-search counts are the reference's try counts."""
    variant, solver, r = cell
    c = reference(variant, solver, r)
    X = oracle.build_csr(c.d1, c.d2, c.user, c.item, c.val)
    assert np.array_equal(X.idx, c.idx) and np.array_equal(X.item, c.item) and np.array_equal(X.val, c.val)
    m = oracle.comp_m(c.U, c.V, X)
    ratio = np.zeros(c.d1)
    try:
        oracle.set_cg(6 * r + 50, 1e-13)
        for u in range(c.d1):
            row, _, inf = oracle.update_u_new(u, c.V, X, m, c.lam, 1.0, c.U[u], solver=solver)
            ratio[u] = np.abs(row - c.Uref[u]).max() / c.bound[u]
            assert inf["ls"] == c.info[u]["tries"], (cid(cell), u, inf, c.info[u]["tries"])
    finally:
        oracle.set_cg()
    u = int(ratio.argmax())
    print(f"[newton-exact] anchor {cid(cell)}: largest |U_oracle - U_ref| / bound = {ratio[u]:.3e} (user {u})")
    assert ratio[u] <= ANCHOR, f"{cid(cell)}: user {u} ({c.lens[u]} ratings, {c.nlev[u]} levels): |dU| / bound = {ratio[u]:.3e}"


@pytest.mark.parametrize("cell", FP64_CELLS, ids=cid)
def test_fixture_preconditions(cell):
    """Per cell, for EVERY user (none is excluded): the rounding of an fp64 solve, cond(H) 2^-52 |delta|_inf, is at most 1 / 100 of
    the user's bound; every accept / reject decision of the line search is at least 1e-3 relative away from a tie (fp32's objective
    tolerance is 2e-5: no precision can flip one) and every search ends in an accepted try; every length of the list is there; the
    inputs are dyadic; and wherever the cell has a comparable pair and a covered user, a covered user has a pair exactly on the
    hinge boundary."""
    c = reference(*cell)
    assert tuple(c.lens[:len(nd.LENGTHS)]) == nd.LENGTHS and abs(int(c.lens.sum()) - 10000) < 1000 and c.d1 == len(nd.LENGTHS) + nd.N_MORE
    assert set(np.unique(np.abs(np.concatenate([c.U.ravel(), c.V.ravel()])))) <= {0.0, 0.5, 1.0} and c.lam == 32.0
    for u, o in enumerate(c.info):
        where = f"{cid(cell)}: user {u} ({c.lens[u]} ratings, {o['levels']} levels)"
        assert o["levels"] == c.nlev[u], where
        assert o["cond"] * 2.0 ** -52 * np.abs(o["delta"]).max() <= PRE * c.bound[u], where
        assert all(x >= MARGIN for x in o["margins"]), (where, o["margins"])
        assert o["accepted"] or o["tries"] == 0, where
    g = c.g64
    assert g.covered.sum() == (23 + nd.N_MORE if g.ld <= 112 else 0) and not g.covered[0]
    if g.covered.any() and c.nlev.max() > 1:
        assert any(c.info[u]["boundary"] > 0 for u in np.flatnonzero(g.covered)), cid(cell)
        if c.variant != "real" or c.solver == 2:
            assert sum(c.info[u]["boundary"] > 0 for u in np.flatnonzero(g.covered)) >= 20, cid(cell)


def test_every_listed_path_is_reached():
    """The table of this module's docstring, from the mirrored geometry."""
    lens = nd.case("five", 2, 12).lens
    assert {1, 2, 3, 7, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025} <= set(lens.tolist())
    # rank geometry
    nts = {r: geometry(nd.case("five", 2, r), np.array([5]), 8).nt for r in nd.RANKS}
    assert nts == {1: 1, 12: 1, 16: 1, 17: 2, 48: 3, 64: 4, 65: 5, 80: 5, 100: 7, 112: 7, 113: 8}
    assert geometry(nd.case("five", 2, 112), np.array([5]), 8).ld == 112 and not geometry(nd.case("five", 2, 113), np.array([5]), 8).covered.any()
    # level counts among covered users of at least a chunk
    seen = set()
    for v in nd.VARIANTS:
        for s in (2, 1):
            c = reference(v, s, 12)
            big = c.g64.covered & (c.lens >= 16)
            seen |= set(c.nlev[big].tolist())
            if v in ("six", "nine", "mixed"):                       # slots 4..7 under kept bounds, with 6, 9 and mixed 1 / 2 / 5 / 9 levels
                assert c.g64.wbcap > 0 and (c.g64.kept & big & (c.nlev >= 6)).any()
            if v in ("ten", "mixed"):                                # a 9-level user kept inside a shard whose Bnd is capped at 10 rows
                assert c.g64.rs_cap > 10 and (c.g64.kept & big & (c.nlev == 9)).any(), v
            if v == "ten":
                assert (~c.g64.kept & big & (c.nlev == 10)).any()
            if v == "real" and s == 1:
                assert c.nlev.max() == 2049 and c.nlev[c.lens == 1024][0] == 1024 and not c.g64.kept[c.nlev > 9].any()
    assert {1, 2, 5, 6, 9, 10} <= seen and max(seen) >= 21 and 21 in seen
    # wbcap = 0 with few levels: rank 100 in fp64 on the full shard only
    for v in ("binary", "five", "six", "nine", "mixed"):
        c = reference(v, 2, 100)
        assert c.g64.wbcap == 0 and c.g64.cap == 1024 and not c.g64.kept.any() and c.nlev.max() <= 9
        assert geometry(c, c.nlev, 4).wbcap == 1024                  # fp32: kept
        assert reference(v, 2, 12).g64.wbcap == 1024


def test_both_sides_of_the_80k_cut():
    """newton_bytes mirrored from pcr_newton.h (its NEWTON_* read from the header's text): at rank 100 in fp64 the full shard
    (cap = 1024) lands above 80 KiB and drops the window bounds, the short shard (cap = 257) lands below and keeps them; every
    fp32 cell lands below."""
    K = header_constants()
    assert (K["MAX_N"], K["MAX_LD"], K["CHUNK"], K["TP"]) == (1024, 112, 16, 17)
    assert newton_bytes(K, 4, 1024, 7, 112, 1024) == 78576 and newton_bytes(K, 8, 1024, 7, 112, 1024) == 82672      # 78.5 KB | 82.7 KB
    for v, s, r in SHORT_CELLS:
        full, short = reference(v, s, r), short_reference(v, s, r)
        assert short.g64.cap == 257 and short.g64.wbcap == 257 and short.g64.bytes_with_bounds < 80 * 1024
        if full.nlev.max() <= 9:
            assert full.g64.bytes_with_bounds > 80 * 1024 and full.g64.wbcap == 0
    for v, s, r in FP32_CELLS:
        c = reference(v, s, r)
        g = geometry(c, c.nlev, 4)
        assert g.bytes_with_bounds <= 80 * 1024 and g.wbcap == g.cap == 1024, (v, s, r)


MUTANT_CELLS = [("slots4to7", ("nine", 2, 12)), ("slots4to7", ("six", 1, 12)), ("strictness", ("five", 2, 12)), ("strictness", ("five", 1, 12)),
                ("chunk_tail", ("five", 2, 12)), ("degree", ("five", 2, 17)), ("beyond64", ("five", 2, 65)), ("beyond64", ("five", 2, 64))]


@pytest.mark.parametrize("mutant,cell", MUTANT_CELLS, ids=[f"{m}-{cid(c)}" for m, c in MUTANT_CELLS])
def test_each_mutant_is_caught_and_moves_nobody_else(mutant, cell):
    """A reference that is wrong in one mechanism of the kernel (newton_ref.MUTANTS) moves at least one user of the group the
    mechanism serves beyond 10 times that user's GPU bound -- so a kernel wrong in that way fails the per-user test -- and moves
    no user outside the group by a single bit.  (beyond64 at rank 64: the group is empty, nothing moves.)"""
    c = reference(*cell)
    Um, info = nr.shard_step(c, c.U, c.V, c.lev, c.g64.covered, mutant)
    group = np.array([o["in_group"] for o in info])
    moved = np.abs(Um - c.Uref).max(1)
    assert np.array_equal(Um[~group], c.Uref[~group]), np.flatnonzero((moved > 0) & ~group)
    assert not group[~c.g64.covered].any()
    lens, nlev = c.lens, c.nlev
    expect = {"slots4to7": c.g64.covered & (nlev >= 6) & (nlev <= 9), "strictness": c.g64.covered & np.array([o["boundary"] > 0 for o in c.info]),
              "chunk_tail": c.g64.covered & (lens % 16 != 0), "degree": c.g64.covered & np.array([o["active"] > 0 for o in c.info]),
              "beyond64": c.g64.covered & np.array([o["active"] > 0 for o in c.info]) & (c.r > 64)}[mutant]
    assert np.array_equal(group, expect)
    if cell == ("five", 2, 64):
        assert not group.any()
        return
    assert group.any() and (moved[group] > 10 * c.bound[group]).any(), (mutant, cid(cell), (moved / c.bound)[group].max())
    print(f"[newton-exact] mutant {mutant} on {cid(cell)}: {int((moved > 10 * c.bound).sum())} of {int(group.sum())} users of the group beyond "
          f"10 x bound, largest |dU| / bound = {(moved / c.bound).max():.3e}")


# ------------------------------------------------------------------------------------------------------------------------------
# 2. on the GPU
# ------------------------------------------------------------------------------------------------------------------------------

def device_step(c, precision):
    """set_factors; comp_m(); update_U() under the mode.  Returns (U, objective, info)."""
    ds = pcr.Dataset.from_triplets(c.d1, c.d2, c.user, c.item, c.val)
    with pcr.tuned(ustep_newton=1):
        s = pcr.Solver(ds, pcr.Parameter(k=c.r, solver_type=c.solver, precision=precision, **{"lambda": c.lam}))
    s.set_factors(c.U, c.V)
    s.comp_m()
    obj, info = s.update_U()
    Ug, _ = s.get_factors()
    s.close()
    return Ug, obj, info


def check_rows(tag, c, g, Ug, bound, info):
    """Every user against the reference under its bound; the summed line-search count; the CG count of the uncovered users."""
    ratio = np.abs(Ug - c.Uref).max(1) / bound
    bad = np.flatnonzero(~(ratio <= 1.0))
    u = int(np.nanargmax(ratio)) if not np.isnan(ratio).all() else 0
    cov = float(np.max(ratio[g.covered], initial=0.0))
    print(f"[newton-exact] {tag}: largest |dU| / bound = {ratio[u]:.3e} (user {c.users[u]}, {c.lens[u]} ratings, {path_of(g, u, c.nlev)}); "
          f"among the covered users {cov:.3e}")
    msg = [f"{tag}: user {c.users[x]} ({c.lens[x]} ratings, {path_of(g, x, c.nlev)}): max |dU| = {np.abs(Ug[x] - c.Uref[x]).max():.3e}, "
           f"bound {bound[x]:.3e}, reference step {c.info[x]['s']}" for x in bad]
    assert not msg, "\n".join(msg)
    ls = sum(o["tries"] for o in c.info)
    assert info["ls"] == ls, f"{tag}: {info['ls']} line-search tries against the reference's {ls}"
    stepping = sum(1 for x, o in enumerate(c.info) if o["tries"] and not g.covered[x])
    assert info["cg"] <= (2 * c.r + 10) * stepping, f"{tag}: {info['cg']} CG iterations for {stepping} uncovered users"
    if stepping:
        assert info["cg"] > 0, tag
    return float(ratio[u])


@pytest.mark.gpu
@pytest.mark.parametrize("cell", FP64_CELLS, ids=cid)
def test_every_user_against_the_reference_fp64(cell):
    """fp64, the full shard: max |dU[u]| <= 1e-7 max(|U_ref[u]|_inf, 1e-3 |U_ref|_inf) for every user, the summed line-search count
    equal to the reference's, CG iterations only for the users the kernel does not cover (all of them at rank 113).  Every rank
    on `five` under PrimalCR++; every scale and the real-valued ratings at ranks 12 and 100 under both solvers."""
    c = reference(*cell)
    Ug, _, info = device_step(c, pcr.PCR_F64)
    check_rows(f"F64 {cid(cell)} full", c, c.g64, Ug, c.bound, info)
    if c.g64.ld > 112:
        assert info["cg"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("cell", SHORT_CELLS, ids=cid)
def test_every_user_against_the_reference_short_shard(cell):
    """The short shard at rank 100 in fp64 (cap = 257: the window bounds are kept, where the full shard of the same cell drops
    them), under the same per-user rule."""
    s = short_reference(*cell)
    Ug, _, info = device_step(s, pcr.PCR_F64)
    check_rows(f"F64 {cid(cell)} short", s, s.g64, Ug, s.bound, info)
    assert info["cg"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("cell", FP32_CELLS, ids=cid)
def test_every_user_against_the_reference_fp32(cell):
    """fp32 storage.  U, V and the scores are exact in fp32, k_unewton builds g, H and delta in fp64 from them, and k_ustep's line
    search forms unew = u + delta * -step in fp64 (pcr_ustep.h: `unew[t] = v`) and stores `(T)unew[t]`: ONE rounding to fp32 of
    a value no larger than |u|_inf + |delta|_inf; the tried scores and the objective are fp32, but the step length is pinned by the
    1e-3 margin.  Nothing else rounds on that path, so the issue's default constant stands:
        max |dU[u]| <= 4 * 2^-24 * (|u|_inf + |delta_ref|_inf)
    (one rounding of relative size 2^-24 where the constant allows two, with a factor 2 to spare)."""
    c = reference(*cell)
    g = geometry(c, c.nlev, 4)
    Ug, _, info = device_step(c, pcr.PCR_F32)
    bound = 4 * 2.0 ** -24 * (np.abs(c.U).max(1) + np.array([np.abs(o["delta"]).max() for o in c.info]))
    moved = np.abs(Ug - c.Uref).max(1)
    assert np.array_equal(moved[bound == 0], np.zeros(int((bound == 0).sum())))
    check_rows(f"F32 {cid(cell)} full", c, g, Ug, np.maximum(bound, 1e-300), info)


@pytest.mark.gpu
@pytest.mark.parametrize("variant,r", SHARD_CELLS, ids=[f"{v}-r{r}" for v, r in SHARD_CELLS])
def test_a_user_does_not_depend_on_its_shard(variant, r):
    """newton_cap, newton_rs and wbcap belong to the shard, so a user's path depends on who else is there (at rank 100 in fp64:
    searched windows beside a user of 1024 ratings, kept ones without).  On these inputs H and g are exact on every path, the
    factorisation is the same code and the step length is pinned by the margin: the rows of the short shard's users are
    BIT-identical whether computed in the short shard or in the full one."""
    c = reference(variant, 2, r)
    s = short_reference(variant, 2, r)
    Uf, _, _ = device_step(c, pcr.PCR_F64)
    Us, _, _ = device_step(s, pcr.PCR_F64)
    diff = np.flatnonzero((Uf[s.users] != Us).any(1))
    msg = [f"{variant} r = {r}: user {s.users[x]} ({s.lens[x]} ratings): full shard {path_of(c.g64, s.users[x], c.nlev)}; short shard "
           f"{path_of(s.g64, x, s.nlev)}; max difference {np.abs(Uf[s.users[x]] - Us[x]).max():.3e}" for x in diff]
    assert not msg, "\n".join(msg)


_TRAJ = {}


def oracle_trajectory(oracle, r):
    """V step, U step, V step, U step from the dyadic start on `five` under PrimalCR++: the V side with the reference's default CG,
    the U side with the CG run to convergence.  Also the plain reference's SECOND U step from the oracle's (U1, V2)."""
    if r not in _TRAJ:
        c = reference("five", 2, r)
        X = oracle.build_csr(c.d1, c.d2, c.user, c.item, c.val)
        U, V, half, cg_v, before = c.U, c.V, [], [], None
        for _ in range(2):
            V, m, oV, iv = oracle.update_V_new(X, c.lam, 1.0, U, V)
            assert iv["accepted"]
            before = (U, V)
            try:
                oracle.set_cg(6 * r + 50, 1e-13)
                U, oU, iu = oracle.update_U_new(X, m, c.lam, 1.0, V, U)
            finally:
                oracle.set_cg()
            half += [oV, oU]; cg_v.append(iv["cg"])
        U2ref, info2 = nr.shard_step(c, before[0], before[1], c.lev, c.g64.covered)
        bound2 = row_bound(U2ref)
        ok = np.array([o["cond"] * 2.0 ** -52 * np.abs(o["delta"]).max() <= PRE * bound2[u] for u, o in enumerate(info2)])
        _TRAJ[r] = dict(U2=U, V2=V, half=half, cg_v=cg_v, U2ref=U2ref, info2=info2, bound2=bound2, ok=ok, ls2=iu["ls"])
    return _TRAJ[r]


@pytest.mark.parametrize("r", [12, 100])
def test_second_step_preconditions(oracle, r):
    """After two non-dyadic half steps nothing is exact any more, so the per-row rule of the second U step is checked here first:
    where cond(H) 2^-52 |delta|_inf of the second step's Hessian is within 1 / 100 of the user's bound -- all users but a handful
    must qualify -- the oracle's second step (converged CG) equals the plain reference's from the same (U1, V2) within ANCHOR."""
    t = oracle_trajectory(oracle, r)
    assert t["ok"].sum() >= len(t["ok"]) - 4, np.flatnonzero(~t["ok"])
    ratio = np.abs(t["U2"] - t["U2ref"]).max(1) / t["bound2"]
    print(f"[newton-exact] second step r={r}: {int(t['ok'].sum())} of {len(t['ok'])} users qualify; oracle against reference, largest "
          f"|dU| / bound = {ratio[t['ok']].max():.3e}; smallest line-search margin {min(min(o['margins']) for o in t['info2'] if o['margins']):.3e}")
    assert (ratio[t["ok"]] <= ANCHOR).all(), np.flatnonzero(t["ok"] & (ratio > ANCHOR))
    # users close to their optimum gain little: the decisions need only stay clear of fp64's objective tolerance (1e-11), 100 times over
    assert all(x >= 100 * TOL[pcr.PCR_F64]["obj"] for o in t["info2"] for x in o["margins"]) and all(o["accepted"] or not o["tries"] for o in t["info2"])
    assert sum(o["tries"] for o in t["info2"]) == t["ls2"]


@pytest.mark.gpu
@pytest.mark.parametrize("r", [12, 100])
def test_two_outer_iterations_under_the_mode(oracle, r):
    """V step, U step, V step, U step from the dyadic start in fp64: the second Newton U step starts from the sorted state k_ustep
    handed over after a Newton direction and a V step rebuilt.  Objectives after each half step within the fp64 trajectory
    tolerance of test_gpu_parity (max(obj, cg / 100) on the V side, max(obj, fac / 100) on the U side), the V side's CG counts equal,
    the second U globally within 2e-7 (the floor of test_exact_newton_u_step_from_the_explicit_hessian) and per row under the
    1e-7 rule against the plain reference for the users test_second_step_preconditions qualifies."""
    c = reference("five", 2, r)
    t = oracle_trajectory(oracle, r)
    tol = TOL[pcr.PCR_F64]
    ds = pcr.Dataset.from_triplets(c.d1, c.d2, c.user, c.item, c.val)
    with pcr.tuned(ustep_newton=1):
        s = pcr.Solver(ds, pcr.Parameter(k=r, solver_type=2, precision=pcr.PCR_F64, **{"lambda": c.lam}))
    s.set_factors(c.U, c.V)
    objs, cgs, ls = [], [], 0
    for _ in range(2):
        oV, iv = s.update_V(); oU, iu = s.update_U()
        objs += [oV, oU]; cgs.append(iv["cg"]); ls = iu["ls"]
    Ug, Vg = s.get_factors()
    s.close()
    err = [abs(a / b - 1) for a, b in zip(objs, t["half"])]
    print(f"[newton-exact] two iterations r={r}: relative objective differences {err}")
    for i, e in enumerate(err):
        assert e < (max(tol["obj"], tol["cg"] * 1e-2) if i % 2 == 0 else max(tol["obj"], tol["fac"] * 1e-2)), (i, objs, t["half"])
    assert cgs == t["cg_v"]
    assert rel(Vg, t["V2"]) < tol["fac"]
    assert rel(Ug, t["U2"]) < 2e-7
    assert ls == t["ls2"]
    ratio = np.abs(Ug - t["U2ref"]).max(1) / t["bound2"]
    ok = t["ok"]
    u = int(np.argmax(np.where(ok, ratio, 0.0)))
    print(f"[newton-exact] second U step r={r}: largest |dU| / bound = {ratio[u]:.3e} (user {u}, {c.lens[u]} ratings, {path_of(c.g64, u, c.nlev)})")
    bad = np.flatnonzero(ok & ~(ratio <= 1.0))
    assert not len(bad), "\n".join(f"second U step r = {r}: user {x} ({c.lens[x]} ratings, {path_of(c.g64, x, c.nlev)}): |dU| / bound = {ratio[x]:.3e}" for x in bad)
