"""The evaluator (k_eval / k_eval2 through Solver.evaluate, pcr_eval.h) against an exact reference on tied scores, every class.

With dyadic factors (tests/exact_data.py) every score is a multiple of 1/4 that fp32 holds exactly, so the fp32 evaluator must
give the fp64 answer, ties are plentiful, and a result is integer counts and a defined order: tests/eval_ref.py.  The fixture
(tests/eval_data.py) has one user per length at the class limits 128 / 512 / 4096, a test set with the lengths reversed, an
all-zero row of U, and four rating modes that pick the kernel: k_eval2 on the solver's level tables (int5), on the evaluator's own
(q10 under PrimalCR++), at 64 levels (d64), and the O(n^2) k_eval in all four instantiations (d65).

Bounds: pairwise error 1e-12, NDCG 1e-9 -- the project's own from test_fuzz_evaluator_against_oracle -- in fp32 and fp64 alike.
Part 1 (CPU) holds the oracle to the reference and shows that each mutant of the reference (ties to the higher index, > for >=,
lround buckets) moves its aggregate by at least 1e-6, 1000 x the NDCG bound: a kernel with `oi > bi` or `>` fails the named cell.
Measured on this fixture over all modes, ranks and k: smallest tie-order shift 6.9e-4 (NDCG), smallest >-for->= shift 9.7e-2,
smallest lround shift 5.3e-2 (both error).
"""
import math

import numpy as np
import pytest

import eval_data as evd
import eval_ref
import exact_data as ed
import primalcr_amd as pcr

PREC = {"F64": pcr.PCR_F64, "F32": pcr.PCR_F32}
ERR_TOL, NDCG_TOL = 1e-12, 1e-9
MUTANT_SHIFT = 1e-6
SET = ("train", "test")

_REF = {}


def reference(mode, r, group="all", mutant=None):
    """[{k: eval_ref.Result} for the training set, the same for the test set] (cached: computed once per case)."""
    key = (mode, r, group, mutant)
    if key not in _REF:
        c = evd.eval_case(mode, r, group)
        _REF[key] = [eval_ref.evaluate(c.U, c.V, *evd.csr(c, w), evd.KS, mutant=mutant) for w in (0, 1)]
    return _REF[key]


def make_solver(c, precision, solver, k=10, **kw):
    idx, item, val = evd.csr(c, 0)
    tidx, titem, tval = evd.csr(c, 1)
    ds = pcr.Dataset.from_csr(c.d1, c.d2, idx, item, val, tidx, titem, tval)
    return pcr.Solver(ds, pcr.Parameter(k=c.r, solver_type=solver, precision=precision, ndcg_k=k, **{"lambda": ed.LAMBDA}), **kw)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the precondition, on the CPU
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r", evd.RANKS)
@pytest.mark.parametrize("mode", evd.MODES)
def test_reference_oracle_and_mutants(oracle, mode, r):
    """The fixture is what eval_data says (lengths on both sides of every class limit, reversed in the test set, disjoint items,
    an all-zero row, d64 / d65 at exactly 64 / 65 raw values); every score is its own float32 round trip and a multiple of 1/4;
    the oracle equals the reference within the evaluator's bounds for k in (1, 10, 100) on both sets; and each applicable mutant
    moves the aggregate it touches by at least 1e-6 in every one of those cells -- what makes the GPU test able to fail."""
    from oracle.oracle_py import CSR
    c = evd.eval_case(mode, r)
    assert lengths_ok(c)
    assert set(np.unique(np.abs(np.concatenate([c.U.ravel(), c.V.ravel()])))) <= {0.0, 0.5, 1.0}
    assert not c.U[list(evd.ZERO_USERS)].any() and c.U[0].any()
    if mode in ("d64", "d65"):
        assert evd.max_raw_levels(c, 0) == evd.max_raw_levels(c, 1) == int(mode[1:])
    elif mode == "q10":
        val = np.concatenate([evd.csr(c, w)[2] for w in (0, 1)])
        assert evd.max_raw_levels(c, 0) == 10 and set(np.rint(val)) == {1.0, 2.0, 3.0, 4.0, 5.0} and not np.array_equal(val, np.rint(val))
    else:
        assert evd.max_raw_levels(c, 0) == evd.max_raw_levels(c, 1) == 5
    ref = reference(mode, r)
    mut = {m: reference(mode, r, mutant=m) for m in ("tie_high", "strict") + (("lround",) if mode == "q10" else ())}
    for w in (0, 1):
        idx, item, val = evd.csr(c, w)
        s = eval_ref.scores(c.U, c.V, idx, item)
        assert np.array_equal(s, s.astype(np.float32).astype(np.float64)) and np.array_equal(4 * s, np.rint(4 * s))
        ties = sum(t.n - len(np.unique(s[idx[t.u]:idx[t.u + 1]])) for t in ref[w][10].users)
        assert ties > 0.3 * s.shape[0], "the fixture is about ties"
        X = CSR(c.d1, c.d2, idx, item, val)
        for k in evd.KS:
            e, n = oracle.eval(c.U, c.V, X, k)
            R = ref[w][k]
            tag = (mode, r, SET[w], k)
            assert abs(e - R.error) < ERR_TOL and abs(n - R.ndcg) < NDCG_TOL, (tag, e, R.error, n, R.ndcg)
            shift = {"tie_high": abs(mut["tie_high"][w][k].ndcg - R.ndcg), "strict": abs(mut["strict"][w][k].error - R.error)}
            if mode == "q10":
                shift["lround"] = abs(mut["lround"][w][k].error - R.error)
            print("MUTANT", *tag, " ".join(f"{m} {x:.3e}" for m, x in shift.items()))
            for m, x in shift.items():
                assert x >= MUTANT_SHIFT, (tag, m, x)


@pytest.mark.parametrize("group", ["wave", "256", "512", "scratch"])
@pytest.mark.parametrize("mode", ["int5", "d65"])
def test_mutants_move_every_class_group(mode, group):
    """The same floor class by class (the single-class cells of the GPU test): a kernel instantiation that is wrong alone --
    one workgroup size of k_eval or k_eval2, or the global-scratch form -- fails the cell named after its class, on either set.
    A GPU cell runs k = 1, 10 and 100 under one test id, so it can fail if ONE of them moves: the floor is asked of the largest
    shift over k.  (Not of each k: a class holds 2 to 8 users, and at k = 1 the tie-order mutant is silent whenever no user's top
    score is shared by two different ratings -- measured 0 in four (mode, class, set) cells at k = 1, never at k = 10 or 100.)"""
    ref = reference(mode, 12, group)
    for m, field in (("tie_high", "ndcg"), ("strict", "error")):
        mut = reference(mode, 12, group, mutant=m)
        for w in (0, 1):
            shift = {k: abs(getattr(mut[w][k], field) - getattr(ref[w][k], field)) for k in evd.KS}
            print("MUTANT", mode, 12, group, SET[w], m, " ".join(f"k={k} {x:.3e}" for k, x in shift.items()))
            assert max(shift.values()) >= MUTANT_SHIFT, (mode, group, SET[w], m, shift)


def lengths_ok(c):
    l0, l1 = evd.lengths(c, 0), evd.lengths(c, 1)
    ok = tuple(l0) == evd.LENGTHS and tuple(l1) == evd.LENGTHS[::-1]
    ok = ok and all(evd.group_of(a) != evd.group_of(b) for a, b in zip(l0, l1) if max(a, b) > 512)      # long here, short there
    for u in range(c.d1):
        (i0, it0, _), (i1, it1, _) = evd.csr(c, 0), evd.csr(c, 1)
        a, b = it0[i0[u]:i0[u + 1]], it1[i1[u]:i1[u + 1]]
        ok = ok and (np.diff(a) > 0).all() and (np.diff(b) > 0).all() and not np.intersect1d(a, b).size and max(a.max(initial=0), b.max(initial=0)) < c.d2
    return bool(ok)


def test_class_groups_partition_the_fixture():
    """Each single-class group holds exactly the users of that class, with the ratings they have in `all`."""
    full = evd.eval_case("d65", 12)
    for w in (0, 1):
        seen = np.zeros(full.d1, np.int64)
        for g in ("wave", "256", "512", "scratch"):
            c = evd.eval_case("d65", 12, g)
            lo, hi = evd.GROUPS[g]
            n = evd.lengths(c, w)
            assert ((n == 0) | ((n >= lo) & (n <= hi))).all() and n.max() > 0
            seen += n
            for u in np.nonzero(n)[0]:
                for part, whole in zip(evd.csr(c, w)[1:], evd.csr(full, w)[1:]):
                    assert np.array_equal(part[evd.csr(c, w)[0][u]:evd.csr(c, w)[0][u + 1]], whole[evd.csr(full, w)[0][u]:evd.csr(full, w)[0][u + 1]])
        assert np.array_equal(seen, evd.lengths(full, w))


# ------------------------------------------------------------------------------------------------------------------------------
# 2. Solver.evaluate against the reference
# ------------------------------------------------------------------------------------------------------------------------------

def expected_slots(c, which):
    """{profile slot: (ratings, users)} of the eval launches over one set: make_bins' classes (empty users ride in the wave class)."""
    n = evd.lengths(c, which)
    out = {}
    for g, slot in evd.SLOT.items():
        lo, hi = evd.GROUPS[g]
        sel = (n >= lo) & (n <= hi)
        if sel.any():
            out[slot] = (int(n[sel].sum()), int(sel.sum()))
    return out


def check_cell(s, c, ref, which, k, tag, fails):
    e, n = s.evaluate(which, k)
    R = ref[which][k]
    de, dn = abs(e - R.error), abs(n - R.ndcg)
    print(f"EVALDIFF {tag} {SET[which]} k={k} err {de:.3e} ndcg {dn:.3e}")
    if not (de <= ERR_TOL and dn <= NDCG_TOL):
        longest = max(t.npairs for t in R.users)
        fails.append(f"{tag} {SET[which]} k={k} group {c.group}: error {e!r} vs {R.error!r} (diff {de:.3e} = {de * R.n_err * longest:.2f} pairs of the "
                     f"longest user, {longest} pairs), ndcg {n!r} vs {R.ndcg!r} (diff {dn:.3e})\n{R.detail()}")
    return e, n


def _cells():
    out = []
    for pname in ("F64", "F32"):
        for solver in (2, 1):
            for mode in evd.MODES:
                for r in evd.RANKS:
                    out.append(pytest.param(pname, solver, mode, r, "all", id=f"{pname}-s{solver}-{mode}-r{r}-all"))
            for mode in ("int5", "d65"):
                for g in ("wave", "256", "512", "scratch"):
                    out.append(pytest.param(pname, solver, mode, 12, g, id=f"{pname}-s{solver}-{mode}-r12-{g}"))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("pname,solver,mode,r,group", _cells())
def test_evaluate_equals_the_reference(pname, solver, mode, r, group):
    """evaluate(0, k) and evaluate(1, k) for k in (1, 10, 100) against eval_ref: error within 1e-12, NDCG within 1e-9, in both
    precisions, both solver types, every mode and rank on the whole fixture and class by class at r = 12 for int5 and d65.  A
    failure names the cell and the class group, prints the reference's per-user terms and the error difference in pairs of the
    longest user.  Each evaluate must have launched exactly the classes the set holds, with their users and ratings: in a `scratch`
    cell that is the global-scratch launch eval/512g over both long users.  The profile names a class and its workgroup form, not
    the kernel: it does not tell k_eval (d65) from k_eval2 (d64) -- that choice is fixed by max_raw_levels, which the CPU test
    pins at 64 / 65, and a wrong choice shows in the numbers (k_eval2 cannot hold 65 runs in one wave's lanes)."""
    c = evd.eval_case(mode, r, group)
    ref = reference(mode, r, group)
    s = make_solver(c, PREC[pname], solver)
    s.set_factors(c.U, c.V)
    s.profile(True)
    fails = []
    for which in (0, 1):
        for k in evd.KS:
            s.profile_reset()
            check_cell(s, c, ref, which, k, f"{pname}-s{solver}-{mode}-r{r}", fails)
            want = expected_slots(c, which)
            got = {n: s.profile_scope(n) for n in s.profile_all() if n.startswith("eval/") and s.profile_launches(n) > 0}
            assert got == want, (SET[which], k, got, want)
            assert all(s.profile_launches(n) == 1 for n in got)
            if group == "scratch":
                assert got["eval/512g"][1] == 2
    s.close()
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the ideal-DCG / discount cache
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["d64", "d65"])
def test_ndcg_k_sequence_on_one_solver(mode):
    """ndcg_k changes between calls on one solver (the ideal DCG and the discounts are cached per set, keyed on the last k; d64
    builds them from the level tables, d65 from the ratings): every result equals the single-call value of a fresh solver, the
    reference within the bounds, and the last call the first bit for bit."""
    c = evd.eval_case(mode, 12)
    ref = reference(mode, 12)
    seq = [(0, 10), (1, 10), (0, 1), (0, 100), (1, 1), (0, 10)]
    s = make_solver(c, pcr.PCR_F32, 2)
    s.set_factors(c.U, c.V)
    fails = []
    got = [check_cell(s, c, ref, w, k, f"seq-{mode}", fails) for w, k in seq]
    s.close()
    assert not fails, "\n".join(fails)
    assert got[-1] == got[0]
    for (w, k), g in zip(seq, got):
        t = make_solver(c, pcr.PCR_F32, 2, k=k)
        t.set_factors(c.U, c.V)
        assert t.evaluate(w, k) == g, (w, k)
        t.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 4. user shards
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("nranks", [2, 3])
@pytest.mark.parametrize("mode", evd.MODES)
def test_shards_add_up_to_one_rank(mode, nranks):
    """Shard-local mode on one GPU: each shard's error times its users with n >= 2, summed and divided by the total, equals the
    one-rank value within 1e-12 (NDCG: users with n >= 1, 1e-9), for both sets.  A shard without such users returns 0/0 and is
    skipped.  The shards are cut by training ratings, so a shard's test users sit in other classes than its training users."""
    c = evd.eval_case(mode, 12)
    ref = reference(mode, 12)
    one = make_solver(c, pcr.PCR_F32, 2)
    one.set_factors(c.U, c.V)
    whole = [one.evaluate(w, 10) for w in (0, 1)]
    one.close()
    sums = np.zeros((2, 2)); cnt = np.zeros((2, 2), np.int64)
    covered = 0
    for q in range(nranks):
        s = make_solver(c, pcr.PCR_F32, 2, rank=q, nranks=nranks)
        s.set_local_only(True)
        s.set_factors(c.U, c.V)
        u0, u1 = s.first_user, s.first_user + s.n_users
        covered += s.n_users
        for w in (0, 1):
            n = evd.lengths(c, w)[u0:u1]
            e, g = s.evaluate(w, 10)
            for j, (x, m) in enumerate(((e, int((n >= 2).sum())), (g, int((n >= 1).sum())))):
                if m == 0:
                    assert math.isnan(x) or x == 0.0
                    continue
                sums[w, j] += x * m; cnt[w, j] += m
        s.close()
    assert covered == c.d1
    for w in (0, 1):
        R = ref[w][10]
        assert (cnt[w, 0], cnt[w, 1]) == (R.n_err, R.n_ndcg)
        tag = (mode, nranks, SET[w])
        assert abs(sums[w, 0] / cnt[w, 0] - whole[w][0]) <= ERR_TOL and abs(sums[w, 0] / cnt[w, 0] - R.error) <= ERR_TOL, (tag, sums[w, 0] / cnt[w, 0], whole[w][0], R.error)
        assert abs(sums[w, 1] / cnt[w, 1] - whole[w][1]) <= NDCG_TOL and abs(sums[w, 1] / cnt[w, 1] - R.ndcg) <= NDCG_TOL, (tag, sums[w, 1] / cnt[w, 1], whole[w][1], R.ndcg)


# ------------------------------------------------------------------------------------------------------------------------------
# 5. pcr.predict
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("r", ed.RANKS)
def test_predict_is_exact_on_dyadic_factors(r):
    """k_predict (G lanes per pair) at every rank class: a few thousand pairs with user 0, the last user, the last item and
    repeated pairs, more than one 256-thread block at every G; the dot products are sums of quarter units, so the result is the
    numpy one bit for bit."""
    rng = np.random.default_rng(300 + r)
    d1, d2, n = 37, 4200, 3001
    U = ed.dyadic_matrix(rng, d1, r, ed.density(r)); V = ed.dyadic_matrix(rng, d2, r, ed.density(r))
    user = rng.integers(0, d1, n); item = rng.integers(0, d2, n)
    user[:4] = (0, d1 - 1, 0, d1 - 1); item[:4] = (0, d2 - 1, d2 - 1, 0)
    user[-3:] = user[10]; item[-3:] = item[10]                             # the same pair three more times
    user[1000:1003] = d1 - 1; item[1000:1003] = d2 - 1
    want = (U[user] * V[item]).sum(1)
    assert np.abs(want).max() > 0 and np.array_equal(4 * want, np.rint(4 * want))
    got = pcr.predict(U, V, user, item)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
