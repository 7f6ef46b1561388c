"""MMR diversity re-ranking (pcr_recommend_diverse_model / pcr_recommend_diverse, omp-pmf-recommend --mmr, Python
recommend_diverse()): topk items taken greedily from the pool of a user's `pool` best items.

ref_mmr() applies the contract of include/primalcr.h in numpy to the pool recommend() returns with K = pool (that pool's
exactness is held by test_recommend*.py).

Exact inputs (the dyadic tradition of test_exact_parity.py): rows of V with entries in {0, +-1} and 0, 1, 4 or 16 non-zeros
(norms 1, 2, 4; cosines multiples of 1/16), some rows duplicated (cos = 1) and some negated (cos = -1), integer U in [-2, 2],
theta in {0, 1/4, 1/2, 3/4, 1}: every m_i is a small multiple of 1/64, exact in any summation order with or without fma
contraction, so items must be equal (==) and scores bitwise equal.  test_precondition_every_margin_is_dyadic proves that with
fractions.Fraction for the generator at every shape used below.

CPU part: argument checks of both entries, the "no device" error, the CLI's usage text and refusals, the wrappers' ValueErrors,
the precondition proof and the non-vacuity of the base case.
GPU part (-m gpu): pool and lane boundaries, ranks, short and empty pools, the partial-list merge, several user batches, both
kernel forms against each other (pcr_tune "rerank_lds"), step-by-step greedy validity on Gaussian factors (the taken entry's m
within 1e-10 R of the best remaining one: the kernel's bound is about (k + 2) 2^-52 R = 5e-14 R, the margin follows
test_diversity.py's ILD_ATOL, a wrong pick is off by orders of magnitude more), the contract's identities, independence of the
other users, live solvers and the CLI.
"""
import ctypes as C
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from conftest import BIN_DIR, ROOT
from test_recommend import excl_mask, ref_topk
from test_recommend_grid import boundary_row, csr_of, int_factors, random_csr, rec_geometry, splits_of

RECOMMEND = os.path.join(BIN_DIR, "omp-pmf-recommend")
TRAIN = os.path.join(BIN_DIR, "omp-pmf-train")
ERR_ARG, ERR_DEVICE = -1, -4
THETAS = (0.0, 0.25, 0.5, 0.75, 1.0)
VALID_RTOL = 1e-10
BASE = dict(d1=40, d2=300, k=100, pool=64, topk=10, theta=0.5, seed=7)
MMR_LDS_CU = 160 * 1024


def run(cmd, cwd, timeout=600):
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=timeout)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def same_lists(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))


def lds_form_fits(pool, k, dtype):
    """Whether pcr_tune("rerank_lds", "1") takes the LDS form: mmr_wave_lds(pool, ld, 1) of pcr_topk.h within 160 KiB."""
    size = 4 if dtype == 0 else 8
    ld = (k + 3) & ~3
    per = 16 // size
    stride = ((ld // per) | 1) * per
    b = pool * stride * size + pool * (8 + size + 4)
    return ((b + 15) & ~15) <= MMR_LDS_CU


# ---------------------------------------------------------------------------------------------------------------- reference
def dyadic_V(rng, d2, k):
    """Rows with entries in {0, +-1} and 0, 1, 4 or 16 non-zeros (at most 4 when k < 16, at most 1 when k < 4); every seventh row
    repeats its predecessor and every eleventh is the negative of the row two before it."""
    counts = [0, 1] + ([4] if k >= 4 else []) + ([16] if k >= 16 else [])
    weight = np.array([1, 3, 6, 6][:len(counts)], np.float64)
    V = np.zeros((d2, k))
    for j in range(d2):
        nz = int(rng.choice(counts, p=weight / weight.sum()))
        V[j, rng.choice(k, nz, replace=False)] = rng.choice([-1.0, 1.0], nz)
    for j in range(3, d2, 7):
        V[j] = V[j - 1]
    for j in range(5, d2, 11):
        V[j] = -V[j - 2]
    return V


def stored(V, dtype):
    return V.astype(np.float32).astype(np.float64) if dtype == 0 else np.asarray(V, np.float64)


def inv_norms(Vs):
    q = (Vs * Vs).sum(1)
    return np.where(q > 0, 1.0 / np.sqrt(np.where(q > 0, q, 1.0)), 0.0)


def cosines(Vs):
    Vh = Vs * inv_norms(Vs)[:, None]
    return Vh @ Vh.T


def ref_mmr(pool_items, pool_scores, V_as_stored, topk, theta, G=None, ties=None):
    """The contract applied to the pools (rows of recommend() with K = pool, padding included): (items int32 [n, topk], scores
    [n, topk]).  All users advance one greedy step at a time, so a step is a handful of array operations on [n, pool].
    ties (optional list) receives, per user and step, the number of entries left that attain the maximum."""
    G = cosines(V_as_stored) if G is None else G
    n, P = pool_items.shape
    items = np.full((n, topk), -1, np.int32); scores = np.full((n, topk), -np.inf)
    left = pool_items >= 0
    j = np.where(left, pool_items, 0)
    s = np.where(left, pool_scores, 0.0)
    L = left.sum(1)
    smin = np.where(L > 0, np.where(left, pool_scores, np.inf).min(1, initial=np.inf), 0.0)
    R = np.where(L > 0, np.where(left, pool_scores, -np.inf).max(1, initial=-np.inf), 0.0) - smin
    R = np.where(R == 0, 1.0, R)
    rel = (1.0 - theta) * (s - smin[:, None])
    c = np.zeros((n, P))
    rows = np.arange(n)
    for t in range(min(topk, P)):
        act = left.any(1)
        if not act.any():
            break
        m = np.where(left, rel - (theta * R)[:, None] * c, -np.inf)
        w = np.argmax(m, axis=1)                                 # (the first maximum: the smaller pool position)
        if ties is not None:
            ties.extend(int(x) for x in ((m == m[rows, w][:, None]) & left).sum(1)[act])
        items[act, t] = j[act, w[act]]; scores[act, t] = s[act, w[act]]
        left[rows[act], w[act]] = False
        col = G[j, j[rows, w][:, None]]
        c = col if t == 0 else np.maximum(c, col)
    return items, scores


def check_valid(items, scores, pool_items, pool_scores, G, topk, theta, what=None):
    """Greedy validity step by step for real-valued factors: every taken entry's m within VALID_RTOL R of the best one left."""
    for i in range(items.shape[0]):
        l = pool_items[i] >= 0
        j, s = pool_items[i][l], pool_scores[i][l]
        L = j.shape[0]
        got = items[i][items[i] >= 0]
        assert got.shape[0] == min(topk, L), (what, i)
        assert np.all(items[i][got.shape[0]:] == -1) and np.all(np.isneginf(scores[i][got.shape[0]:])), (what, i)
        assert np.unique(got).shape[0] == got.shape[0], (what, i)
        pos = {int(x): p for p, x in enumerate(j)}
        assert all(int(x) in pos for x in got), (what, i)
        order = [pos[int(x)] for x in got]
        assert np.array_equal(bits(scores[i, :len(order)]), bits(s[order])), (what, i)
        if L == 0:
            continue
        smin = s.min()
        R = s.max() - smin
        R = 1.0 if R == 0 else R
        Gp = G[np.ix_(j, j)]
        c = np.zeros(L)
        left = np.ones(L, bool)
        for t, w in enumerate(order):
            m = (1.0 - theta) * (s - smin) - (theta * R) * c
            assert m[w] >= m[left].max() - VALID_RTOL * R, (what, i, t, m[w], m[left].max())
            left[w] = False
            c = Gp[:, w].copy() if t == 0 else np.maximum(c, Gp[:, w])


def _model_call(U, V, index, item, users, topk, pool, theta, dtype=1, n=None, out=True):
    """pcr_recommend_diverse_model through ctypes, arrays as given (None = NULL); returns the status code."""
    import primalcr_amd as pcr
    n = (len(users) if users is not None else U.shape[0]) if n is None else n
    items = np.empty((max(n, 1), max(topk, 1)), np.int32); scores = np.empty((max(n, 1), max(topk, 1)))
    ptr = lambda a: None if a is None else a.ctypes.data
    return pcr.lib().pcr_recommend_diverse_model(ptr(U), U.shape[0], ptr(V), V.shape[0], U.shape[1], ptr(index), ptr(item), n, ptr(users),
                                                 topk, pool, theta, dtype, ptr(items) if out else None, ptr(scores) if out else None, 0)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_model_entry_argument_checks():
    import primalcr_amd as pcr
    rng = np.random.default_rng(1)
    U, V = rng.standard_normal((20, 5)), rng.standard_normal((30, 5))
    index = np.array([0] + [2] * 20, np.int64)
    item = np.array([3, 7], np.int32)
    users = np.arange(20, dtype=np.int32)

    def bad(*a, **kw):
        assert _model_call(*a, **kw) == ERR_ARG
        assert b"pcr_recommend_diverse_model" in pcr.lib().pcr_last_error()

    bad(U, V, index, item, users, 5, 10, float("nan"))
    bad(U, V, index, item, users, 5, 10, -0.01)
    bad(U, V, index, item, users, 5, 10, 1.01)
    bad(U, V, index, item, users, 0, 10, 0.5)
    bad(U, V, index, item, users, -1, 10, 0.5)
    bad(U, V, index, item, users, 5, 4, 0.5)
    bad(U, V, index, item, users, 5, 1025, 0.5)
    bad(U, V, index, item, users, 1025, 1025, 0.5)
    # every argument error of pcr_recommend_model
    bad(U, V, index, item, users, 5, 10, 0.5, dtype=5)
    bad(U, V, index, item, users, 5, 10, 0.5, out=False)
    bad(U, V, index, item, np.array([0, 20], np.int32), 5, 10, 0.5)
    bad(U, V, index, item, np.array([-1], np.int32), 5, 10, 0.5)
    bad(U, V, index, item, None, 5, 10, 0.5, n=21)
    bad(U, V, index, item, users, 5, 10, 0.5, n=-1)
    nm = index.copy(); nm[5] = 1
    bad(U, V, nm, item, users, 5, 10, 0.5)
    bad(U, V, index, np.array([3, 30], np.int32), users, 5, 10, 0.5)
    bad(U, V, index, None, users, 5, 10, 0.5)
    nz = index.copy(); nz[0] = 1
    bad(U, V, nz, item, users, 5, 10, 0.5)
    # the solver entry checks its solver first
    one = np.array([5], np.int32)
    buf_i = np.empty(4, np.int32); buf_s = np.empty(4)
    assert pcr.lib().pcr_recommend_diverse(None, 1, one.ctypes.data, 2, 4, 0.5, 0, buf_i.ctypes.data, buf_s.ctypes.data) == ERR_ARG


def test_python_wrappers_refuse_bad_arguments():
    import primalcr_amd as pcr
    rng = np.random.default_rng(2)
    U, V = rng.standard_normal((6, 3)), rng.standard_normal((9, 3))
    for kw in (dict(topk=0), dict(topk=5, pool=4), dict(topk=5, pool=1025), dict(topk=5, theta=1.5), dict(topk=5, theta=-0.1),
               dict(topk=5, theta=float("nan")), dict(topk=2000)):
        with pytest.raises(ValueError):
            pcr.recommend_diverse(U, V, **kw)
        with pytest.raises(ValueError):
            pcr.Solver.recommend_diverse(None, **kw)                      # (checked before the solver is touched)
    with pytest.raises(ValueError):
        pcr.recommend_diverse(U, V, 3, exclude=(np.zeros(7, np.int64), np.array([1], np.int32)))
    from primalcr_amd.api import _rerank_args
    assert _rerank_args(10, None, 0.5) == (10, 100, 0.5) and _rerank_args(200, None, 0)[1] == 1024 and _rerank_args(1, None, 1)[1] == 10
    assert pcr.recommend_diverse is pcr.api.recommend_diverse and "recommend_diverse" in pcr.__all__


def test_model_entry_without_a_device_is_a_device_error():
    code = ("import sys, numpy as np; sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')\n"
            "from test_rerank import _model_call\n"
            "U = np.ones((4, 3)); V = np.ones((6, 3))\n"
            "print(_model_call(U, V, np.array([0, 1, 1, 1, 1], np.int64), np.array([2], np.int32), np.arange(4, dtype=np.int32), 2, 4, 0.5))\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    assert int(out.stdout.strip().splitlines()[-1]) == ERR_DEVICE


def test_cli_usage_and_refusals(tmp_path):
    import primalcr_amd as pcr
    from primalcr_amd import synth
    r = run([RECOMMEND], tmp_path)
    assert r.returncode == 1 and "--mmr theta" in r.stdout and "--pool P" in r.stdout and r.stdout.startswith("Usage: omp-pmf-recommend [-K topk]")
    R = synth.generate("tiny", seed=3)
    d = synth.write_dir(R, str(tmp_path / "data"))
    # refused before the model is read
    r = run([RECOMMEND, "--pool", "50", str(tmp_path / "missing.model"), "out.txt"], tmp_path)
    assert r.returncode == 1 and "--pool" in r.stderr and "--mmr" in r.stderr and "can't open" not in r.stderr
    r = run([RECOMMEND, "--mmr", "0.5", "--eval", d, str(tmp_path / "missing.model")], tmp_path)
    assert r.returncode == 1 and "--mmr" in r.stderr and "can't open" not in r.stderr
    r = run([RECOMMEND, "--mmr", "0.5", "--diversity", str(tmp_path / "missing.model")], tmp_path)
    assert r.returncode == 1 and "--mmr" in r.stderr and "can't open" not in r.stderr
    for v in ("1.5", "-0.1", "nan", "x", ""):
        r = run([RECOMMEND, "--mmr", v, "m.model", "out.txt"], tmp_path)
        assert r.returncode == 1 and "--mmr" in r.stderr, v
    for v in ("0", "1025", "x"):
        r = run([RECOMMEND, "--mmr", "0.5", "--pool", v, "m.model", "out.txt"], tmp_path)
        assert r.returncode == 1 and "--pool" in r.stderr, v
    r = run([RECOMMEND, "--mmr", "0.5", "--pool", "5", "-K", "10", "m.model", "out.txt"], tmp_path)
    assert r.returncode == 1 and "--pool" in r.stderr and "can't open" not in r.stderr
    r = run([RECOMMEND, "--mmr"], tmp_path)
    assert r.returncode == 1 and "--mmr needs a value" in r.stderr and r.stdout.startswith("Usage: omp-pmf-recommend")
    rng = np.random.default_rng(2)
    pcr.model_save(str(tmp_path / "ok.model"), rng.standard_normal((R.d1, 4)), rng.standard_normal((R.d2, 4)))
    r = run([RECOMMEND, "--mmr", "0.5", "ok.model"], tmp_path)                # the plain form's two positionals
    assert r.returncode == 1 and r.stdout.startswith("Usage: omp-pmf-recommend")


def _exact_case(seed, d1, d2, k, special=None):
    rng = np.random.default_rng(seed)
    U, V = int_factors(rng, d1, k), dyadic_V(rng, d2, k)
    index, item = random_csr(rng, d1, d2, special)
    return U, V, index, item


def _short_case():
    """test_short_and_empty_pools' inputs: exclusion rows that leave 40, 7, 1, 0, 64, 63, 10 and 9 eligible items; zero rows of V."""
    rng = np.random.default_rng(61)
    d1, d2, k = 24, 300, 16
    U, V = int_factors(rng, d1, k), dyadic_V(rng, d2, k)
    V[np.arange(0, d2, 9)] = 0.0
    keep = {0: 40, 1: 7, 2: 1, 3: 0, 4: 64, 5: 63, 6: 10, 7: 9}
    rows = []
    for u in range(d1):
        left = np.sort(rng.choice(d2, keep.get(u % 8), replace=False))
        rows.append(np.setdiff1d(np.arange(d2), left).astype(np.int32))
    index, item = csr_of(rows)
    return U, V, index, item


# every (seed, d1, d2, k, pools) of the exact GPU cases below (the partial-list merge's exclusion rows do not touch the factors;
# its proof runs on the generator's own CSR)
EXACT_SHAPES = [(BASE["seed"], BASE["d1"], BASE["d2"], BASE["k"], (BASE["pool"],)),
                (21, 70, 300, 16, (1, 2, 63, 64, 65, 100)), (22, 70, 1100, 16, (1024,)),
                (31, 70, 300, 1, (64,)), (32, 70, 300, 7, (64,)), (33, 70, 300, 16, (64,)), (34, 70, 300, 100, (64,)),
                (35, 70, 300, 132, (64,)), (36, 70, 300, 200, (64,)), (41, 64, 5000, 8, (100,)), (51, 500, 1100, 4, (1024,))]
PROOF_USERS, PROOF_USERS_1024 = 70, 16   # every user of the cases with pools up to 100; the first 16 at pool 1024 (a million pairs each)


def test_precondition_every_margin_is_dyadic():
    """For the generator at every (k, pool, theta) of the exact cases, the short-pool case included: every cosine between two pool
    entries and every m_i -- for EVERY pool entry as the row taken, so whatever rows a greedy run takes at whatever topk, and for
    c_i = 0 -- is recomputed in exact rational arithmetic, is a dyadic rational of at most 24 significant bits and equals the float
    computation.  So no summation order, fma contraction or rounding can move a comparison, and the bitwise assertions of the GPU
    tests are sound.  The sweep (all users of the cases with pools up to 100, a sample of PROOF_USERS_1024 users at pool 1024; all
    pool x pool pairs, all five thetas) uses int64 numerators over the
    common denominator 64 (theta = q / 4, cos = g / 16): exact integers; for the first two users and eight taken rows the same
    values are formed with fractions.Fraction and must agree with both."""
    def dyadic24(x):
        d = x.denominator
        if d & (d - 1):
            return False
        n = abs(x.numerator)
        while n and n % 2 == 0:
            n //= 2
        return n < (1 << 24)

    cases = [(seed,) + _exact_case(seed, d1, d2, k) + (pools,) for seed, d1, d2, k, pools in EXACT_SHAPES] + [(61,) + _short_case() + ((64,),)]
    for seed, U, V, index, item, pools in cases:
        d1, d2 = U.shape[0], V.shape[0]
        users = np.arange(min(d1, PROOF_USERS if max(pools) < 1024 else PROOF_USERS_1024))
        q = (V * V).sum(1)
        assert set(np.unique(q)) <= {0.0, 1.0, 4.0, 16.0}
        assert set(np.unique(inv_norms(V))) <= {0.0, 1.0, 0.5, 0.25}
        nrm = np.sqrt(q).astype(np.int64)                                # 0, 1, 2, 4
        Vi = V.astype(np.int64)
        S = U[users] @ V.T
        excl = excl_mask(d1, d2, index, item)[users]
        for pool in pools:
            pi, ps = ref_topk(S, excl, pool)
            for i in range(users.shape[0]):
                l = pi[i] >= 0
                j, s = pi[i][l], ps[i][l]
                if j.shape[0] == 0:
                    continue
                dots = Vi[j] @ Vi[j].T
                den = nrm[j][:, None] * nrm[j][None, :]
                assert np.all((dots * 16) % np.where(den > 0, den, 1) == 0)
                g16 = np.where(den > 0, (dots * 16) // np.where(den > 0, den, 1), 0)     # cos = g16 / 16, exactly
                G = cosines(V[j])
                assert np.array_equal(G * 16.0, g16.astype(np.float64))
                si = s.astype(np.int64)
                assert np.array_equal(si.astype(np.float64), s)
                smin = int(si.min()); R = int(si.max()) - smin
                R = 1 if R == 0 else R
                for qn, theta in enumerate(THETAS):                      # theta = qn / 4
                    for g, Gx in ((g16, G), (np.zeros((1, j.shape[0]), np.int64), np.zeros((1, j.shape[0])))):   # c_i a cosine; c_i = 0
                        M64 = (4 - qn) * 16 * (si - smin)[None, :] - qn * R * g         # 64 m, for (row taken a, entry b)
                        assert np.abs(M64).max() < (1 << 24)
                        mf = (1.0 - theta) * (s - float(smin))[None, :] - (theta * float(R)) * Gx
                        assert np.array_equal(mf * 64.0, M64.astype(np.float64)), (seed, pool, theta)
                if i >= 2:
                    continue
                norm = {0: Fraction(0), 1: Fraction(1), 2: Fraction(1, 2), 4: Fraction(1, 4)}
                fs, fR = Fraction(smin), Fraction(R)
                for a in range(min(8, j.shape[0])):
                    for b in range(j.shape[0]):
                        gf = Fraction(int(dots[a, b])) * norm[int(nrm[j[a]])] * norm[int(nrm[j[b]])]
                        assert dyadic24(gf) and Fraction(G[a, b]) == gf == Fraction(int(g16[a, b]), 16)
                        for qn, theta in enumerate(THETAS):
                            th = Fraction(theta)
                            m = (1 - th) * (Fraction(int(si[b])) - fs) - th * fR * gf
                            mf = (1.0 - theta) * (s[b] - float(smin)) - (theta * float(R)) * G[a, b]
                            assert dyadic24(m) and Fraction(mf) == m, (seed, pool, theta)
                            assert m == Fraction(int((4 - qn) * 16 * (si[b] - smin) - qn * R * g16[a, b]), 64)


def test_base_case_is_not_vacuous():
    """The base case re-ranks: at least half of the users' lists differ from the plain top-10, and at least 10 % of all greedy
    steps have two or more entries tied at the maximum (so the position tie-break decides them)."""
    b = BASE
    U, V, index, item = _exact_case(b["seed"], b["d1"], b["d2"], b["k"])
    S = U @ V.T
    excl = excl_mask(b["d1"], b["d2"], index, item)
    pi, ps = ref_topk(S, excl, b["pool"])
    ties = []
    items, _ = ref_mmr(pi, ps, V, b["topk"], b["theta"], ties=ties)
    changed = int((items != pi[:, :b["topk"]]).any(1).sum())
    tied = sum(1 for t in ties if t >= 2)
    print("changed", changed, "of", b["d1"], "tied steps", tied, "of", len(ties))
    assert len(ties) == b["d1"] * b["topk"]
    assert 2 * changed >= b["d1"]
    assert 10 * tied >= len(ties)


# ---------------------------------------------------------------------------------------------------------------- GPU helpers
def both_forms(fn, pool, k, dtype):
    """fn() under both kernel forms (where the LDS form applies): bitwise the same lists; returns them."""
    import primalcr_amd as pcr
    with pcr.tuned(rerank_lds=0):
        a = fn()
    if lds_form_fits(pool, k, dtype):
        with pcr.tuned(rerank_lds=1):
            b = fn()
        assert same_lists(a, b), ("forms differ", pool, k, dtype)
    c = fn()                                                        # the default choice
    assert same_lists(a, c), ("default differs", pool, k, dtype)
    return a


def check_exact(U, V, exclude, users, dtype, pool, topks, thetas=THETAS, G=None, what=None):
    import primalcr_amd as pcr
    G = cosines(stored(V, dtype)) if G is None else G
    pi, ps = pcr.recommend(U, V, pool, exclude=exclude, users=users, dtype=dtype)
    for topk in topks:
        for theta in thetas:
            got = both_forms(lambda: pcr.recommend_diverse(U, V, topk, pool=pool, theta=theta, exclude=exclude, users=users, dtype=dtype),
                             pool, U.shape[1], dtype)
            want = ref_mmr(pi, ps, None, topk, theta, G=G)
            assert np.array_equal(got[0], want[0]), (what, pool, topk, theta)
            assert np.array_equal(bits(got[1]), bits(want[1])), (what, pool, topk, theta)
    return pi, ps


DTYPES = pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.timeout(900)
@DTYPES
def test_base_case(dtype):
    b = BASE
    U, V, index, item = _exact_case(b["seed"], b["d1"], b["d2"], b["k"])
    assert lds_form_fits(b["pool"], b["k"], dtype)
    check_exact(U, V, (index, item), None, dtype, b["pool"], (b["topk"],))


@pytest.mark.gpu
@pytest.mark.timeout(900)
@DTYPES
@pytest.mark.parametrize("pool", [1, 2, 63, 64, 65, 100, 1024])
def test_pool_and_lane_boundaries(dtype, pool):
    d1, d2, k = 70, (1100 if pool == 1024 else 300), 16
    U, V, index, item = _exact_case(22 if pool == 1024 else 21, d1, d2, k)
    assert lds_form_fits(pool, k, dtype) == (not (pool == 1024 and dtype == 1))     # (1024 fp64 rows of 18 values: 167 KiB)
    G = cosines(stored(V, dtype))
    check_exact(U, V, (index, item), None, dtype, pool, sorted({1, min(10, pool), pool}), G=G)


@pytest.mark.gpu
@pytest.mark.timeout(900)
@DTYPES
@pytest.mark.parametrize("k,seed", [(1, 31), (7, 32), (16, 33), (100, 34), (132, 35), (200, 36)])
def test_ranks(dtype, k, seed):
    U, V, index, item = _exact_case(seed, 70, 300, k)
    assert lds_form_fits(64, k, dtype)
    check_exact(U, V, (index, item), None, dtype, 64, (10,))


@pytest.mark.gpu
@pytest.mark.timeout(900)
@DTYPES
def test_short_and_empty_pools(dtype):
    """Exclusion rows that leave 40 (< pool), 7 (< topk), 1 and 0 eligible items, with zero rows of V among them."""
    pool, topk = 64, 10
    U, V, index, item = _short_case()
    pi, ps = check_exact(U, V, (index, item), None, dtype, pool, (topk, pool), what="short")
    assert [int((pi[u] >= 0).sum()) for u in range(8)] == [40, 7, 1, 0, 64, 63, 10, 9]
    assert (np.abs(V[pi[pi >= 0]]).sum(1) == 0).any()                       # zero rows were in a pool
    import primalcr_amd as pcr
    it, sc = pcr.recommend_diverse(U, V, topk, pool=pool, theta=0.5, exclude=(index, item), dtype=dtype)
    assert np.all(it[3] == -1) and np.all(np.isneginf(sc[3])) and (it[1] >= 0).sum() == 7 and np.all(it[1, 7:] == -1) and np.all(np.isneginf(sc[1, 7:]))


@pytest.mark.gpu
@pytest.mark.timeout(900)
@DTYPES
def test_partial_list_merge(dtype):
    d1, d2, k, pool = 64, 5000, 8, 100
    assert splits_of(d1, d2, pool, dtype) == 4
    per = rec_geometry(d1, d2, pool, dtype)[0].per
    U, V, index, item = _exact_case(41, d1, d2, k, {u: boundary_row(u, d2, per) for u in range(d1)})
    check_exact(U, V, (index, item), None, dtype, pool, (10,), thetas=(0.0, 0.5, 1.0))


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_several_user_batches():
    import primalcr_amd as pcr
    n, d1, d2, k, pool, topk, dtype, theta = 90000, 500, 1100, 4, 1024, 2, 1, 0.5
    g = rec_geometry(n, d2, pool, dtype)
    assert len(g) >= 2
    U, V, index, item = _exact_case(51, d1, d2, k)
    rng = np.random.default_rng(52)
    users = rng.integers(0, d1, n).astype(np.int32)
    assert lds_form_fits(pool, k, dtype)                                    # (two users per workgroup in the LDS form)
    got = both_forms(lambda: pcr.recommend_diverse(U, V, topk, pool=pool, theta=theta, exclude=(index, item), users=users, dtype=dtype),
                     pool, k, dtype)
    # every repeated id returns identical bits, whichever batch it sits in
    first = np.full(d1, -1, np.int64)
    first[users[::-1]] = np.arange(n - 1, -1, -1)
    assert np.array_equal(got[0], got[0][first[users]]) and np.array_equal(bits(got[1]), bits(got[1][first[users]]))
    edge = [r for b in g for r in (b.b0, b.b0 + b.users - 1)]
    rows = np.unique(np.concatenate([edge, rng.integers(0, n, 200 - len(edge))])).astype(np.int64)
    pi, ps = pcr.recommend(U, V, pool, exclude=(index, item), users=users[rows], dtype=dtype)
    want = ref_mmr(pi, ps, V, topk, theta)
    assert np.array_equal(got[0][rows], want[0]) and np.array_equal(bits(got[1][rows]), bits(want[1]))
    assert (got[0][rows] != pi[:, :topk]).any()


def _gauss(seed, d1, d2, k):
    rng = np.random.default_rng(seed)
    U, V = rng.standard_normal((d1, k)), rng.standard_normal((d2, k))
    V[::13] *= 3.0                                                          # norms vary
    V[7::29] = V[6::29][:V[7::29].shape[0]] * 0.5 + 0.01 * rng.standard_normal(V[7::29].shape)    # near-parallel pairs
    index, item = random_csr(rng, d1, d2)
    return U, V, index, item


@pytest.mark.gpu
@pytest.mark.timeout(900)
@DTYPES
@pytest.mark.parametrize("k", [100, 200])
def test_general_factors_are_greedy_step_by_step(dtype, k):
    import primalcr_amd as pcr
    d1, d2, pool, topk = 60, 1500, 100, 20
    U, V, index, item = _gauss(70 + k, d1, d2, k)
    G = cosines(stored(V, dtype))
    pi, ps = pcr.recommend(U, V, pool, exclude=(index, item), dtype=dtype)
    forms = [0] + ([1] if lds_form_fits(pool, k, dtype) else [])
    for theta in (0.3, 0.7):
        changed = 0
        for form in forms:
            with pcr.tuned(rerank_lds=form):
                it, sc = pcr.recommend_diverse(U, V, topk, pool=pool, theta=theta, exclude=(index, item), dtype=dtype)
            check_valid(it, sc, pi, ps, G, topk, theta, (k, theta, form))
            changed += int((it != pi[:, :topk]).any(1).sum())
        assert changed >= len(forms) * d1 // 2                              # the re-ranking does re-rank


@pytest.mark.gpu
@pytest.mark.timeout(900)
@DTYPES
def test_identities(dtype):
    import primalcr_amd as pcr
    d1, d2, k, topk = 60, 1500, 100, 20
    U, V, index, item = _gauss(81, d1, d2, k)
    ex = (index, item)
    plain = pcr.recommend(U, V, topk, exclude=ex, dtype=dtype)
    for pool in (topk, 100, 1024):
        for form in (0, 1):
            with pcr.tuned(rerank_lds=form):
                assert same_lists(pcr.recommend_diverse(U, V, topk, pool=pool, theta=0.0, exclude=ex, dtype=dtype), plain), (pool, form)
        first = pcr.recommend_diverse(U, V, topk, pool=pool, theta=0.9, exclude=ex, dtype=dtype)
        assert np.array_equal(first[0][:, 0], plain[0][:, 0]) and np.array_equal(bits(first[1][:, 0]), bits(plain[1][:, 0]))
    for theta in (0.5, 1.0):
        it, sc = pcr.recommend_diverse(U, V, topk, pool=topk, theta=theta, exclude=ex, dtype=dtype)
        o, p = np.argsort(it, axis=1, kind="stable"), np.argsort(plain[0], axis=1, kind="stable")
        assert np.array_equal(np.take_along_axis(it, o, 1), np.take_along_axis(plain[0], p, 1))
        assert np.array_equal(bits(np.take_along_axis(sc, o, 1)), bits(np.take_along_axis(plain[1], p, 1)))
        assert (it != plain[0]).any()


@pytest.mark.gpu
@pytest.mark.timeout(900)
@DTYPES
def test_independence_of_the_other_users(dtype):
    import primalcr_amd as pcr
    d1, d2, k = 300, 2500, 40
    U, V, index, item = _gauss(91, d1, d2, k)
    kw = dict(pool=100, theta=0.6, exclude=(index, item), dtype=dtype)
    rng = np.random.default_rng(92)
    a = pcr.recommend_diverse(U, V, 10, **kw)
    assert same_lists(a, pcr.recommend_diverse(U, V, 10, **kw))
    perm = rng.permutation(d1).astype(np.int32)
    b = pcr.recommend_diverse(U, V, 10, users=perm, **kw)
    assert same_lists(b, (a[0][perm], a[1][perm]))
    sub = np.array([299, 0, 17, 17, 64], np.int32)
    c = pcr.recommend_diverse(U, V, 10, users=sub, **kw)
    assert same_lists(c, (a[0][sub], a[1][sub]))


@pytest.mark.gpu
@pytest.mark.timeout(1200)
def test_live_solvers():
    """Solver.recommend_diverse on PCR++ and CCDR1 equals recommend_diverse on get_factors() in the solver's storage type; a
    shard returns its users' rows of the full call; training afterwards is bitwise that of a run without the call; the profile
    slot has launches."""
    import primalcr_amd as pcr
    from primalcr_amd import synth
    R = synth.generate("small", seed=17)
    ds = pcr.Dataset.from_ratings(R)
    idx, it, val = ds.csr(0)
    tidx, tit, tval = ds.csr(1)
    rng = np.random.default_rng(9)
    r = 16
    for solver_type in (pcr.PCR_SOLVER_PCRPP, pcr.PCR_SOLVER_CCDR1):
        for prec in (pcr.PCR_F32, pcr.PCR_F64):
            what = (solver_type, prec)
            p = pcr.Parameter(k=r, precision=prec, solver_type=solver_type, **{"lambda": 100.0})
            s, t = pcr.Solver(ds, p), pcr.Solver(ds, p)
            if solver_type == pcr.PCR_SOLVER_CCDR1:
                U0, V0 = pcr.initial_col(R.d1, r), np.zeros((R.d2, r))
            else:
                U0, V0 = pcr.initial(R.d1, r), pcr.initial(R.d2, r)
            s.set_factors(U0, V0); t.set_factors(U0, V0)
            s.iterate(1); t.iterate(1)
            U, V = s.get_factors()
            s.profile(True)
            a = s.recommend_diverse(10, pool=64, theta=0.5)
            prof = s.profile_all()
            assert prof.get("recommend/rerank", (0, 0))[1] >= 2 and "recommend/score" in prof, prof
            s.profile(False)
            assert same_lists(a, pcr.recommend_diverse(U, V, 10, pool=64, theta=0.5, exclude=ds, dtype=prec)), what
            assert a[0].shape == (R.d1, 10)
            users = rng.choice(R.d1, 33, replace=False).astype(np.int32)
            b = s.recommend_diverse(5, theta=0.8, users=users, exclude_train=False)
            assert same_lists(b, pcr.recommend_diverse(U, V, 5, pool=50, theta=0.8, users=users, dtype=prec)), what
            if solver_type == pcr.PCR_SOLVER_PCRPP:
                lo, hi = R.d1 // 3, R.d1
                dsl = pcr.Dataset.from_csr(hi - lo, R.d2, idx[lo:hi + 1] - idx[lo], it[idx[lo]:idx[hi]], val[idx[lo]:idx[hi]].copy(),
                                           tidx[lo:hi + 1] - tidx[lo], tit[tidx[lo]:tidx[hi]], tval[tidx[lo]:tidx[hi]].copy())
                sh = pcr.Solver(dsl, p, rank=1, nranks=2, shard=(lo, R.d1))      # (pcr_solver_create_shard)
                sh.set_local_only(True)
                sh.set_factors_local(U[lo:hi], V)
                c = sh.recommend_diverse(10, pool=64, theta=0.5)
                assert same_lists(c, (a[0][lo:hi], a[1][lo:hi])), what
                mine = np.array([hi - 1, lo, lo + 5], np.int32)                  # GLOBAL ids of the shard
                d = sh.recommend_diverse(10, pool=64, theta=0.5, users=mine)
                assert same_lists(d, (a[0][mine], a[1][mine])), what
                with pytest.raises(pcr.PcrError, match="pcr_recommend_diverse"):
                    sh.recommend_diverse(10, users=np.array([0], np.int32))      # outside the shard
                sh.close()
            s.iterate(1); t.iterate(1)
            Us, Vs = s.get_factors(); Ut, Vt = t.get_factors()
            assert np.array_equal(Us, Ut) and np.array_equal(Vs, Vt), what
            s.close(); t.close()


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_cli_end_to_end(tmp_path):
    import primalcr_amd as pcr
    from primalcr_amd import synth
    R = synth.generate("small", seed=13)
    d = synth.write_dir(R, str(tmp_path / "data"))
    out = run([TRAIN, "-k", "8", "-t", "2", "-l", "100", d, "m.model"], tmp_path)
    assert out.returncode == 0, out.stderr
    U, V = pcr.model_load(str(tmp_path / "m.model"))
    ds = pcr.Dataset.from_ratings(R)
    r = run([RECOMMEND, "--mmr", "0.5", "--pool", "64", "-x", d, "m.model", "lists.txt"], tmp_path)
    assert r.returncode == 0, r.stderr
    items, _ = pcr.recommend_diverse(U, V, 10, pool=64, theta=0.5, exclude=ds)
    lines = (tmp_path / "lists.txt").read_text().strip().splitlines()
    assert len(lines) == R.d1
    for u, line in enumerate(lines):
        f = [int(x) for x in line.split()]
        assert f[0] == u + 1 and f[1:] == [int(j) + 1 for j in items[u] if j >= 0], u
    plain, _ = pcr.recommend(U, V, 10, exclude=ds)
    assert (items != plain).any()
    (tmp_path / "users").write_text("3\n1\n3\n")
    r = run([RECOMMEND, "--mmr", "1", "-K", "4", "--f32", "--scores", "-u", "users", "m.model", "three.txt"], tmp_path)
    assert r.returncode == 0, r.stderr
    it, sc = pcr.recommend_diverse(U, V, 4, theta=1.0, users=np.array([2, 0, 2], np.int32), dtype=pcr.PCR_F32)
    lines = (tmp_path / "three.txt").read_text().strip().splitlines()
    assert [int(l.split()[0]) for l in lines] == [3, 1, 3]
    for i, line in enumerate(lines):
        assert [x.split(":")[0] for x in line.split()[1:]] == [str(int(j) + 1) for j in it[i]]
        assert [x.split(":")[1] for x in line.split()[1:]] == [f"{v:.6f}" for v in sc[i]]
