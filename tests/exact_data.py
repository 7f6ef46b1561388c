"""Dyadic data of the exact-parity tests (tests/test_exact_parity.py) and their definitional reference in integer arithmetic.

U, V and the probe vectors hold entries of {-1, -1/2, 0, 1/2, 1} and lambda is a power of two.  Then every score m = u.v is a
multiple of 1/4, every hinge term 1 - (m_j - m_k) too, and the gradient, the Hessian-vector product (unit 1/4) and the objective
(unit 1/16) are sums of small integers in those units: exact in fp32 and in fp64 in ANY summation order, as long as every partial
sum stays below 2^24 units (checked by test_dyadic_preconditions_and_integer_brute_force with two bits to spare)."""
import numpy as np

LAMBDA = 32.0
RANKS = (1, 7, 12, 100, 132)            # one chunk / not a multiple of 4 / several chunks / the headline rank / beyond 128
UNIT = 4                                # m, g and Ha are multiples of 1 / UNIT; the objective of 1 / UNIT^2
# every user-length class boundary of the kernels (wave / 256 / 512 / 1024 threads, 2048 split, global scratch beyond 4096)
CLASS_EDGES = (0, 1, 2, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097)
CLASS_CAPS = (0, 1, 2, 32, 64, 128, 256, 512, 1024, 2048, 4096)


def density(r):
    """Share of non-zero factor entries: keeps the scores of every rank within a few units of the hinge width, so that 20-90 % of
    the comparable pairs are active and the window boundaries fall inside every user."""
    return 1.0 if r <= 12 else 0.2 if r <= 100 else 0.1


def dyadic_matrix(rng, n, r, dens):
    X = rng.choice(np.array([-1.0, -0.5, 0.5, 1.0]), size=(n, r))
    return X * (rng.random((n, r)) < dens)


class Case:
    pass


def dyadic_case(r, solver, seed=0, real=False, d1=700, d2=6000):
    """Ratings of test_gpu_parity._mixed_set (users of 0 .. 5000 ratings over 6000 items, 5 levels) with dyadic U, V, two dyadic
    probe vectors and lambda = 32.  real: ratings moved off the integers inside their lround bucket -- PrimalCR++ (solver 2) still
    sees 5 levels, PrimalCR (solver 1) compares the raw doubles: a level per rating."""
    from test_gpu_parity import _mixed_set
    c = Case()
    c.r, c.solver, c.seed, c.real, c.lam = int(r), int(solver), int(seed), bool(real), LAMBDA
    c.d1, c.d2, c.user, c.item, c.val = _mixed_set(seed=11 + seed, d1=d1, d2=d2)
    rng = np.random.default_rng(1000 * seed + 10 * r + solver)
    if real:
        c.val = c.val + rng.uniform(-0.49, 0.49, c.val.shape[0])
    dens = density(r)
    c.U = dyadic_matrix(rng, c.d1, r, dens)
    c.V = dyadic_matrix(rng, c.d2, r, dens)
    c.a = dyadic_matrix(rng, c.d2, r, dens)
    c.a2 = dyadic_matrix(rng, c.d2, r, 1.0 if r <= 12 else 0.5)
    return c


def levels_of(val, solver):
    """What the two solvers compare: PrimalCR++ the lround bucket, PrimalCR the rating itself."""
    return np.rint(val).astype(np.int64) if solver == 2 else np.asarray(val, np.float64)      # (no rating sits on a .5)


def class_of(n):
    """'len 700 (class 513..1024)' -- the U step's length class of a user with n ratings."""
    lo = 0
    for cap in CLASS_CAPS:
        if n <= cap:
            return f"len {n} (class {lo}..{cap})"
        lo = cap + 1
    return f"len {n} (class > 4096, global scratch)"


def brute_force(c, idx, item, val, block=512, levels=None):
    """The definition, in integers (levels: each rating's level, in CSR order; None: levels_of(val, c.solver)).
    With M = 4 m, U2 = 2 U, V2 = 2 V:
        16 obj = sum_u sum_{level_j > level_k} max(0, 4 - (M_j - M_k))^2 + 2 lambda (|U2|^2 + |V2|^2)
        4 g[item_j] += -d U2[u],  4 g[item_k] += +d U2[u]   for every such pair with d = 4 - (M_j - M_k) > 0,   4 g += 2 lambda V2
    Returns (16 obj, 4 g, 4 m, pairs inside the hinge, comparable pairs), all int64."""
    U2 = np.rint(2 * c.U).astype(np.int64); V2 = np.rint(2 * c.V).astype(np.int64)
    assert np.array_equal(U2, 2 * c.U) and np.array_equal(V2, 2 * c.V)
    lam2 = int(2 * c.lam)
    assert lam2 == 2 * c.lam
    M = (U2[np.repeat(np.arange(c.d1), np.diff(idx))] * V2[item]).sum(1)          # 4 m, CSR order
    lev = levels_of(val, c.solver) if levels is None else np.asarray(levels)
    g4 = lam2 * V2
    obj16 = lam2 * int((U2 * U2).sum() + (V2 * V2).sum())
    active = comparable = 0
    for u in range(c.d1):
        s, e = int(idx[u]), int(idx[u + 1])
        if e - s < 2:
            continue
        Mu = M[s:e].astype(np.int32); Lu = lev[s:e]
        t = np.zeros(e - s, np.int64)                                               # d(16 obj)/d(M) / 2 per rating
        for b0 in range(0, e - s, block):
            b1 = min(b0 + block, e - s)
            above = Lu[b0:b1, None] > Lu[None, :]                                   # rows j (higher level) x columns k
            D = np.int32(UNIT) - (Mu[b0:b1, None] - Mu[None, :])
            act = above & (D > 0)
            D = np.where(act, D, np.int32(0)).astype(np.int64)
            comparable += int(above.sum()); active += int(act.sum())
            obj16 += int((D * D).sum())
            t[b0:b1] -= D.sum(1)
            t += D.sum(0)
        np.add.at(g4, item[s:e], t[:, None] * U2[u][None, :])
    return obj16, g4, M, active, comparable
