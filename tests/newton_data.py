"""Fixture of the exact-Newton U step's edge tests (tests/test_newton_exact.py): one small rating structure with a user at every
length at which k_unewton (primalcr_amd/csrc/pcr_newton.h) changes its path, the dyadic factors of tests/exact_data.py and ratings
from the scales of tests/scale_data.py whose level counts select the window form (kept bounds for 2..9 levels, searched otherwise).

    structure   d2 = 6000; one user per length in LENGTHS (n < 8: empty prefix segments; 15 | 16 | 17: NEWTON_CHUNK; 255 | 256 | 257:
                the block; 1023 | 1024 | 1025: NEWTON_MAX_N, the last one and 2049 leave the kernel for the converged CG), N_MORE
                users of 3..200 ratings: 46 users, about 10 000 ratings; items seeded, ascending per user
    factors     exact_data.dyadic_matrix with density(r), lambda = 32: scores are multiples of 1/4, so window membership, g and H
                are exact in fp32 and in fp64 in any summation order, and pairs with m_j - m_k = 1 exactly are frequent
    ratings     scale_data.SCALES[scale] (`mixed`: user u draws from scale_data.MIXED[u % 4]); `real`: the scale `five` moved off
                the integers inside its rounding bucket (exact_data's jitter): 5 levels under PrimalCR++, a level per rating under PrimalCR
    short       the users of at most SHORT_MAX ratings as a Dataset of their own: same items, same rows of V, same rows of U
"""
import numpy as np

import exact_data as ed
import scale_data as sd

D2 = 6000
LENGTHS = (0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049)
N_MORE = 20
SHORT_MAX = 257
STRUCTURE_SEED = 7300
RATING_SEED = 61000
FACTOR_SEED = 83000
LAMBDA = ed.LAMBDA
SCALES = ("one", "binary", "five", "six", "nine", "ten", "jester", "mixed")
VARIANTS = SCALES + ("real",)
RANKS = (1, 12, 16, 17, 48, 64, 65, 80, 100, 112, 113)     # nt = 1, 1, 1, 2, 3, 4, 5, 5, 7 (pad), 7 (no pad); 113: ld = 116 > NEWTON_MAX_LD

_STRUCT = []


def structure():
    """(d1, idx int64[d1 + 1], user, item): the users of LENGTHS in that order, then the N_MORE seeded ones."""
    if not _STRUCT:
        rng = np.random.default_rng(STRUCTURE_SEED)
        lens = np.concatenate([LENGTHS, rng.integers(3, 201, N_MORE)]).astype(np.int64)
        user = np.repeat(np.arange(len(lens)), lens)
        item = np.concatenate([np.sort(rng.choice(D2, int(n), replace=False)) for n in lens]).astype(np.int64)
        idx = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        _STRUCT.append((len(lens), idx, user, item))
    return _STRUCT[0]


def rating_values(variant):
    """The fixture's ratings under a scale or `real`, in CSR order."""
    d1, idx, user, _ = structure()
    rng = np.random.default_rng(RATING_SEED + 100 * VARIANTS.index(variant))
    if variant == "real":
        return sd.SCALES["five"][rng.integers(0, 5, user.shape[0])] + rng.uniform(-0.49, 0.49, user.shape[0])
    if variant != "mixed":
        pool = sd.SCALES[variant]
        return pool[rng.integers(0, len(pool), user.shape[0])]
    val = np.empty(user.shape[0])
    for u in range(d1):
        pool = sd.SCALES[sd.MIXED[u % 4]]
        val[idx[u]:idx[u + 1]] = pool[rng.integers(0, len(pool), int(idx[u + 1] - idx[u]))]
    return val


def case(variant, solver, r):
    """A Case like scale_data.scale_case on this structure: the full shard, with the factors of rank r (the same for every variant
    and both solvers, so that a user's rows are the same in every cell of a rank)."""
    c = ed.Case()
    c.variant, c.r, c.solver, c.lam = variant, int(r), int(solver), LAMBDA
    c.d1, c.idx, c.user, c.item = structure()
    c.d2 = D2
    c.val = rating_values(variant)
    rng = np.random.default_rng(FACTOR_SEED + r)
    dens = ed.density(r)
    c.U = ed.dyadic_matrix(rng, c.d1, r, dens)
    c.V = ed.dyadic_matrix(rng, c.d2, r, dens)
    c.lens = np.diff(c.idx)
    c.users = np.arange(c.d1)                                    # this shard's users as rows of the full shard
    return c


def short_case(c):
    """The sub-shard of c's users of at most SHORT_MAX ratings, renumbered in order: same items, same V, the same rows of U."""
    keep = np.flatnonzero(c.lens <= SHORT_MAX)
    s = ed.Case()
    s.variant, s.r, s.solver, s.lam, s.d2, s.V = c.variant, c.r, c.solver, c.lam, c.d2, c.V
    s.users = keep
    s.d1 = len(keep)
    s.lens = c.lens[keep]
    s.idx = np.concatenate([[0], np.cumsum(s.lens)]).astype(np.int64)
    sel = np.concatenate([np.arange(c.idx[u], c.idx[u + 1]) for u in keep]).astype(np.int64)
    s.user = np.repeat(np.arange(s.d1), s.lens)
    s.item, s.val = c.item[sel], c.val[sel]
    s.U = c.U[keep].copy()
    return s


def level_counts(c):
    """Distinct levels per user of the case under its solver (0 for a user without ratings)."""
    return sd.level_counts(c.idx, c.val, c.solver)
