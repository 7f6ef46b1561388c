"""The fixture of the exact evaluator tests (tests/test_eval_exact.py): the smallest rating sets that reach every form of
k_eval / k_eval2, with dyadic factors (tests/exact_data.py) so that every score is exact in fp32 and in fp64 and ties abound.

Users: one per length of LENGTHS over D2 items -- the evaluator's class limits 128 / 512 / 4096 (pcr_classes.h, BIN_LIMIT) on
both sides, the power-of-two padding edges of k_eval2's sort, the empty user.  The TEST set holds the same lengths in reverse user
order on items disjoint from the user's training items: every long-training user is a short-test user and the reverse.
ZERO_USERS have an all-zero row of U: every score of theirs ties and the top-k is the index order.

Rating modes:
    int5   integers 1..5                      the training set shares the solver's level tables
    q10    integer + {0, 0.25}                10 raw values in 5 lround buckets: the evaluator's own tables under PrimalCR++
    d64    1 + i/16, i < 64, all 64 present   k_eval2 (LDS and global-scratch forms) at nlev == 64
    d65    1 + i/16, i < 65, all 65 present   the whole set falls to k_eval, the global-scratch instantiation included
Class groups keep the users of one evaluator class (by their length in the set in question) and empty the others.
"""
import functools

import numpy as np

import exact_data as ed

LENGTHS = (0, 1, 2, 3, 63, 64, 65, 128, 129, 255, 256, 257, 512, 513, 1023, 1024, 1025, 2048, 2049, 4095, 4096, 4097, 4150)
D1, D2 = len(LENGTHS), 4200
RANKS = (1, 12, 100)
KS = (1, 10, 100)
MODES = ("int5", "q10", "d64", "d65")
ZERO_USERS = (6, 16, 21)                         # training lengths 65, 1025, 4097; test lengths 1025, 65, 1
GROUPS = {"wave": (0, 128), "256": (129, 512), "512": (513, 4096), "scratch": (4097, 1 << 30), "all": (0, 1 << 30)}
SLOT = {"wave": "eval/64", "256": "eval/256", "512": "eval/512", "scratch": "eval/512g"}       # profile slot of each class


def group_of(n):
    return next(g for g, (lo, hi) in GROUPS.items() if lo <= n <= hi)


def _values(rng, mode, n):
    if mode == "int5":
        return rng.integers(1, 6, n).astype(np.float64)
    if mode == "q10":
        return rng.integers(1, 6, n) + 0.25 * rng.integers(0, 2, n)
    nlev = {"d64": 64, "d65": 65}[mode]
    lv = rng.integers(0, nlev, n)
    if n >= nlev:
        lv[:nlev] = np.arange(nlev)                                       # every value present, then shuffled
    return 1.0 + rng.permutation(lv) / 16.0


class EvalCase:
    pass


@functools.lru_cache(maxsize=None)
def eval_case(mode, r, group="all", seed=0):
    """The two CSRs (idx, item, val: items ascending per user), U [D1, r] and V [D2, r]; c.csr(which) picks one."""
    lo, hi = GROUPS[group]
    rng = np.random.default_rng(7000 + 100 * seed + MODES.index(mode))     # the ratings do not depend on r or on the group
    sets = [([0], [], []), ([0], [], [])]
    for u in range(D1):
        perm = rng.permutation(D2)
        n0, n1 = LENGTHS[u], LENGTHS[D1 - 1 - u]
        for w, (n, items) in enumerate(((n0, perm[:n0]), (n1, perm[n0:n0 + n1]))):
            vals = _values(rng, mode, n)                                   # drawn whether kept or not: groups share the ratings
            if not lo <= n <= hi:
                n, items, vals = 0, items[:0], vals[:0]
            idx, it, va = sets[w]
            idx.append(idx[-1] + n); it.append(np.sort(items)); va.append(vals)
    c = EvalCase()
    c.mode, c.r, c.group, c.d1, c.d2 = mode, int(r), group, D1, D2
    c.sets = [(np.asarray(idx, np.int64), np.concatenate(it).astype(np.int32), np.concatenate(va)) for idx, it, va in sets]
    frng = np.random.default_rng(9000 + 100 * seed + r)
    c.U = ed.dyadic_matrix(frng, D1, r, ed.density(r))
    c.V = ed.dyadic_matrix(frng, D2, r, ed.density(r))
    c.U[list(ZERO_USERS)] = 0.0
    return c


def csr(c, which):
    return c.sets[which]


def lengths(c, which):
    return np.diff(c.sets[which][0])


def triplets(c, which):
    idx, item, val = c.sets[which]
    return np.repeat(np.arange(c.d1), np.diff(idx)).astype(np.int32), item, val


def max_raw_levels(c, which):
    idx, _, val = c.sets[which]
    return max((len(np.unique(val[idx[u]:idx[u + 1]])) for u in range(c.d1)), default=0)
