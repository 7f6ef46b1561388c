"""Rating scales for the exact-parity method (tests/test_rating_scales.py): one small rating structure that still reaches every
user-length class, the dyadic factors of tests/exact_data.py, and the ratings drawn from fifteen scales whose level counts select
the host route of pcr_build_levels (presence mask / insertion / sort), the window-cache form (ws = levels - 1 for 2..9 levels,
the unrolled path at exactly 5, searching sweeps otherwise), the LDS sizes (rs_cap = levels + 2) and the Gram cut (> 64 levels).

    structure   d2 = 6000; one user per length in exact_data.CLASS_EDGES, one of 5000 ratings, 45 users of 3..200 ratings
                (65 users, about 25 000 ratings), items seeded
    factors     exact_data.dyadic_matrix with density(r); lambda = 32
    ratings     rating_values(scale): seeded draws from SCALES[scale]; `mixed` gives user u the scale MIXED[u % 4]

levels_of is the integer reference's bucketing: half away from zero for PrimalCR++ (what lround does), the raw double for PrimalCR.
"""
from fractions import Fraction

import numpy as np

import exact_data as ed

D2 = 6000
N_SHORT = 45
STRUCTURE_SEED = 9100
LAMBDA = ed.LAMBDA

# name -> the values a rating is drawn from (uniformly, seeded)
SCALES = {
    "five": np.arange(1.0, 6.0),                       # the control: the scale of every other exact test (ws = 4, the unrolled path)
    "one": np.array([3.0]),                            # 1 level: no comparable pair, ws = 0, g = lambda V exactly
    "binary": np.array([0.0, 1.0]),                    # ws = 1, a rating of 0
    "three": np.array([1.0, 3.0, 5.0]),                # ws = 2, gaps in the presence mask
    "four": np.arange(1.0, 5.0),                       # ws = 3, just below the unrolled path
    "six": np.arange(1.0, 7.0),                        # ws = 5, just above it
    "nine": np.arange(1.0, 10.0),                      # ws = 8, the last cached count
    "ten": np.arange(1.0, 11.0),                       # the first searching count
    "halfstar": np.arange(1, 11) * 0.5,                # PrimalCR++: 5 levels through the half-away rule; PrimalCR: 10, non-integer
    "signed": np.arange(-5, 6) * 0.5,                  # negative halves: -0.5 -> -1, -1.5 -> -2; PrimalCR++ merges -0.5 / -1.0 etc.
    "jester": np.arange(-10.0, 11.0),                  # 21 levels, a negative mask base
    "l64": np.arange(1.0, 65.0),                       # the last bit of the mask route; the Gram class still allowed
    "l65": np.arange(1.0, 66.0),                       # the first set off it, past 64 distinct (sort route); no Gram class
    "wide6": np.arange(0.0, 101.0, 20.0),              # 6 levels over a range >= 64: insertion route with ws = 5
    "percent": np.arange(0.0, 101.0),                  # 101 levels: sort route, searching sweeps, no Gram class
}
MIXED = ("one", "binary", "five", "nine")            # `mixed`: user u draws from SCALES[MIXED[u % 4]]
ALL_SCALES = tuple(SCALES) + ("mixed",)
# the shard's largest per-user level count under (PrimalCR++, PrimalCR): what the table of the test's docstring claims
MAX_LEVELS = {"five": (5, 5), "one": (1, 1), "binary": (2, 2), "three": (3, 3), "four": (4, 4), "six": (6, 6), "nine": (9, 9), "ten": (10, 10),
              "halfstar": (5, 10), "signed": (7, 11), "jester": (21, 21), "l64": (64, 64), "l65": (65, 65), "wide6": (6, 6),
              "percent": (101, 101), "mixed": (9, 9)}


def window_slots(max_levels):
    """ws of the class layout (pcr_classes.h, ustep_lds_images): a slot per other level for 2..9 levels, else the sweeps search."""
    return max_levels - 1 if 2 <= max_levels <= 9 else 0


def levels_of(val, solver):
    """What the two solvers compare: PrimalCR++ the rating rounded half away from zero -- where(v >= 0, floor(v + .5), ceil(v - .5))
    evaluated without the rounding of v + .5 (0.49999999999999994 + .5 is 1.0 in binary64, yet lround gives 0): |v| is split into
    floor and an exactly representable remainder, which is compared with a half -- PrimalCR the raw double."""
    v = np.asarray(val, np.float64)
    if solver != 2:
        return v
    a = np.abs(v)
    t = np.floor(a)
    return (np.sign(v) * (t + (a - t >= 0.5))).astype(np.int64)


def half_away_exact(v):
    """The same rule in rational arithmetic, for single doubles: the definition levels_of is held to."""
    q = Fraction(float(v))
    n = int(abs(q) + Fraction(1, 2))                                           # floor(|v| + 1/2): int() truncates a positive rational
    return n if q >= 0 else -n


_STRUCT = []


def structure():
    """(d1, idx int64[d1 + 1], user, item): users in the order CLASS_EDGES, 5000, the short ones; items seeded, ascending per user."""
    if not _STRUCT:
        rng = np.random.default_rng(STRUCTURE_SEED)
        lens = np.concatenate([ed.CLASS_EDGES, [5000], rng.integers(3, 201, N_SHORT)]).astype(np.int64)
        user = np.repeat(np.arange(len(lens)), lens)
        item = np.concatenate([np.sort(rng.choice(D2, int(n), replace=False)) for n in lens]).astype(np.int64)
        idx = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        _STRUCT.append((len(lens), idx, user, item))
    return _STRUCT[0]


def rating_values(scale, seed=0):
    """The fixture's ratings under a scale, in CSR order."""
    d1, idx, user, _ = structure()
    rng = np.random.default_rng(31000 + 100 * ALL_SCALES.index(scale) + seed)
    if scale != "mixed":
        pool = SCALES[scale]
        return pool[rng.integers(0, len(pool), user.shape[0])]
    val = np.empty(user.shape[0])
    for u in range(d1):
        pool = SCALES[MIXED[u % 4]]
        val[idx[u]:idx[u + 1]] = pool[rng.integers(0, len(pool), int(idx[u + 1] - idx[u]))]
    return val


def split_values(bounds, later, seed=0):
    """Ratings for the shard cells: the users of shard 0 (users [bounds[0], bounds[1])) draw from 1..5, every later shard from
    SCALES[later] -- shard 0 then runs at ws = 4 while the others, and the one-rank solver, run at the later scale's ws."""
    d1, idx, user, _ = structure()
    rng = np.random.default_rng(47000 + 100 * ALL_SCALES.index(later) + 10 * (len(bounds) - 1) + seed)
    five = SCALES["five"][rng.integers(0, 5, user.shape[0])]
    late = SCALES[later][rng.integers(0, len(SCALES[later]), user.shape[0])]
    return np.where(user < int(bounds[1]), five, late)


def scale_case(scale, solver, r, val=None):
    """A Case like exact_data.dyadic_case on the small structure, with the ratings of `scale` (or the given ones)."""
    c = ed.Case()
    c.scale, c.r, c.solver, c.lam = scale, int(r), int(solver), LAMBDA
    c.d1, idx, c.user, c.item = structure()
    c.d2 = D2
    c.val = rating_values(scale) if val is None else np.asarray(val, np.float64)
    rng = np.random.default_rng(52000 + 10 * r + solver)
    dens = ed.density(r)
    c.U = ed.dyadic_matrix(rng, c.d1, r, dens)
    c.V = ed.dyadic_matrix(rng, c.d2, r, dens)
    c.a = ed.dyadic_matrix(rng, c.d2, r, dens)
    c.a2 = ed.dyadic_matrix(rng, c.d2, r, 1.0 if r <= 12 else 0.5)
    return c


def level_counts(idx, val, solver):
    """Distinct levels per user (0 for a user without ratings), in numpy."""
    lev = levels_of(val, solver)
    return np.array([np.unique(lev[idx[u]:idx[u + 1]]).size for u in range(len(idx) - 1)], np.int64)


def all_pairs(idx, val, solver):
    """|Omega_u| per user by the definition: every ordered pair of the user's ratings whose first level is above the second."""
    lev = levels_of(val, solver)
    out = np.zeros(len(idx) - 1, np.int64)
    for u in range(len(idx) - 1):
        L = lev[idx[u]:idx[u + 1]]
        out[u] = int((L[:, None] > L[None, :]).sum())
    return out
