"""Data sets of tests/test_ccd_implicit.py: small enough that the dense form of the unrated cells is cheap (4200 x 40 cells at most).

long_set():   4200 users x 40 items, item-long.  Nine items have exactly 0, 1, 2, 63, 64, 65, 4095, 4096 and 4097 ratings (both ends of
              the sweep's wave loop and both sides of ccd::LONG); two more items and five users are empty; one user has rated every
              item that anyone rated (its row has no unrated cell but the empty items'; with empty items in the set no row can be
              fuller).  Edge ids are scattered over the id range.  Ratings are seeded integers 1..5.  The short test set holds
              entries of an empty user, of an empty item and of the longest item.
wide_set():   its transpose (user-long): the same cells, users and items exchanged.
full_set():   12 x 9 with every cell rated.
"""
import functools

import numpy as np

from primalcr_amd import synth

LONG_DEGREES = (0, 1, 2, 63, 64, 65, 4095, 4096, 4097)
D_LONG, D_SHORT = 4200, 40
N_EMPTY_LONG, N_EMPTY_SHORT = 5, 2                                         # empty users; empty items besides the degree-0 one


@functools.lru_cache(maxsize=None)
def long_set(seed=31):
    """-> (Ratings, item_of, empty_users, empty_items, full_user)"""
    rng = np.random.default_rng(seed)
    users = rng.permutation(D_LONG)
    empty_users, full_user, pool = np.sort(users[:N_EMPTY_LONG]), int(users[N_EMPTY_LONG]), users[N_EMPTY_LONG + 1:]
    items = rng.permutation(D_SHORT)
    item_of = {L: int(j) for L, j in zip(LONG_DEGREES, items)}
    extra_empty = items[len(LONG_DEGREES):len(LONG_DEGREES) + N_EMPTY_SHORT]
    rest = items[len(LONG_DEGREES) + N_EMPTY_SHORT:]
    us, it = [], []
    degrees = [(item_of[L], L) for L in LONG_DEGREES] + [(int(j), int(rng.integers(30, 300))) for j in rest]
    for j, L in degrees:
        if L == 0:
            continue
        raters = np.concatenate([[full_user], rng.choice(pool, L - 1, replace=False)])
        us.append(raters); it.append(np.full(L, j))
    us, it = np.concatenate(us), np.concatenate(it)
    o = np.lexsort((it, us))
    us, it = us[o].astype(np.int32), it[o].astype(np.int32)
    assert np.unique(us.astype(np.int64) * D_SHORT + it).shape[0] == us.shape[0]
    val = rng.integers(1, 6, us.shape[0]).astype(np.float64)
    empty_items = np.sort(np.concatenate([[item_of[0]], extra_empty]))
    tu = np.concatenate([np.full(4, empty_users[0]), rng.integers(0, D_LONG, 4), rng.integers(0, D_LONG, 4), rng.integers(0, D_LONG, 28)])
    ti = np.concatenate([rng.integers(0, D_SHORT, 4), np.full(4, item_of[0]), np.full(4, item_of[4097]), rng.integers(0, D_SHORT, 28)])
    o = np.argsort(tu, kind="stable")
    tv = rng.integers(1, 6, tu.shape[0]).astype(np.float64)
    R = synth.Ratings(D_LONG, D_SHORT, us, it, val, tu[o].astype(np.int32), ti[o].astype(np.int32), tv)
    return R, item_of, empty_users, empty_items, full_user


@functools.lru_cache(maxsize=None)
def wide_set():
    """-> (Ratings, user_of, empty_users, empty_items, full_item): long_set with users and items exchanged."""
    R, item_of, empty_users, empty_items, full_user = long_set()
    o = np.lexsort((R.user, R.item))
    t = np.argsort(R.titem, kind="stable")
    W = synth.Ratings(R.d2, R.d1, R.item[o].copy(), R.user[o].copy(), R.val[o].copy(), R.titem[t].copy(), R.tuser[t].copy(), R.tval[t].copy())
    return W, item_of, empty_items, empty_users, full_user


@functools.lru_cache(maxsize=None)
def full_set(seed=37):
    rng = np.random.default_rng(seed)
    d1, d2 = 12, 9
    us, it = np.divmod(np.arange(d1 * d2), d2)
    val = rng.integers(1, 6, d1 * d2).astype(np.float64)
    tu = np.sort(rng.integers(0, d1, 10)).astype(np.int32)
    return synth.Ratings(d1, d2, us.astype(np.int32), it.astype(np.int32), val, tu, rng.integers(0, d2, 10).astype(np.int32),
                         rng.integers(1, 6, 10).astype(np.float64))


def completed(R, w, alpha):
    """The set with every unrated cell added as a rating 0 of weight alpha (user-major, items ascending) -> (Ratings, weights)."""
    wd = np.full((R.d1, R.d2), float(alpha))
    vd = np.zeros((R.d1, R.d2))
    wd[R.user, R.item] = 1.0 if w is None else w
    vd[R.user, R.item] = R.val
    us, it = np.divmod(np.arange(R.d1 * R.d2), R.d2)
    C = synth.Ratings(R.d1, R.d2, us.astype(np.int32), it.astype(np.int32), vd.ravel(), R.tuser, R.titem, R.tval)
    return C, wd.ravel()
