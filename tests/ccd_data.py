"""Data sets of the CCDR1 tests (tests/test_ccd.py, tests/test_ccd_reference.py) and of their goldens (tools/make_ccd_golden.py)."""
import os

import numpy as np

from primalcr_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SYNTH_SEEDS = {"synth3": 3, "synth4": 4}


def unsorted_test_set():
    """A small seeded set whose test file is NOT user-sorted: in every fourth pair of neighbouring users (with no item in common) the
    second one's entries come first.  The reference's convert() puts the first user's entries into the second one's row (the row
    of the largest user seen so far), while the printed rmse walks the file's own triplets (util.cpp:206-215).  (No row gets an
    item twice: equal scores would make NDCG depend on std::sort's order of ties, which the reference leaves unspecified.)"""
    R = synth.generate("small", seed=5, d1=200, d2=120, nnz=4000)
    rows = [np.flatnonzero(R.tuser == u) for u in range(R.d1)]
    order, swapped = [], 0
    for u in range(0, R.d1 - 1, 2):
        a, b = rows[u], rows[u + 1]
        if u % 8 == 0 and len(a) and len(b) and not set(R.titem[a]) & set(R.titem[b]):
            order += [b, a]; swapped += 1
        else:
            order += [a, b]
    if R.d1 % 2:
        order.append(rows[-1])
    p = np.concatenate(order)
    assert swapped > 0 and p.shape[0] == R.tuser.shape[0]
    return synth.Ratings(R.d1, R.d2, R.user, R.item, R.val, R.tuser[p], R.titem[p], R.tval[p])


def long_column_set():
    """Users and items beyond the sweeps' 4096-rating bound (a workgroup per column): user 0 rates 4300 items, item 0 is rated by
    all 4600 users, every other user rates three more items."""
    d1, d2 = 4600, 4400
    rng = np.random.default_rng(9)
    pairs = {(0, j) for j in range(4300)} | {(u, 0) for u in range(d1)}
    for u in range(1, d1):
        pairs |= {(u, int(j)) for j in rng.choice(np.arange(1, d2), 3, replace=False)}
    pr = np.array(sorted(pairs), np.int32)
    val = rng.integers(1, 6, pr.shape[0]).astype(np.float64)
    tu = np.repeat(np.arange(0, d1, 5, dtype=np.int32), 2)
    ti = rng.integers(0, d2, tu.shape[0]).astype(np.int32)
    tv = rng.integers(1, 6, tu.shape[0]).astype(np.float64)
    return synth.Ratings(d1, d2, pr[:, 0].copy(), pr[:, 1].copy(), val, tu, ti, tv)


# ------------------------------------------------------------------------------------------------ tests/test_ccd_reference.py
# column lengths at the sweep's edges: empty, a wave (64), two waves, a workgroup's stride (256), the one-wave / workgroup class
# bound (4096: ccd::LONG), a workgroup column of 17 passes and one whose last pass is short
EDGE_LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 4095, 4096, 4097, 4352, 8200)
EDGE_FILL = 8200


def edge_set(seed=17, values=None):
    """-> (Ratings, user_of, item_of): for every L of EDGE_LENGTHS one user (user_of[L]) and one item (item_of[L]) with exactly L
    ratings.  The edge users rate "filler" items only and the edge items are rated by filler users only, so the lengths do not
    disturb each other; every filler user rates 2 more filler items.  Edge ids are scattered over the id range.  Ratings are
    seeded integers 1..5, or `values` everywhere.  The test set (user-sorted) holds entries of the empty user, of the empty item
    and of the longest user and item."""
    rng = np.random.default_rng(seed)
    n_edge = len(EDGE_LENGTHS)
    d = EDGE_FILL + n_edge

    def side():
        ids = rng.permutation(d)
        edge = ids[:n_edge]
        fill = np.sort(ids[n_edge:])
        return {L: int(e) for L, e in zip(EDGE_LENGTHS, edge)}, fill
    user_of, ufill = side()
    item_of, ifill = side()
    us, it = [], []
    for L in EDGE_LENGTHS:
        us.append(np.full(L, user_of[L])); it.append(rng.choice(ifill, L, replace=False))
        us.append(rng.choice(ufill, L, replace=False)); it.append(np.full(L, item_of[L]))
    a = rng.integers(0, EDGE_FILL, EDGE_FILL)
    b = (a + rng.integers(1, EDGE_FILL, EDGE_FILL)) % EDGE_FILL            # a second, different filler item
    us += [ufill, ufill]; it += [ifill[a], ifill[b]]
    us, it = np.concatenate(us), np.concatenate(it)
    o = np.lexsort((it, us))
    us, it = us[o].astype(np.int32), it[o].astype(np.int32)
    assert np.unique(us.astype(np.int64) * d + it).shape[0] == us.shape[0]
    val = rng.integers(1, 6, us.shape[0]).astype(np.float64) if values is None else np.full(us.shape[0], float(values))
    Lmax = EDGE_LENGTHS[-1]
    tu = np.concatenate([np.full(8, user_of[0]), np.full(8, user_of[Lmax]), rng.integers(0, d, 8), rng.integers(0, d, 8),
                         rng.integers(0, d, 300)])
    ti = np.concatenate([rng.integers(0, d, 8), rng.integers(0, d, 8), np.full(8, item_of[0]), np.full(8, item_of[Lmax]),
                         rng.integers(0, d, 300)])
    o = np.argsort(tu, kind="stable")
    tv = rng.integers(1, 6, tu.shape[0]).astype(np.float64)
    return synth.Ratings(d, d, us, it, val, tu[o].astype(np.int32), ti[o].astype(np.int32), tv), user_of, item_of


def fixed_point_set():
    """edge_set's structure with every rating equal to 2.  With U0 = 1, lambda = 1, k = 1 every non-empty item gets
    v = 2n / (n + n) = 1 exactly and every non-empty user then u = 1: the residual is 1 everywhere, loss = nnz, reg = 2 nnz,
    obj = 3 nnz in every inner and outer iteration, in fp32 and in fp64, whatever the order of the sums (every partial sum is a
    small integer).  One dropped or doubled rating in either sweep gives (2n - 2) / (2n - 1) != 1."""
    return edge_set(values=2)


def dyadic_first_sweep(k, seed=23):
    """-> (Ratings, user_of, item_of, U0, lambda): edge_set with U0 in {0, +-1/4, +-1/2, +-1} and lambda = 1/2.  In the first item
    sweep g (a multiple of 1/4 below 2^16) and h (a multiple of 1/16) are exact in any order: v = g / h is one correctly rounded
    division."""
    R, user_of, item_of = edge_set()
    rng = np.random.default_rng(seed)
    U0 = rng.choice(np.array([0.0, 0.25, -0.25, 0.5, -0.5, 1.0, -1.0]), (R.d1, k))
    return R, user_of, item_of, U0, 0.5


def big_set(seed=29):
    """270 000 x 270 000, about 1.1 M ratings (above 1 048 576: the element-wise segments run at their block cap), every user and
    every item rated (a diagonal and a second, strided one, then random fill), a test set of one triplet per user (above
    262 144): every fixed-order sum runs over more than one block's worth of partials."""
    d = 270_000
    rng = np.random.default_rng(seed)
    i = np.arange(d, dtype=np.int64)
    key = np.concatenate([i * d + i, i * d + (3 * i + 1) % d,                # (3 i + 1 = i mod d has no solution: d is even)
                          rng.integers(0, d, 580_000) * d + rng.integers(0, d, 580_000)])
    key = np.unique(key)
    us, it = (key // d).astype(np.int32), (key % d).astype(np.int32)
    val = rng.integers(1, 6, key.shape[0]).astype(np.float64)
    ti = rng.integers(0, d, d).astype(np.int32)
    tv = rng.integers(1, 6, d).astype(np.float64)
    return synth.Ratings(d, d, us, it, val, i.astype(np.int32), ti, tv)


def ratings(name):
    if name in SYNTH_SEEDS:
        return synth.generate("small", seed=SYNTH_SEEDS[name], d1=200, d2=120, nnz=4000)
    if name == "unsorted":
        return unsorted_test_set()
    if name == "long":
        return long_column_set()
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    return synth.Ratings(int(g["d1"]), int(g["d2"]), g["user"], g["item"], g["val"], g["tuser"], g["titem"], g["tval"])
