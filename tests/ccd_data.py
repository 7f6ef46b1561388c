"""Data sets of the CCDR1 tests (tests/test_ccd.py) and of their goldens (tools/make_ccd_golden.py)."""
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


def ratings(name):
    if name in SYNTH_SEEDS:
        return synth.generate("small", seed=SYNTH_SEEDS[name], d1=200, d2=120, nnz=4000)
    if name == "unsorted":
        return unsorted_test_set()
    if name == "long":
        return long_column_set()
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    return synth.Ratings(int(g["d1"]), int(g["d2"]), g["user"], g["item"], g["val"], g["tuser"], g["titem"], g["tval"])
