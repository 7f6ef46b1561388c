"""Item-degree edges for the ranking solver's V step (tests/test_item_edges.py): a rating set designed BY ITEM, with the dyadic
factors of tests/exact_data.py, the integer definition of the Hessian-vector product, and a numpy restatement of the cutting rule
of the SpMM plan (pcr_plan.h) that tells which edge of k_spmm / k_spmm_fin a launch configuration reaches.

Every other fixture of the V step draws each user's items uniformly, so item degrees are flat (3 .. 29 on test_gpu_parity._mixed_set)
and no item is empty.  Here (640 users, 1031 items -- a prime: no multiple of a chunk, a tile count, a range count or a lane group):

    item 0                  rated by every user (a partial row from every tile and every shard)
    item 1, item d2-1       no rating (item_slot[j] == item_slot[j+1]; the last one sits at the end of the table)
    items 2 .. 399          28 ladder items (every 10th from 10 on) among seeded degrees 0 .. 6
    items 400 .. 447        no rating: with 64 item ranges (16 items each) the ranges [402, 418) and [418, 434) are empty
    items 448 .. 599        seeded degrees 0 .. 6
    items 600 .. 919        exactly one rating each, by the even users in turn: consecutive entries of the tile-major CSC, every
                            one of them a new item
    items 920 .. 1028       seeded degrees 0 .. 6
    item d2-2               one rating, by the last user

The ladder's degrees are LADDER; its rungs alternate between a contiguous run of users (one tile, one shard) and a random set
(all of them).  Two dense users (5 and 633) rate every item that has a rating -- user 5 from degree 1 on, user 633 from degree 2 on,
both counted IN the degree -- except the singles block (a chunk there must be all-new at a tile) and item d2-2: they are the dense
rows of the blocked-user V step and the only users beyond 512 ratings.
"""
import numpy as np

import exact_data as ed

D1, D2 = 640, 1031
DENSE = (5, 633)
LADDER = (7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513, D1 - 1)
LADDER_ITEMS = tuple(range(10, 10 + 10 * len(LADDER), 10))
EMPTY_RUN = (400, 448)
SINGLES = (600, 920)
STRUCTURE_SEED = 4242


def item_degrees():
    """The designed degree of every item (what np.bincount(item) of the fixture must return)."""
    rng = np.random.default_rng(STRUCTURE_SEED)
    deg = rng.integers(0, 7, D2)
    deg[0] = D1
    deg[1] = deg[D2 - 1] = 0
    deg[list(LADDER_ITEMS)] = LADDER
    deg[EMPTY_RUN[0]:EMPTY_RUN[1]] = 0
    deg[SINGLES[0]:SINGLES[1]] = 1
    deg[D2 - 2] = 1
    return deg


def _structure():
    """(user, item) of every rating, sorted by user then item."""
    deg = item_degrees()
    rng = np.random.default_rng(STRUCTURE_SEED + 1)
    plain = np.setdiff1d(np.arange(D1), DENSE)
    contiguous = {j: q % 2 == 0 for q, j in enumerate(LADDER_ITEMS)}
    users, items = [], []
    for j in range(D2):
        n = int(deg[j])
        if n == 0:
            continue
        if j == 0:
            who = np.arange(D1)
        elif SINGLES[0] <= j < SINGLES[1]:
            who = np.array([2 * (j - SINGLES[0])])                            # even users 0, 2, .. 638: never a dense one
        elif j == D2 - 2:
            who = np.array([D1 - 1])
        else:
            dense = np.array(DENSE[:min(n, 2)])
            rest = n - dense.size
            if contiguous.get(j, False):                                        # a run of plain users from a seeded start
                s = int(rng.integers(0, plain.size - rest + 1))
                who = np.concatenate([dense, plain[s:s + rest]])
            else:
                who = np.concatenate([dense, rng.choice(plain, rest, replace=False)])
        users.append(who); items.append(np.full(who.size, j))
    user = np.concatenate(users).astype(np.int64); item = np.concatenate(items).astype(np.int64)
    o = np.lexsort((item, user))
    return user[o], item[o]


def item_edge_case(r, solver, real=False):
    """A Case like exact_data.dyadic_case -- the same dyadic U, V, a, a2, lambda = 32 and density(r) -- on the item-edge rating
    structure.  Ratings are seeded integers 1 .. 5; real: moved off the integers inside their lround bucket."""
    c = ed.Case()
    c.r, c.solver, c.seed, c.real, c.lam = int(r), int(solver), 0, bool(real), ed.LAMBDA
    c.d1, c.d2 = D1, D2
    c.user, c.item = _structure()
    c.val = np.random.default_rng(STRUCTURE_SEED + 2).integers(1, 6, c.user.shape[0]).astype(np.float64)
    rng = np.random.default_rng(77000 + 10 * r + solver)
    if real:
        c.val = c.val + rng.uniform(-0.49, 0.49, c.val.shape[0])
    dens = ed.density(r)
    c.U = ed.dyadic_matrix(rng, c.d1, r, dens)
    c.V = ed.dyadic_matrix(rng, c.d2, r, dens)
    c.a = ed.dyadic_matrix(rng, c.d2, r, dens)
    c.a2 = ed.dyadic_matrix(rng, c.d2, r, 1.0 if r <= 12 else 0.5)
    c.deg = np.bincount(c.item, minlength=c.d2)
    return c


def brute_force_Ha(c, idx, item, val, a, block=512, levels=None):
    """The definition of the Hessian-vector product, in integers, beside exact_data.brute_force (levels: each rating's level, in
    CSR order; None: exact_data.levels_of(val, c.solver)).  With M = 4 m, U2 = 2 U, A2 = 2 a
    and S = 4 (u . a) = U2[u] . A2[item] per rating:
        4 Ha[item_j] += (S_j - S_k) U2[u],  4 Ha[item_k] -= (S_j - S_k) U2[u]   for every active pair level_j > level_k,
        4 Ha += 2 lambda A2
    A pair is active when it lies inside the hinge: 4 - (M_j - M_k) > 0 for PrimalCR (solver 1: `mask < 1.0`), >= 0 for PrimalCR++
    (solver 2: its sweep takes the window CLOSED, m_k >= m_j - 1 and m_j <= m_k + 1 -- a pair exactly on the kink adds nothing to
    the objective and the gradient, but counts in the generalised Hessian; on dyadic scores such pairs are common, so the
    convention is part of what is checked).  Returns 4 Ha, int64."""
    U2 = np.rint(2 * c.U).astype(np.int64); A2 = np.rint(2 * np.asarray(a)).astype(np.int64); V2 = np.rint(2 * c.V).astype(np.int64)
    assert np.array_equal(U2, 2 * c.U) and np.array_equal(A2, 2 * np.asarray(a)) and np.array_equal(V2, 2 * c.V)
    lam2 = int(2 * c.lam)
    assert lam2 == 2 * c.lam
    d1 = len(idx) - 1
    ru = np.repeat(np.arange(d1), np.diff(idx))
    M = (U2[ru] * V2[item]).sum(1)
    S = (U2[ru] * A2[item]).sum(1)
    lev = ed.levels_of(val, c.solver) if levels is None else np.asarray(levels)
    Ha4 = lam2 * A2
    for u in range(d1):
        s, e = int(idx[u]), int(idx[u + 1])
        if e - s < 2:
            continue
        Mu = M[s:e]; Su = S[s:e]; Lu = lev[s:e]
        t = np.zeros(e - s, np.int64)
        for b0 in range(0, e - s, block):
            b1 = min(b0 + block, e - s)
            above = Lu[b0:b1, None] > Lu[None, :]                                   # rows j (higher level) x columns k
            D = ed.UNIT - (Mu[b0:b1, None] - Mu[None, :])
            act = above & ((D >= 0) if c.solver == 2 else (D > 0))
            W = np.where(act, Su[b0:b1, None] - Su[None, :], 0)
            t[b0:b1] += W.sum(1)
            t -= W.sum(0)
        np.add.at(Ha4, item[s:e], t[:, None] * U2[u][None, :])
    return Ha4


def plan_shape(idx, item, d2, ntiles, chunk, n_rng, exclude=()):
    """The documented cutting rule of pcr_plan.h, restated to CHOOSE the fixture's coverage (it does not test the plan): tile
    boundaries by lower_bound(uptr, nnz t / ntiles) (the cap on a tile's users is far away at these sizes), inside a tile the
    entries ordered by item then user, chunks of `chunk` entries that never straddle a tile or an item range
    [d2 r / n_rng, d2 (r + 1) / n_rng); a new-item flag on every entry whose item differs from its predecessor's, except a chunk's
    first; one slab slot per (chunk, item) incidence.  exclude: users the blocked-user V step takes out of the chunks.
    Returns what the kernels' edges depend on."""
    idx = np.asarray(idx, np.int64); item = np.asarray(item, np.int64)
    nu, nnz = len(idx) - 1, int(idx[-1])
    ntiles = max(1, min(int(ntiles), max(nu, 1)))
    n_rng = max(1, min(int(n_rng), 64, d2))
    tile_u = [0]
    for t in range(1, ntiles):
        u = int(np.searchsorted(idx, nnz * t // ntiles, side="left"))
        tile_u.append(min(max(u, tile_u[-1]), nu))
    tile_u = np.array(tile_u + [nu])
    rng_item = np.array([d2 * r // n_rng for r in range(n_rng + 1)])
    user = np.repeat(np.arange(nu), np.diff(idx))
    keep = ~np.isin(user, np.asarray(exclude, np.int64))
    user, it = user[keep], item[keep]
    tile = np.searchsorted(tile_u[:-1], user, side="right") - 1                 # largest t with tile_u[t] <= u
    rng = np.searchsorted(rng_item[:-1], it, side="right") - 1
    o = np.lexsort((user, it, tile))
    it, tile, rng = it[o], tile[o], rng[o]
    n = it.size
    grp = tile * n_rng + rng                                                    # ascending along the sorted entries
    first_of_grp = np.ones(n, bool); first_of_grp[1:] = grp[1:] != grp[:-1]
    grp_start = np.maximum.accumulate(np.where(first_of_grp, np.arange(n), 0))
    off = (np.arange(n) - grp_start) % chunk                                    # position inside the chunk
    chunk_first = off == 0
    new_item = np.ones(n, bool); new_item[1:] = (it[1:] != it[:-1]) | (tile[1:] != tile[:-1])
    flag = new_item & ~chunk_first
    cstart = np.flatnonzero(chunk_first)
    clen = np.diff(np.append(cstart, n))
    cid = np.cumsum(chunk_first) - 1
    nflag = np.bincount(cid[flag], minlength=cstart.size)
    full = clen == chunk
    last = np.zeros(n, bool); last[cstart + clen - 1] = True
    occupied = np.unique(grp).size
    return dict(
        ntiles=ntiles, chunk=int(chunk), n_rng=n_rng, nchunks=int(cstart.size), slab_rows=int((chunk_first | flag).sum()),
        inside=int((full & (nflag == 0) & ~new_item[cstart]).sum()),          # full chunks wholly inside a column begun earlier
        all_new=int((full & (nflag == chunk - 1) & new_item[cstart]).sum()),    # full chunks whose every entry starts an item
        slot_counts=set(np.bincount(it[chunk_first | flag], minlength=d2).tolist()),
        short_last=set(clen[~full].tolist()),
        flag_on_32=bool((flag & (off % 32 == 0)).any()), flag_on_64=bool((flag & (off % 64 == 0)).any()),
        flag_on_last=bool((flag & last).any()),
        empty_tile_range=ntiles * n_rng - int(occupied) > 0,             # a (tile, range) without entries: no chunk at all
        empty_range=np.unique(rng).size < n_rng,                           # a whole range without entries: k_spmm_fin alone
    )
