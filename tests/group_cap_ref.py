"""The reference of the group cap (include/primalcr.h, "group-capped top-K lists"), in plain numpy / Python.

ref_capped applies the contract to the pools recommend() returns with K = pool; ref_capped_full walks a user's whole eligible
catalogue in recommendation order (descending score, equal scores by ascending item id) and knows no pool at all.  The
contract's exactness claim ties the two: a status-0 row of ref_capped is the row of ref_capped_full, a status-1 row is a prefix
of it (test_group_cap.py holds that on random tied scores, and on the device).
"""
import numpy as np

CAP_EXACT, CAP_POOL_EXHAUSTED = 0, 1


def walk(order_items, order_scores, groups, cap, topk, by_kept=False):
    """The rule over one user's entries in recommendation order: (kept items, their scores), at most topk.  An entry is kept iff
    its group id is negative or fewer than cap EARLIER entries (kept or not; by_kept: kept ones only) have the same group id."""
    seen = {}
    items, scores = [], []
    for j, s in zip(order_items, order_scores):
        g = int(groups[j])
        keep = g < 0 or seen.get(g, 0) < cap
        if g >= 0 and (keep or not by_kept):
            seen[g] = seen.get(g, 0) + 1
        if keep:
            items.append(int(j)); scores.append(s)
            if len(items) == topk:
                break
    return items, scores


def ref_capped(pool_items, pool_scores, groups, cap, topk, by_kept=False):
    """The contract applied to the pools (rows of recommend() with K = pool, padding included): (items int32 [n, topk], scores
    [n, topk], status uint8 [n])."""
    n, P = pool_items.shape
    items = np.full((n, topk), -1, np.int32); scores = np.full((n, topk), -np.inf); status = np.zeros(n, np.uint8)
    for i in range(n):
        L = int((pool_items[i] >= 0).sum())
        assert np.all(pool_items[i, L:] == -1)
        it, sc = walk(pool_items[i, :L], pool_scores[i, :L], groups, cap, topk, by_kept)
        items[i, :len(it)] = it; scores[i, :len(it)] = sc
        status[i] = CAP_EXACT if (len(it) == topk or L < P) else CAP_POOL_EXHAUSTED
    return items, scores, status


def ref_capped_full(scores_row, eligible, groups, cap, topk):
    """The group-capped top-topk of one user's whole eligible catalogue: scores_row [d2], eligible bool [d2]; (items, scores)
    lists of at most topk entries."""
    elig = np.nonzero(eligible)[0]
    s = scores_row[elig]
    o = np.lexsort((elig, -s))
    return walk(elig[o], s[o], groups, cap, topk)


def stats_of(items, status):
    """pcr_cap_stats from finished rows."""
    length = (items >= 0).sum(1)
    return dict(users=int(items.shape[0]), exact=int((status == CAP_EXACT).sum()), exhausted=int((status == CAP_POOL_EXHAUSTED).sum()),
                short_rows=int((length < items.shape[1]).sum()), kept=int(length.sum()))
