"""Brute-force numpy definitions of the filtered evaluation (include/primalcr.h, "filtered evaluation": pcr_evaluate_topn_filtered,
pcr_evaluate_ranks_filtered, pcr_sample_negatives) on a dense score matrix, for tests/test_filtered_eval.py.  Nothing here is
shared with the library: the eligibility sets are dense boolean rows, the ranks are counted item by item."""
import numpy as np

MASK64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def eligible(d1, d2, allow=None, candidates=None):
    """F[u, j]: item j is in F_u -- in u's candidate row (candidates None: every item) with allow[j] nonzero (None: all)."""
    F = np.ones((d1, d2), bool)
    if candidates is not None:
        cptr, citem = candidates
        F[:] = False
        for u in range(d1):
            F[u, citem[cptr[u]:cptr[u + 1]]] = True
    if allow is not None:
        F &= (np.asarray(allow) != 0)[None, :]
    return F


def train_mask(d1, d2, exclude):
    M = np.zeros((d1, d2), bool)
    if exclude is not None:
        index, item = exclude
        for u in range(d1):
            M[u, item[index[u]:index[u + 1]]] = True
    return M


def restrict_test(F, tindex, titem, tval):
    """The test CSR with every rating whose item is outside F_u struck out; also the kept positions."""
    d1 = F.shape[0]
    keep = np.zeros(titem.shape[0], bool)
    for u in range(d1):
        z = np.arange(tindex[u], tindex[u + 1])
        keep[z] = F[u, titem[z]]
    ptr = np.zeros(d1 + 1, np.int64)
    for u in range(d1):
        ptr[u + 1] = ptr[u] + int(keep[tindex[u]:tindex[u + 1]].sum())
    return (ptr, np.ascontiguousarray(titem[keep]), np.ascontiguousarray(tval[keep])), np.nonzero(keep)[0]


def ref_lists(S, F, exclude, K):
    """The K best of F_u minus the training row, descending score, equal scores by ascending id, padded with -1."""
    d1, d2 = S.shape
    T = train_mask(d1, d2, exclude)
    items = np.full((d1, K), -1, np.int32)
    for u in range(d1):
        el = np.nonzero(F[u] & ~T[u])[0]
        o = np.lexsort((el, -S[u, el]))[:K]
        items[u, :o.shape[0]] = el[o]
    return items


def ref_ranks(S, F, exclude, tindex, titem, tval, threshold):
    """(ranks[tnnz], per_user[d1, 5], summary, |R_u^f| per user): rank_u(j) = 1 + #{i in N_u^f before j} + #{j' in R_u^f before j}."""
    d1, d2 = S.shape
    T = train_mask(d1, d2, exclude)
    ids = np.arange(d2)
    ranks = np.zeros(titem.shape[0], np.int64)
    per = np.full((d1, 5), np.nan)
    nrel = np.zeros(d1, np.int64)
    for u in range(d1):
        z = np.arange(tindex[u], tindex[u + 1])
        z = z[(tval[z] >= threshold) & F[u, titem[z]]]
        if z.shape[0] == 0:
            continue
        rel = np.unique(titem[z])
        isrel = np.zeros(d2, bool); isrel[rel] = True
        nonrel = F[u] & ~isrel & ~T[u]
        s = S[u]
        rk, right = {}, 0
        for j in rel:
            before = (s > s[j]) | ((s == s[j]) & (ids < j))
            rk[int(j)] = 1 + int((before & nonrel).sum()) + int((before & isrel).sum())
            right += int((~before & nonrel).sum())
        ranks[z] = [rk[int(j)] for j in titem[z]]
        R, N, tot = len(rk), int(nonrel.sum()), sum(rk.values())
        first = min(rk.values())
        per[u] = (first, 1.0 / first, tot / R, right / (R * N) if N else np.nan, (tot - R) / (R * (N + R - 1)) if N + R > 1 else 0.0)
        nrel[u] = R
    c = ~np.isnan(per[:, 0])
    a = c & ~np.isnan(per[:, 3])
    n, na = int(c.sum()), int(a.sum())
    mean = lambda x, k: float(x.sum()) / k if k else 0.0
    summary = dict(users=n, users_auc=na, relevant=int(nrel.sum()), mrr=mean(per[c, 1], n), mean_rank=mean(per[c, 2], n),
                   auc=mean(per[a, 3], na), mpr=mean(per[c, 4], n))
    return ranks, per, summary, nrel


def mix(x):
    x &= MASK64
    x ^= x >> 30; x = (x * 0xBF58476D1CE4E5B9) & MASK64
    x ^= x >> 27; x = (x * 0x94D049BB133111EB) & MASK64
    x ^= x >> 31
    return x


def ref_sample_negatives(d2, tindex, titem, train=None, n_neg=99, seed=0, include_test=True, first_user=0):
    """The rule of pcr_sample_negatives restated with Python integers: (index, item)."""
    rows = tindex.shape[0] - 1
    out = []
    for u in range(rows):
        test = set(int(j) for j in titem[tindex[u]:tindex[u + 1]])
        if not test:
            out.append([]); continue
        tr = set() if train is None else set(int(j) for j in train[1][train[0][u]:train[0][u + 1]])
        pool = [j for j in range(d2) if j not in tr and j not in test]
        inpool = set(pool)
        m = min(n_neg, len(pool))
        key = mix(seed + GOLDEN * (first_user + u + 1))
        want = 0 if m == len(pool) else m if 2 * m <= len(pool) else len(pool) - m
        drawn, t = [], 0
        while len(drawn) < want:
            j = mix(key + GOLDEN * (t + 1)) % d2
            t += 1
            if j in inpool and j not in drawn:
                drawn.append(j)
        neg = set(drawn) if (m != len(pool) and 2 * m <= len(pool)) else inpool - set(drawn)
        assert len(neg) == m
        out.append(sorted(neg | (test if include_test else set())))
    index = np.zeros(rows + 1, np.int64)
    index[1:] = np.cumsum([len(r) for r in out])
    return index, np.array([j for r in out for j in r], np.int32)
