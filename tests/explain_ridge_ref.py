"""Plain-numpy fp64 reference of explain_ridge() (include/primalcr.h, "explaining squared-loss recommendations"): per user the
regularised Gram matrix of its rated rows on the free set, np.linalg.cholesky / solve on the storage-rounded factors, and every
contribution e_p(j) = r_p (v_{i_p} . G^-1 v_j) as a dense [len, L_u] matrix in the sorted row's order."""
import numpy as np

OK, SINGULAR = 0, 1


def rounded(M, f32):
    """M as the storage type holds it, widened back to fp64."""
    M = np.asarray(M, np.float64)
    return M.astype(np.float32).astype(np.float64) if f32 else M


def sorted_row(ratings, i):
    """User i's row by ascending item id, equal items keeping their order: (items, ratings)."""
    index, item, val = ratings
    a, b = int(index[i]), int(index[i + 1])
    o = np.argsort(item[a:b], kind="stable")
    return np.asarray(item[a:b])[o], np.asarray(val[a:b], np.float64)[o]


def chol_solve(G, B):
    Lc = np.linalg.cholesky(G)
    return np.linalg.solve(Lc.T, np.linalg.solve(Lc, B))


def user_system(Fr, it, lam, weighted, P):
    """(G, mu) of a user with rated items `it` on the free coordinates P."""
    A = Fr[it][:, P]
    mu = lam * len(it) if weighted else lam
    return A.T @ A + mu * np.eye(len(P)), mu


def ref_user(Fr, it, r, uh, lst, lam, weighted=True, nonneg=False):
    """One user: uh its row as stored (None: the minimiser itself is explained), lst its non-padding list.  Returns a dict with
    e [len, L_u], score / residual / support / opposition [L_u], ustar, uh, mu, P, loss, dist2."""
    k = Fr.shape[1]
    n = len(it)
    P = np.flatnonzero(uh > 0.0) if nonneg else np.arange(k)
    ustar = np.zeros(k)
    e = np.zeros((n, len(lst)))
    mu = lam * n if weighted else lam
    if n > 0 and len(P) > 0:
        G, mu = user_system(Fr, it, lam, weighted, P)
        A = Fr[it]
        ustar[P] = chol_solve(G, A[:, P].T @ r)
        Z = np.zeros((k, len(lst)))
        Z[P] = chol_solve(G, Fr[lst][:, P].T)
        e = r[:, None] * (A @ Z)
    given = uh is not None
    if not given:
        uh = ustar
    Vl = Fr[lst]
    res = Fr[it] @ uh - r if n else np.zeros(0)
    return {"e": e, "score": Vl @ uh, "residual": Vl @ (uh - ustar) if given else np.zeros(len(lst)),
            "support": np.where(e > 0.0, e, 0.0).sum(axis=0), "opposition": np.where(e < 0.0, e, 0.0).sum(axis=0),
            "ustar": ustar, "uh": uh, "mu": mu, "P": P, "loss": float(res @ res), "dist2": float((uh - ustar) @ (uh - ustar)), "items": it, "r": r}


def ref_explain_ridge(F, ratings, U, lists, lam, weighted=True, nonneg=False, f32=False):
    """Every user of `ratings` (index, item, val): a list of ref_user dicts.  lam: one value, or one per user."""
    Fr = rounded(F, f32)
    Ur = None if U is None else rounded(U, f32)
    n = len(ratings[0]) - 1
    lam = np.broadcast_to(np.asarray(lam, np.float64), (n,))
    out = []
    for i in range(n):
        it, r = sorted_row(ratings, i)
        lst = np.asarray(lists[i])
        lst = lst[lst >= 0]
        out.append(ref_user(Fr, it, r, None if Ur is None else Ur[i], lst, float(lam[i]), weighted, nonneg))
    return out


def tables(ref, L, top):
    """The entry's outputs from the reference, for data on which every operation is exact: items int32 [n, L, top], contrib
    [n, L, top] (descending e, equal e by ascending position; padding (-1, 0.0)), per_pair [n, L, 4] (NaN on padding) and
    per_user [n, 5]."""
    n = len(ref)
    items = np.full((n, L, top), -1, np.int32)
    contrib = np.zeros((n, L, top))
    pp = np.full((n, L, 4), np.nan)
    pu = np.zeros((n, 5))
    for i, u in enumerate(ref):
        Lu = u["e"].shape[1]
        for l in range(Lu):
            o = np.argsort(-u["e"][:, l], kind="stable")[:top]
            items[i, l, :len(o)] = u["items"][o]
            contrib[i, l, :len(o)] = u["e"][o, l]
        pp[i, :Lu] = np.stack([u["score"], u["support"], u["opposition"], u["residual"]], axis=1)
        solved = len(u["items"]) > 0 and len(u["P"]) > 0
        if not solved:
            pp[i, :Lu, 3] = u["score"]
        pu[i] = (len(u["items"]), len(u["P"]), u["loss"], u["dist2"], OK)
    return items, contrib, pp, pu


def entry_tolerance(Fr, u, lst, scale=1e-10):
    """[len, L_u]: scale |r_p| |v_p| |v_j| / mu -- |G^-1| <= 1 / mu, and a Cholesky solve is good to about k 2^-52 cond(G)."""
    vp = np.linalg.norm(Fr[u["items"]], axis=1) * np.abs(u["r"])
    vj = np.linalg.norm(Fr[lst], axis=1)
    return scale * vp[:, None] * vj[None, :] / u["mu"] if len(vp) else np.zeros((0, len(lst)))
