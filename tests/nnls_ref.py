"""Plain-numpy reference of the non-negative fold-in (include/primalcr.h, "non-negative fold-in") for tests/test_foldin_nnls.py.

Per user: A = the rated rows of F ROUNDED TO THE STORAGE TYPE first, mu = lam * n (weighted) or lam, G = A^T A + mu I, b = A^T r,
and the header's pivoting rule word for word with np.linalg.solve on G_PP in float64.  The row is rounded to the storage type;
loss = |r - A u^|^2 and obj = loss + mu |u^|^2 at the rounded row u^.
"""
import numpy as np

import ridge_ref as rr

DIRECT, CG = 0, 1
OK, SINGULAR, CAP = 0, 1, 2
PIVOT_CAP = 64
DIRECT_MAX = 112


def form(k):
    return DIRECT if (k + 15) // 16 * 16 <= DIRECT_MAX else CG


def solve_user(G, b, cap=PIVOT_CAP):
    """(u, P (bool mask), pivots, status, y) of min 1/2 u^T G u - b^T u over u >= 0 by the Kim-Park rule."""
    k = len(b)
    P = np.ones(k, bool)
    alpha, beta = 3, k + 1
    u, y = np.zeros(k), np.zeros(k)
    for pivot in range(1, cap + 1):
        u = np.zeros(k)
        if P.any():
            u[P] = np.linalg.solve(G[np.ix_(P, P)], b[P])
        y = G @ u - b
        y[P] = 0.0
        V = (P & (u < 0.0)) | (~P & (y < 0.0))
        nv = int(V.sum())
        if nv == 0:
            return u, P, pivot, OK, y
        if nv < beta:
            beta, alpha, X = nv, 3, V
        elif alpha > 0:
            alpha, X = alpha - 1, V
        else:
            X = np.zeros(k, bool)
            X[np.flatnonzero(V).max()] = True
        P = P ^ X
    return np.maximum(u, 0.0), P, cap, CAP, y


def system(Fs, item, val, lam, weighted):
    it, r = rr.sorted_row(item, val)
    A = Fs[it]
    mu = lam * len(r) if weighted else lam
    return A, r, mu, A.T @ A + mu * np.eye(Fs.shape[1]), A.T @ r


def fold_in(F, index, item, val, lam, weighted=True, f32=False):
    """dict of rows [n, k], passive [n, k] bool, pivots [n], loss [n], obj [n], kkt [n] (the residual over |b|), margin [n] (the
    complementarity margin), cond [n] (of G) of the users of the CSR (index, item, val) over F's rows."""
    Fs = rr.storage(F, f32)
    n, k = len(index) - 1, F.shape[1]
    out = dict(rows=np.zeros((n, k)), passive=np.zeros((n, k), bool), pivots=np.zeros(n, np.int64), loss=np.zeros(n), obj=np.zeros(n),
               kkt=np.zeros(n), margin=np.full(n, np.inf), cond=np.ones(n), status=np.zeros(n, np.int64))
    for i in range(n):
        if index[i + 1] == index[i]:
            continue
        A, r, mu, G, b = system(Fs, item[index[i]:index[i + 1]], val[index[i]:index[i + 1]], lam, weighted)
        u, P, piv, st, y = solve_user(G, b)
        out["passive"][i], out["pivots"][i], out["status"][i] = P, piv, st
        out["rows"][i] = rr.storage(u, f32)
        out["loss"][i], out["obj"][i] = rr.loss_obj(A, r, mu, out["rows"][i])
        nb = max(float(np.linalg.norm(b)), 1e-300)
        g = G @ u - b                                          # KKT: u >= 0, g >= 0 on Z, g = 0 on P
        out["kkt"][i] = max(np.abs(g[P]).max(initial=0.0), np.maximum(-g[~P], 0.0).max(initial=0.0), np.maximum(-u, 0.0).max()) / nb
        mp = u[P].min(initial=np.inf) / max(np.abs(u).max(), 1e-300)
        mz = y[~P].min(initial=np.inf) / nb
        out["margin"][i] = min(mp, mz)
        out["cond"][i] = np.linalg.cond(G)
    return out
