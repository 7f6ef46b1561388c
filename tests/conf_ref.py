"""Plain-numpy reference of the confidence-weighted / implicit fold-in (include/primalcr.h, "confidence-weighted and implicit
fold-in") for tests/test_foldin_conf.py.

Per user, by the definition: F ROUNDED TO THE STORAGE TYPE first, a_p = F[I_p] in ascending item order (equal items keep their
order, the weights with them), G = F^T F over all rows of F,
    M = alpha G + sum_p (c_p - alpha) a_p a_p^T + mu I,   b = sum_p c_p r_p a_p,
    mu = lam (sum_p c_p + alpha (d - len)) (weighted) or lam,
u = np.linalg.solve(M, b) in float64, rounded to the storage type; at the rounded row u^
    loss = sum_p c_p (r_p - a_p.u^)^2 + alpha (u^^T G u^ - sum_p (a_p.u^)^2),   obj = loss + mu |u^|^2.
weights and alpha are used in float64 as given.  A user without ratings gets a zero row and loss = obj = 0.
"""
import numpy as np

import ridge_ref as rr


def form(n, k, implicit):
    """The rule of (len, k, alpha > 0): the ridge rule, or PRIMAL / CG by the padded rank alone for alpha > 0."""
    if not implicit:
        return rr.form(n, k)
    return rr.PRIMAL if (k + 15) // 16 * 16 <= rr.DIRECT_MAX else rr.CG


def block(n, k, implicit):
    if form(n, k, implicit) == rr.CG or n > rr.WAVE_MAX:
        return 256
    return 256 if implicit and (k + 15) // 16 * 16 > 64 else 64


def sorted_row(item, val, w):
    o = np.argsort(item, kind="stable")
    return item[o], val[o], w[o]


def mu_of(lam, c, alpha, d, weighted):
    return lam * (float(np.sum(c)) + alpha * (d - len(c))) if weighted else lam


def system(A, r, c, alpha, G, mu):
    k = A.shape[1]
    M = alpha * G + (A * (c - alpha)[:, None]).T @ A + mu * np.eye(k)
    return M, A.T @ (c * r)


def loss_obj(A, r, c, alpha, G, mu, u):
    s = A @ u
    loss = float(np.sum(c * (r - s) ** 2)) + alpha * (float(u @ G @ u) - float(s @ s))
    return loss, loss + mu * float(u @ u)


def fold_in(F, index, item, val, lam, weights=None, alpha=0.0, weighted=True, f32=False):
    """(rows [n, k], loss [n], obj [n]) of the users of the CSR (index, item, val) over F's rows."""
    Fs = rr.storage(F, f32)
    G = Fs.T @ Fs
    n, (d, k) = len(index) - 1, F.shape
    w = np.ones(len(item)) if weights is None else np.asarray(weights, np.float64)
    U, loss, obj = np.zeros((n, k)), np.zeros(n), np.zeros(n)
    for i in range(n):
        a, b = index[i], index[i + 1]
        if a == b:
            continue
        it, r, c = sorted_row(item[a:b], val[a:b], w[a:b])
        A = Fs[it]
        mu = mu_of(lam, c, alpha, d, weighted)
        M, rhs = system(A, r, c, alpha, G, mu)
        U[i] = rr.storage(np.linalg.solve(M, rhs), f32)
        loss[i], obj[i] = loss_obj(A, r, c, alpha, G, mu, U[i])
    return U, loss, obj


def conditions(F, index, item, lam, weights=None, alpha=0.0, weighted=True):
    """Per user (smallest eigenvalue, condition number) of the systems a form may factor: the k x k primal M and, for alpha == 0
    and len <= k, the len x len dual A A^T + mu C^-1."""
    G = F.T @ F
    n, (d, k) = len(index) - 1, F.shape
    w = np.ones(len(item)) if weights is None else np.asarray(weights, np.float64)
    out = np.ones((n, 2))
    for i in range(n):
        a, b = index[i], index[i + 1]
        if a == b:
            continue
        A, c = F[item[a:b]], w[a:b]
        mu = mu_of(lam, c, alpha, d, weighted)
        ev = np.linalg.eigvalsh(system(A, np.zeros(b - a), c, alpha, G, mu)[0])
        lo, cond = ev[0], ev[-1] / ev[0]
        if alpha == 0.0 and b - a <= k:
            ed = np.linalg.eigvalsh(A @ A.T + mu * np.diag(1.0 / c))
            lo, cond = min(lo, ed[0]), max(cond, ed[-1] / ed[0])
        out[i] = lo, cond
    return out


def completed(F, index, item, val, weights, alpha):
    """The implicit problem written out: every user's row over ALL d items, the rated ones first, the unrated ones as rating 0 of
    weight alpha; a completed row's weights add up to the sparse row's W = sum c + alpha (d - len).  Users hold distinct items (an
    item rated twice is subtracted twice in the sparse problem, which a completed row cannot say).  Returns (index, item, val,
    weights) of the completed rows."""
    d = F.shape[0]
    w = np.ones(len(item)) if weights is None else np.asarray(weights, np.float64)
    idx, its, vals, ws = [0], [], [], []
    for i in range(len(index) - 1):
        a, b = index[i], index[i + 1]
        assert len(set(item[a:b])) == b - a
        rest = np.setdiff1d(np.arange(d, dtype=np.int32), item[a:b])
        its.append(np.concatenate([item[a:b], rest])); vals.append(np.concatenate([val[a:b], np.zeros(len(rest))]))
        ws.append(np.concatenate([w[a:b], np.full(len(rest), alpha)]))
        idx.append(idx[-1] + d)
    return np.array(idx, np.int64), np.concatenate(its).astype(np.int32), np.concatenate(vals), np.concatenate(ws)
