"""Plain-numpy reference of the ridge fold-in (include/primalcr.h, "ridge fold-in") for tests/test_foldin_ridge.py.

Per user: A = the rated rows of F ROUNDED TO THE STORAGE TYPE first, mu = lam * n (weighted) or lam, the solution of
(A^T A + mu I) u = A^T r by np.linalg.solve in float64 (through the n x n dual system when n < k: the smaller, better
conditioned one), rounded to the storage type; loss = |r - A u^|^2 and obj = loss + mu |u^|^2 at the rounded row u^.
"""
import numpy as np

DUAL, PRIMAL, CG = 0, 1, 2
OK, SINGULAR, CG_CAP = 0, 1, 2
WAVE_MAX, DIRECT_MAX = 64, 112


def form(n, k):
    if n <= k and n <= DIRECT_MAX:
        return DUAL
    if n > k and (k + 15) // 16 * 16 <= DIRECT_MAX:
        return PRIMAL
    return CG


def storage(x, f32):
    x = np.asarray(x, np.float64)
    return x.astype(np.float32).astype(np.float64) if f32 else x


def sorted_row(item, val):
    """A user's ratings in ascending item order (equal items keep their order)."""
    o = np.argsort(item, kind="stable")
    return item[o], val[o]


def solve_user(A, r, mu):
    n, k = A.shape
    if n == 0:
        return np.zeros(k)
    if n < k:
        return A.T @ np.linalg.solve(A @ A.T + mu * np.eye(n), r)
    return np.linalg.solve(A.T @ A + mu * np.eye(k), A.T @ r)


def loss_obj(A, r, mu, u):
    e = r - A @ u
    loss = float(e @ e)
    return loss, loss + mu * float(u @ u)


def fold_in(F, index, item, val, lam, weighted=True, f32=False):
    """(rows [n, k], loss [n], obj [n]) of the users of the CSR (index, item, val) over F's rows."""
    Fs = storage(F, f32)
    n, k = len(index) - 1, F.shape[1]
    U, loss, obj = np.zeros((n, k)), np.zeros(n), np.zeros(n)
    for i in range(n):
        it, r = sorted_row(item[index[i]:index[i + 1]], val[index[i]:index[i + 1]])
        A = Fs[it]
        mu = lam * len(r) if weighted else lam
        U[i] = storage(solve_user(A, r, mu), f32)
        loss[i], obj[i] = loss_obj(A, r, mu, U[i])
    return U, loss, obj


def conditions(F, index, item, lam, weighted=True):
    """Per user the condition numbers of the dual (n x n) and of the primal (k x k) system."""
    n, k = len(index) - 1, F.shape[1]
    out = np.ones((n, 2))
    for i in range(n):
        A = F[item[index[i]:index[i + 1]]]
        m = A.shape[0]
        if m == 0:
            continue
        mu = lam * m if weighted else lam
        s2 = np.linalg.svd(A, compute_uv=False) ** 2
        lo_small = s2.min() if len(s2) == min(m, k) else 0.0
        out[i, 0] = (s2.max() + mu) / ((lo_small if m <= k else 0.0) + mu)
        out[i, 1] = (s2.max() + mu) / ((lo_small if m >= k else 0.0) + mu)
    return out


def make_users(d2, lens, seed, dup_user=None, desc_user=None):
    """One user per length: distinct items of [0, d2) in ascending order, ratings in 1..5; dup_user repeats its first item in its
    last slot (two ratings of one item), desc_user's row is given in descending item order."""
    rng = np.random.default_rng(seed)
    index, items, vals = [0], [], []
    for u, n in enumerate(lens):
        it = np.sort(rng.choice(d2, size=n, replace=False)).astype(np.int32)
        v = rng.integers(1, 6, size=n).astype(np.float64)
        if u == dup_user and n >= 2:
            it[-1] = it[0]
        if u == desc_user:
            it, v = it[::-1].copy(), v[::-1].copy()
        items.append(it); vals.append(v)
        index.append(index[-1] + n)
    return (np.array(index, np.int64), np.concatenate(items).astype(np.int32) if items else np.zeros(0, np.int32),
            np.concatenate(vals) if vals else np.zeros(0))
