"""A plain numpy CCDR1 (CCD++ rank-one squared-loss factorisation): the in-tree reference of tests/test_ccd_reference.py.

One residual array over the ratings, per-column sums by np.bincount (np.add.at when the accumulator is np.longdouble).  `acc` is
the arithmetic type of every sum and of u and v inside a rank; `store` is the storage type being emulated: values are rounded to
it and back exactly where the device rounds (U0 and the ratings on entry, the residual after the add-back and after the
subtraction, u and v at the rank's write-back; the subtraction and the reg terms use the rounded u and v; u and v are not rounded
between inner iterations).  With store = float32 every product that the device forms inside an fma before a cast (rounded u x
rounded v, old u x old v) is a product of two float32 values, exact in fp64: multiply-then-add here equals fma-then-cast there.
"""
from collections import namedtuple

import numpy as np

CcdResult = namedtuple("CcdResult", "W H recs inner ranks ratios")
# recs: one (iter, rank, loss, obj, diff, reg, rmse, inner) per executed rank (rank 1-based: the printed line; inner: inner
# iterations executed so far); inner / ranks: inner iterations and ranks executed in all; ratios: innerfundec_cur /
# (fundec_max * eps) of every stopping test with fundec_max > 0 (how far each decision is from its threshold)


def ccd_ref(d1, d2, user, item, val, U0, k, lam, maxiter, T=5, eps=1e-3, nmf=0, acc=np.float64, store=np.float64, perm=None,
            test=None, hook=None):
    """-> CcdResult.  perm: feed the ratings in this order (every sum then runs in another order).  test = (tuser, titem, tval).
    hook(oiter, t, us, vs): called with the rounded u and v of a rank just before they are written back (may change them in place:
    a stored value that came out one ulp off)."""
    user = np.asarray(user, np.int64); item = np.asarray(item, np.int64); val = np.asarray(val, np.float64)
    if perm is not None:
        user, item, val = user[perm], item[perm], val[perm]

    def rnd(x):
        return x.astype(store).astype(acc)

    def by(idx, w, n):
        if acc is np.float64:
            return np.bincount(idx, weights=w, minlength=n)
        out = np.zeros(n, acc)
        np.add.at(out, idx, w)
        return out

    lam = acc(lam)
    nu = np.bincount(user, minlength=d1).astype(acc)
    ni = np.bincount(item, minlength=d2).astype(acc)
    r = rnd(val.astype(acc))
    W = rnd(np.asarray(U0, np.float64).astype(acc)).reshape(d1, k).copy()
    H = np.zeros((d2, k), acc)
    reg = acc(0)
    for t in range(k):
        reg += np.sum(W[:, t] * W[:, t] * nu)
    tn = 0
    if test is not None and len(test[0]):
        tu, ti = np.asarray(test[0], np.int64), np.asarray(test[1], np.int64)
        tres = np.asarray(test[2], np.float64).astype(acc)
        tn = tres.shape[0]

    def sweep(idx, n, cnt, xe, y):
        """One RankOneUpdate per column: y = g / h, g = sum x r, h = lambda n + sum x^2; 0 and no fundec for an empty column."""
        g = by(idx, xe * r, n)
        h = lam * cnt + by(idx, xe * xe, n)
        nz = cnt > 0
        new = np.zeros(n, acc)
        new[nz] = g[nz] / h[nz]
        delta = y - new
        f = h * delta * delta
        if nmf > 0:
            neg = nz & (new < 0)
            f[neg] = (-2 * g * y)[neg]                                    # (the reference's NMF branch drops the h term)
            new[neg] = 0
        f[~nz] = 0
        return new, np.sum(f)

    recs, ratios = [], []
    inner = ranks = 0
    oldobj = acc(0)
    for oi in range(1, maxiter + 1):
        fundec_max, early = acc(0), 0
        for t in range(k):
            if early >= 5:
                break
            u = W[:, t].copy(); oldu = u.copy()
            v = H[:, t].copy(); oldv = np.zeros(d2, acc) if oi == 1 else v.copy()
            if oi > 1:
                r = rnd(r + oldu[user] * oldv[item])
            for it in range(1, T + 1):
                v, fv = sweep(item, d2, ni, u[user], v)
                u, fu = sweep(user, d1, nu, v[item], u)
                cur = fv + fu
                inner += 1
                if fundec_max > 0:
                    ratios.append(float(cur / (fundec_max * eps)))
                if cur < fundec_max * eps:
                    if it == 1:
                        early += 1
                    break
                if not (oi == 1 and t == 0 and it == 1):
                    fundec_max = max(fundec_max, cur)
            us, vs = rnd(u), rnd(v)
            if hook is not None:
                hook(oi, t, us, vs)
            W[:, t] = us; H[:, t] = vs
            r = rnd(r - us[user] * vs[item])
            loss = np.sum(r * r)
            reg += np.sum(ni * vs * vs - ni * oldv * oldv)
            reg += np.sum(nu * (us * us) - nu * (oldu * oldu))
            obj = loss + reg * lam
            rmse = 0.0
            if tn:
                tres -= us[tu] * vs[ti] - oldu[tu] * oldv[ti]
                rmse = float(np.sqrt(np.sum(tres * tres) / tn))
            recs.append((oi, t + 1, float(loss), float(obj), float(oldobj - obj), float(reg), rmse, inner))
            oldobj = obj
            ranks += 1
    return CcdResult(W.astype(np.float64), H.astype(np.float64), recs, inner, ranks, ratios)
