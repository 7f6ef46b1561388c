"""A plain numpy CCDR1 with one confidence weight per rating: the in-tree reference of tests/test_ccd_weights.py.

tests/ccd_ref.py with `w`:  min sum_z c_z (r_z - u_i . v_j)^2 + lambda (sum_i W_i |u_i|^2 + sum_j W_j |v_j|^2), W = a row's sum of
c_z.  The rank-one update of a non-empty column is g = sum (c x) r, h = lambda W + sum (c x) x, new = g / h, fundec = h (old -
new)^2; loss = sum (c r) r; the reg bookkeeping uses W where ccd_ref uses the counts; an empty column is decided by its count; the
stopping rule and the test rmse do not see weights.  `acc`, `store`, `perm` and `hook` are ccd_ref's knobs; the weights are rounded
to `store` on entry, as the ratings are.  With w = 1 every expression is ccd_ref's, bit for bit (c x = x, W = the count), which
ties this reference to the goldens of the reference binary; with all weights the same power of two g, h, fundec, loss and reg
scale exactly and the factors are the unweighted ones.

`defect` seeds one mistake, for the tests that show the bounds would see it: "count_reg" regularises by the rating count
instead of W (in h and in the reg bookkeeping); "plain_loss" drops the weights from the loss alone.
"""
import numpy as np

from ccd_ref import CcdResult


def ccd_weight_ref(d1, d2, user, item, val, w, U0, k, lam, maxiter, T=5, eps=1e-3, nmf=0, acc=np.float64, store=np.float64, perm=None,
                   test=None, hook=None, defect=None):
    """-> CcdResult.  w: one weight per rating, in the order of user / item / val."""
    assert defect in (None, "count_reg", "plain_loss")
    user = np.asarray(user, np.int64); item = np.asarray(item, np.int64); val = np.asarray(val, np.float64)
    w = np.asarray(w, np.float64)
    if perm is not None:
        user, item, val, w = user[perm], item[perm], val[perm], w[perm]

    def rnd(x):
        return x.astype(store).astype(acc)

    def by(idx, x, n):
        if acc is np.float64:
            return np.bincount(idx, weights=x, minlength=n)
        out = np.zeros(n, acc)
        np.add.at(out, idx, x)
        return out

    lam = acc(lam)
    nu = np.bincount(user, minlength=d1).astype(acc)
    ni = np.bincount(item, minlength=d2).astype(acc)
    c = rnd(w.astype(acc))
    assert np.all(np.isfinite(c)) and np.all(c > 0)
    Wu, Wi = (nu, ni) if defect == "count_reg" else (by(user, c, d1), by(item, c, d2))
    r = rnd(val.astype(acc))
    W = rnd(np.asarray(U0, np.float64).astype(acc)).reshape(d1, k).copy()
    H = np.zeros((d2, k), acc)
    reg = acc(0)
    for t in range(k):
        reg += np.sum(W[:, t] * W[:, t] * Wu)
    tn = 0
    if test is not None and len(test[0]):
        tu, ti = np.asarray(test[0], np.int64), np.asarray(test[1], np.int64)
        tres = np.asarray(test[2], np.float64).astype(acc)
        tn = tres.shape[0]

    def sweep(idx, n, cnt, Wc, xe, y):
        """One weighted RankOneUpdate per column; 0 and no fundec for an empty column (by its count)."""
        cx = c * xe
        g = by(idx, cx * r, n)
        h = lam * Wc + by(idx, cx * xe, n)
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
                v, fv = sweep(item, d2, ni, Wi, u[user], v)
                u, fu = sweep(user, d1, nu, Wu, v[item], u)
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
            loss = np.sum(r * r) if defect == "plain_loss" else np.sum((c * r) * r)
            reg += np.sum(Wi * vs * vs - Wi * oldv * oldv)
            reg += np.sum(Wu * (us * us) - Wu * (oldu * oldu))
            obj = loss + reg * lam
            rmse = 0.0
            if tn:
                tres -= us[tu] * vs[ti] - oldu[tu] * oldv[ti]
                rmse = float(np.sqrt(np.sum(tres * tres) / tn))
            recs.append((oi, t + 1, float(loss), float(obj), float(oldobj - obj), float(reg), rmse, inner))
            oldobj = obj
            ranks += 1
    return CcdResult(W.astype(np.float64), H.astype(np.float64), recs, inner, ranks, ratios)
