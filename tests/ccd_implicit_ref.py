"""A plain numpy CCDR1 under implicit feedback: the in-tree reference of tests/test_ccd_implicit.py.

tests/ccd_weight_ref.py plus `alpha`, the weight of every UNRATED cell, whose target is 0:

    min sum_{z in Omega} c_z (r_z - u_i . v_j)^2 + alpha sum_{(i,j) not in Omega} (u_i . v_j)^2 + lambda (sum_i W_i |u_i|^2 + sum_j W_j |v_j|^2),
    W_i = (the sum of c_z over user i's ratings) + alpha (d2 - n_i),  W_j likewise with d1 - n_j.

Written from the definition, with no Gram identity: the rated cells' residual is handled exactly as in ccd_weight_ref (rounded to
`store`); the unrated cells' part comes from a dense p^ = W[:, != t] @ H[:, != t].T (the prediction without rank t, in `acc`) masked to
the unrated cells -- their residual is -p^ and has no storage: per column g = sum_Omega (c x) r^ - alpha sum_unrated x p^, h = lambda W
+ sum_Omega (c x) x + alpha sum_unrated x^2; loss = sum_Omega (c r) r + alpha sum_unrated (W H^T)^2.  Every column is updated, an
empty one too.  `acc`, `store`, `perm` and `hook` are ccd_ref's knobs (with `perm` the dense sums run in reversed order too; with a
long-double `acc`, which has no BLAS, the dense product is carried from rank to rank instead of being formed anew); alpha is rounded
to `store` on entry, as the weights are.  On a fully rated set every unrated sum is empty and every expression is
ccd_weight_ref's, bit for bit; scaling all weights and alpha by one power of two scales g, h, fundec, loss and reg exactly.

`defect` seeds one mistake, for the tests that show the bounds would see it:
  "no_obs_correction"  the all-cells sums are not reduced by the rated cells (the mask is all ones);
  "obs_reg"            W without alpha (d - n);
  "empty_zero"         empty columns are set to 0, as the explicit path does;
  "stale_gram"         the sum x p^ over the unrated cells uses the STORED column of the other side, not its current work vector.
"""
import numpy as np

from ccd_ref import CcdResult

DEFECTS = (None, "no_obs_correction", "obs_reg", "empty_zero", "stale_gram")


def ccd_implicit_ref(d1, d2, user, item, val, w, alpha, U0, k, lam, maxiter, T=5, eps=1e-3, nmf=0, acc=np.float64, store=np.float64,
                     perm=None, test=None, hook=None, defect=None):
    """-> CcdResult.  w: one weight per rating in the order of user / item / val, or None (c = 1)."""
    assert defect in DEFECTS
    user = np.asarray(user, np.int64); item = np.asarray(item, np.int64); val = np.asarray(val, np.float64)
    w = np.ones(val.shape[0]) if w is None else np.asarray(w, np.float64)
    flip = perm is not None
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

    def over_users(A, x):
        """sum_i A[i, j] x[i] for every item j"""
        return (A[::-1] * x[::-1, None]).sum(axis=0) if flip else (A * x[:, None]).sum(axis=0)

    def over_items(A, x):
        """sum_j A[i, j] x[j] for every user i"""
        return (A[:, ::-1] * x[None, ::-1]).sum(axis=1) if flip else (A * x[None, :]).sum(axis=1)

    lam = acc(lam)
    a = rnd(np.array([alpha], np.float64).astype(acc))[0]
    assert np.isfinite(a) and a > 0
    nu = np.bincount(user, minlength=d1).astype(acc)
    ni = np.bincount(item, minlength=d2).astype(acc)
    c = rnd(w.astype(acc))
    assert np.all(np.isfinite(c)) and np.all(c > 0)
    M = np.ones((d1, d2), acc)                                            # 1 on the unrated cells
    if defect != "no_obs_correction":
        M[user, item] = 0
    Wu, Wi = by(user, c, d1), by(item, c, d2)
    if defect != "obs_reg":
        Wu, Wi = Wu + a * (acc(d2) - nu), Wi + a * (acc(d1) - ni)
    r = rnd(val.astype(acc))
    W = rnd(np.asarray(U0, np.float64).astype(acc)).reshape(d1, k).copy()
    H = np.zeros((d2, k), acc)
    full = np.zeros((d1, d2), acc)                                        # W @ H.T, kept only when acc is not float64
    reg = acc(0)
    for t in range(k):
        reg += np.sum(W[:, t] * W[:, t] * Wu)
    tn = 0
    if test is not None and len(test[0]):
        tu, ti = np.asarray(test[0], np.int64), np.asarray(test[1], np.int64)
        tres = np.asarray(test[2], np.float64).astype(acc)
        tn = tres.shape[0]

    def sweep(idx, n, cnt, Wc, xe, y, gm, hm):
        """One RankOneUpdate per column, the unrated cells' sums gm (of -alpha x p^) and hm (of alpha x^2) included."""
        cx = c * xe
        g = by(idx, cx * r, n) + gm
        h = lam * Wc + by(idx, cx * xe, n) + hm
        nz = cnt > 0 if defect == "empty_zero" else np.ones(n, bool)
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
            stored_u, stored_v = W[:, t].copy(), H[:, t].copy()
            if oi > 1:
                r = rnd(r + oldu[user] * oldv[item])
            if acc is np.float64:
                others = np.arange(k) != t
                MP = M * (W[:, others] @ H[:, others].T)                  # p^ on the unrated cells, 0 elsewhere
            else:                                                         # (no BLAS for long double: the dense product is carried along)
                MP = M * (full - np.outer(W[:, t], H[:, t]))
            for it in range(1, T + 1):
                xs = stored_u if defect == "stale_gram" else u
                gm, hm = over_users(MP, xs), over_users(M, u * u)
                v, fv = sweep(item, d2, ni, Wi, u[user], v, -a * gm, a * hm)
                xs = stored_v if defect == "stale_gram" else v
                gm, hm = over_items(MP, xs), over_items(M, v * v)
                u, fu = sweep(user, d1, nu, Wu, v[item], u, -a * gm, a * hm)
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
            if acc is not np.float64:
                full = full + (np.outer(us, vs) - np.outer(oldu, stored_v))
            P = MP + M * np.outer(us, vs)                                 # the prediction on the unrated cells: rank t's term joins p^
            loss = np.sum((c * r) * r) + a * np.sum(P * P)
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
