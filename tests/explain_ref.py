"""Plain-numpy fp64 reference of explain() (include/primalcr.h, "explaining recommendations") for tests/test_explain.py.

``pair_coeffs``   the all-pairs coefficients t of ONE user (d loss / d m), formed exactly as foldin_ref.pair_obj_grad forms them.
``ref_explain``   per user: the factors rounded to the storage type, the row sorted by item (stable), t, g = lam_u u + V_I^T t,
                  e[p, j] = -(t_p / lam_u) (v_p . v_j), rho, score, support, opposition and the contributors by a stable argsort
                  of -e (ties: ascending position in the item-sorted row); padding as the entry writes it.
``term_bounds``   the documented error bound of every e[p, j], evaluated from the data.
"""
import numpy as np

from foldin_ref import BLOCK, levels_of


def pair_coeffs(u, Vr, val, solver):
    """(m, t, loss): m = Vr u, t[p] = d loss / d m_p over the pairs (j above k by level) of max(0, 1 - (m_j - m_k))^2."""
    n = Vr.shape[0]
    m = Vr @ u if n else np.zeros(0)
    t = np.zeros(n)
    loss = 0.0
    if n == 0:
        return m, t, loss
    lev = levels_of(val, solver)
    for a in range(0, n, BLOCK):
        b = min(n, a + BLOCK)
        h = np.where(lev[a:b, None] > lev[None, :], 1.0 - (m[a:b, None] - m[None, :]), 0.0)
        np.maximum(h, 0.0, out=h)
        loss += float(np.einsum("ij,ij->", h, h))
        t[a:b] -= 2.0 * h.sum(axis=1)
        t += 2.0 * h.sum(axis=0)
    return m, t, loss


def rounded(X, f32):
    X = np.asarray(X, np.float64)
    return X.astype(np.float32).astype(np.float64) if f32 else X


def sorted_row(index, item, val, i):
    """User i's row in ascending item order, equal items keeping their order: (items, ratings)."""
    a, b = int(index[i]), int(index[i + 1])
    o = np.argsort(item[a:b], kind="stable")
    return np.asarray(item[a:b])[o], np.asarray(val[a:b], np.float64)[o]


def ref_explain(V, ratings, U, lists, lam, top, solver, f32=False, weights=None, keep=False):
    """Returns a dict: items int32 [n, L, top], contrib [n, L, top], per_pair [n, L, 4], per_user [n, 3]; with keep also the
    per-user lists `e` ([len, L_u] contributions), `t`, `rows` (the sorted item ids), `g` and `lam_u`."""
    index, item, val = ratings
    V, U = rounded(V, f32), rounded(U, f32)
    lists = np.asarray(lists)
    n, L = lists.shape
    out = {"items": np.full((n, L, top), -1, np.int32), "contrib": np.zeros((n, L, top)), "per_pair": np.full((n, L, 4), np.nan),
           "per_user": np.zeros((n, 3)), "e": [], "t": [], "rows": [], "g": [], "lam_u": []}
    for i in range(n):
        it, rv = sorted_row(index, item, val, i)
        lam_u = lam / weights[i] if weights is not None else lam
        Vr, u = V[it], U[i]
        m, t, loss = pair_coeffs(u, Vr, rv, solver)
        g = lam_u * u + (Vr.T @ t if len(it) else 0.0)
        Lu = int((lists[i] >= 0).sum())
        Vl = V[lists[i, :Lu]]
        e = -(t / lam_u)[:, None] * (Vr @ Vl.T)                               # [len, Lu]
        out["per_user"][i] = (len(it), loss, float(g @ g))
        pp = out["per_pair"][i]
        pp[:Lu, 0] = Vl @ u
        pp[:Lu, 1] = np.where(e > 0, e, 0.0).sum(axis=0)
        pp[:Lu, 2] = np.where(e < 0, e, 0.0).sum(axis=0)
        pp[:Lu, 3] = (Vl @ g) / lam_u
        for l in range(Lu):
            o = np.argsort(-e[:, l], kind="stable")[:top]
            out["items"][i, l, :len(o)] = it[o]
            out["contrib"][i, l, :len(o)] = e[o, l]
        if keep:
            out["e"].append(e); out["t"].append(t); out["rows"].append(it); out["g"].append(g); out["lam_u"].append(lam_u)
    return out


def term_bounds(V, U, lists, ref, i, k, eps_m):
    """For user i of a ref_explain(..., keep=True) result, V and U rounded as it rounded them: (b0 [len, L_u], bc [len, L_u],
    extra [L_u]).  b0 = (k + 2) 2^-52 sum_t |v_pt v_jt| |t_p| / lam_u is the documented bound of e[p, j] for given coefficients;
    extra = (k + 2) 2^-52 (sum_t |v_jt g_t| / lam_u + sum_t |v_jt u_t|) the same for rho and the score.  bc = dc |v_p . v_j| / lam_u
    is what the rounding of m = V_I u adds when two implementations are compared: the device and this reference both form m with
    rounding error, in different orders (the device in the storage type), dm = (k + 2) eps_m max_p sum_t |u_t v_pt| with
    eps_m = 2^-53 or 2^-24, and a coefficient moves by at most dc = 2 n dm."""
    it, t, lam_u, g = ref["rows"][i], ref["t"][i], ref["lam_u"][i], ref["g"][i]
    Lu = ref["e"][i].shape[1]
    Vr, Vl, u = V[it], V[np.asarray(lists)[i, :Lu]], U[i]
    n = len(it)
    dm = (k + 2) * eps_m * (np.abs(Vr) @ np.abs(u)).max() if n else 0.0
    dc = 2.0 * n * dm
    b0 = (k + 2) * 2.0 ** -52 * (np.abs(Vr) @ np.abs(Vl).T) * np.abs(t)[:, None] / lam_u
    bc = dc * np.abs(Vr @ Vl.T) / lam_u
    extra = (k + 2) * 2.0 ** -52 * (np.abs(Vl) @ np.abs(g) / lam_u + np.abs(Vl) @ np.abs(u))
    return b0, bc, extra
