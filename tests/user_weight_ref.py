"""Definitional reference of the per-user-weighted PrimalCR / PrimalCR++ problem (tests/test_user_weights.py), in plain numpy:

    obj = sum_u c_u L_u + lambda/2 (|U|^2 + |V|^2),     L_u = sum_{(j,k): level_j > level_k} max(0, 1 - (m_uj - m_uk))^2
    g   = lambda V + sum_u c_u dL_u/dV,                  Ha = lambda a + sum_u c_u (generalised Hessian of L_u) a

ALL pairs of a user are enumerated (n x n blocks, no sweep, no sort), the weight is applied per user and nowhere else.  The terms
of a user do not depend on the weights, so they are computed once (user_terms) and combined with any weight vector (combine).

The enumeration is generic in its number type: with float64 scores and width 1.0 it is the reference at any input; with the
dyadic cases of tests/exact_data.py scaled to integers (scores in quarter units, width 4) it is the same definition in int64,
which the precondition test uses to bound every partial sum."""
import numpy as np

import exact_data as ed


class Terms:
    """Per-user pieces of the problem: loss[u] = L_u, pairs[u] = |Omega_u|, and per rating (CSR order) tg = dL_u/dm / 2 and
    th = (generalised Hessian of L_u in score space, applied to the probe's scores) / 2."""
    pass


def _enumerate(M, S, lev, idx, one, closed, block=512):
    """M, S: scores and probe scores per rating (float64, or int64 in some unit), one: the hinge width in M's unit, closed: the
    Hessian counts a pair exactly on the kink (PrimalCR++'s closed window; exact_data / item_edge_data state the convention)."""
    d1 = len(idx) - 1
    loss = np.zeros(d1, M.dtype); pairs = np.zeros(d1, np.int64)
    tg = np.zeros(M.shape[0], M.dtype); th = np.zeros(M.shape[0], M.dtype)
    for u in range(d1):
        s, e = int(idx[u]), int(idx[u + 1])
        if e - s < 2:
            continue
        Mu, Su, Lu = M[s:e], S[s:e], lev[s:e]
        for b0 in range(0, e - s, block):
            b1 = min(b0 + block, e - s)
            above = Lu[b0:b1, None] > Lu[None, :]                                   # rows j (higher level) x columns k
            D = one - (Mu[b0:b1, None] - Mu[None, :])
            Dp = np.where(above & (D > 0), D, 0)
            pairs[u] += int(above.sum())
            loss[u] += (Dp * Dp).sum()
            tg[s + b0:s + b1] -= Dp.sum(1)
            tg[s:e] += Dp.sum(0)
            W = np.where(above & ((D >= 0) if closed else (D > 0)), Su[b0:b1, None] - Su[None, :], 0)
            th[s + b0:s + b1] += W.sum(1)
            th[s:e] -= W.sum(0)
    return loss, pairs, tg, th


def user_terms(U, V, idx, item, val, solver, a):
    """Float64 terms of every user at (U, V) with probe a."""
    t = Terms()
    t.idx = np.asarray(idx, np.int64); t.item = np.asarray(item, np.int64)
    t.ru = np.repeat(np.arange(len(t.idx) - 1), np.diff(t.idx))
    t.U = np.asarray(U, np.float64); t.V = np.asarray(V, np.float64); t.a = np.asarray(a, np.float64)
    t.m = (t.U[t.ru] * t.V[t.item]).sum(1)
    s = (t.U[t.ru] * t.a[t.item]).sum(1)
    t.loss, t.pairs, t.tg, t.th = _enumerate(t.m, s, ed.levels_of(val, solver), t.idx, 1.0, solver == 2)
    return t


def _scatter(t, coef):
    """sum over ratings of coef[z] U[user z] into the rows item z (d2 x r), column by column"""
    out = np.zeros_like(t.V)
    for col in range(t.V.shape[1]):
        out[:, col] = np.bincount(t.item, weights=coef * t.U[t.ru, col], minlength=t.V.shape[0])
    return out


def combine(t, w, lam, ignore_user=None):
    """(objective, g, Ha, loss part, g without lambda V, Ha without lambda a) of the weighted problem.  ignore_user: the MUTANT
    reference of the duplication test -- that user's weight is taken as 1 whatever w says."""
    w = np.array(w, np.float64)
    if ignore_user is not None:
        w[ignore_user] = 1.0
    wr = w[t.ru]
    loss = float((w * t.loss).sum())
    g0 = _scatter(t, wr * 2.0 * t.tg)
    h0 = _scatter(t, wr * 2.0 * t.th)
    obj = loss + lam / 2.0 * float((t.U ** 2).sum() + (t.V ** 2).sum())
    return obj, lam * t.V + g0, lam * t.a + h0, loss, g0, h0


def class_weights(lens, values):
    """Weights from `values` dealt round-robin inside every user-length class of exact_data.CLASS_CAPS (users in index order), so
    that every class with at least len(values) users holds every value."""
    lens = np.asarray(lens)
    cls = np.searchsorted(np.asarray(ed.CLASS_CAPS), lens, side="left")            # class c: CAPS[c-1] < len <= CAPS[c]
    w = np.ones(len(lens))
    for c in np.unique(cls):
        who = np.flatnonzero(cls == c)
        w[who] = np.asarray(values, np.float64)[(np.arange(who.size) + int(c)) % len(values)]
    return w, cls


def integer_budget(c, idx, item, val, w, a):
    """The weighted dyadic case in int64 (exact_data's scaling: U2 = 2 U, V2 = 2 V, A2 = 2 a, scores in quarter units, w2 = 2 w):
    the sweep coefficient a kernel stores per rating is c_u dL/dm = w2 tg4 / 4 (a whole number of QUARTERS: the derivative's
    factor 2 absorbs the half weights), and 8 g = sum (w2 tg4) U2 + 8 lambda V.  Returns, for the gradient and the probe:
      coef    max |w2 tg4|: the stored coefficient in quarter units
      abssum  max over (item, column) of sum |w2 tg4| |U2| + |8 lambda V|: bounds EVERY partial sum of that entry, in any order
              and any split, in eighth units
      val8    8 g and 8 Ha themselves
    and 32 obj."""
    U2 = np.rint(2 * c.U).astype(np.int64); V2 = np.rint(2 * c.V).astype(np.int64); A2 = np.rint(2 * np.asarray(a)).astype(np.int64)
    w2 = np.rint(2 * np.asarray(w)).astype(np.int64)
    assert np.array_equal(U2, 2 * c.U) and np.array_equal(V2, 2 * c.V) and np.array_equal(A2, 2 * np.asarray(a)) and np.array_equal(w2, 2 * np.asarray(w))
    lam8 = int(4 * c.lam)                                                            # 8 lambda V = 4 lambda V2
    assert lam8 == 4 * c.lam
    idx = np.asarray(idx, np.int64); item = np.asarray(item, np.int64)
    ru = np.repeat(np.arange(len(idx) - 1), np.diff(idx))
    M4 = (U2[ru] * V2[item]).sum(1); S4 = (U2[ru] * A2[item]).sum(1)
    loss16, pairs, tg4, th4 = _enumerate(M4, S4, ed.levels_of(val, c.solver), idx, 4, c.solver == 2)
    out = {}
    for name, t4, B2 in (("g", tg4, V2), ("Ha", th4, A2)):
        coef = w2[ru] * t4
        val8 = lam8 * B2.copy(); abssum = np.abs(lam8 * B2)
        np.add.at(val8, item, coef[:, None] * U2[ru])
        np.add.at(abssum, item, np.abs(coef)[:, None] * np.abs(U2[ru]))
        out[name] = dict(coef=int(np.abs(coef).max()), abssum=int(abssum.max()), val8=val8)
    out["obj32"] = int((w2 * loss16).sum()) + int(4 * c.lam) * int((U2 * U2).sum() + (V2 * V2).sum())
    return out
