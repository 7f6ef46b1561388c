"""Plain-numpy / oracle reference of the fold-in (include/primalcr.h, "fold-in") for tests/test_foldin.py.

``pair_obj_grad``  the all-pairs objective and gradient of ONE user, blocked by 512 rows as tests/exact_data.py::brute_force.
``ref_fold_in``    the fold-in loop over the oracle's update_u_new / update_u + comp_m, with the STALLED rule applied from the
                   numpy objective (the oracle itself moves to the last tried point, quirk q5).
``make_users``     the fixture: one user per length, ratings as the solver type wants them.
"""
import numpy as np

from oracle.oracle_py import CSR

CONVERGED, STEP_CAP, STALLED = 0, 1, 2
BLOCK = 512


def levels_of(val, solver):
    """The level keys of training: lround buckets for PrimalCR++ (2), the raw double for PrimalCR (1)."""
    val = np.asarray(val, np.float64)
    return np.sign(val) * np.floor(np.abs(val) + 0.5) if solver == 2 else val


def pair_obj_grad(u, Vr, val, lam, solver, want_grad=True):
    """lam/2 |u|^2 + sum over pairs (j above k by level) of max(0, 1 - (m_j - m_k))^2 and its gradient in u; m = Vr u."""
    # (the windows' strictness -- PrimalCR's mask < 1 against PrimalCR++'s <= 1 -- changes neither: a pair at the boundary adds 0)
    u = np.asarray(u, np.float64)
    n = Vr.shape[0]
    obj = lam / 2.0 * float(u @ u)
    g = lam * u
    if n == 0:
        return obj, (g if want_grad else None)
    m = Vr @ u
    lev = levels_of(val, solver)
    t = np.zeros(n)
    loss = 0.0
    for a in range(0, n, BLOCK):
        b = min(n, a + BLOCK)
        h = np.where(lev[a:b, None] > lev[None, :], 1.0 - (m[a:b, None] - m[None, :]), 0.0)
        np.maximum(h, 0.0, out=h)
        loss += float(np.einsum("ij,ij->", h, h))
        if want_grad:
            t[a:b] -= 2.0 * h.sum(axis=1)
            t += 2.0 * h.sum(axis=0)
    return obj + loss, ((g + Vr.T @ t) if want_grad else None)


def user_rows(X, V, i):
    a, b = int(X.idx[i]), int(X.idx[i + 1])
    return V[X.item[a:b]], X.val[a:b]


def n_levels(X, i, solver):
    a, b = int(X.idx[i]), int(X.idx[i + 1])
    return len(np.unique(levels_of(X.val[a:b], solver)))


def ref_step(orc, X, V, lam, solver, U, stepsize=1.0, users=None, numpy_too=False):
    """One fold-in step of every user (or of `users`) from U: returns (U_new, info) with per-user arrays cg, ls, obj (the
    oracle's obj_u_new: the objective at the returned row) and status (CONVERGED / STEP_CAP = stepped / STALLED).  A STALLED or
    CONVERGED user keeps its row.  The all-pairs numpy objective decides the STALLED rule when the oracle used all 20 tries; with
    numpy_too it is evaluated for every user: obj0 and gn2 at U."""
    n = X.d1
    U = np.ascontiguousarray(U, np.float64)
    m = orc.comp_m(U, V, X)
    Un = U.copy()
    info = {k: np.zeros(n) for k in ("cg", "ls", "obj")}
    info["obj0"], info["gn2"] = np.full(n, np.nan), np.full(n, np.nan)
    info["status"] = np.full(n, STEP_CAP)
    for i in (range(n) if users is None else users):
        Vr, val = user_rows(X, V, i)
        if numpy_too:
            o0, g = pair_obj_grad(U[i], Vr, val, lam, solver)
            info["obj0"][i], info["gn2"][i] = o0, (float(g @ g) if Vr.shape[0] else 0.0)
        un, obj, st = orc.update_u_new(i, V, X, m, lam, stepsize, U[i], solver=solver)
        info["cg"][i], info["ls"][i], info["obj"][i] = st["cg"], st["ls"], obj
        if st["ls"] == 0:                                   # the reference skipped the user: no rating, |g|^2 < 1e-4, no pair
            info["status"][i] = CONVERGED
        elif st["ls"] < 20 or pair_obj_grad(un, Vr, val, lam, solver, False)[0] < pair_obj_grad(U[i], Vr, val, lam, solver, False)[0]:
            Un[i] = un
        else:                                               # no try accepted: the fold-in stays where it was
            info["status"][i] = STALLED
            info["obj"][i] = pair_obj_grad(U[i], Vr, val, lam, solver, False)[0]
    return Un, info


def ref_fold_in(orc, X, V, lam, solver, U0, steps, stepsize=1.0, numpy_too=False):
    """The whole loop: returns (U, per) with per-user steps, cg, ls, obj, gn2, status and `hist`, the list of ref_step infos."""
    n = X.d1
    U = np.ascontiguousarray(U0, np.float64).copy()
    per = {k: np.zeros(n) for k in ("steps", "cg", "ls", "obj", "gn2")}
    per["status"] = np.full(n, STEP_CAP)
    active = list(range(n))
    hist = []
    for _ in range(steps):
        if not active:
            break
        U, info = ref_step(orc, X, V, lam, solver, U, stepsize, users=active, numpy_too=numpy_too)
        hist.append(info)
        nxt = []
        for i in active:
            per["cg"][i] += info["cg"][i]; per["ls"][i] += info["ls"][i]
            per["obj"][i], per["gn2"][i] = info["obj"][i], info["gn2"][i]
            if info["status"][i] == STEP_CAP:
                per["steps"][i] += 1
                nxt.append(i)
            else:
                per["status"][i] = info["status"][i]
        active = nxt
    return U, per, hist


def make_users(d2, lengths, solver, seed, forced=None):
    """One user per entry of `lengths`: distinct items ascending; integer ratings 1..5 for PrimalCR++ (2), quarter steps + 0.125
    for PrimalCR (1) so that every value is its own level.  forced: {user: ratings} overrides.  Returns an oracle CSR."""
    rng = np.random.default_rng(seed)
    idx = np.zeros(len(lengths) + 1, np.int64)
    items, vals = [], []
    for i, n in enumerate(lengths):
        it = np.sort(rng.choice(d2, size=n, replace=False))
        v = rng.integers(1, 6, size=n).astype(np.float64) if solver == 2 else 1.125 + 0.25 * rng.integers(0, 20, size=n)
        if forced and i in forced:
            v = np.asarray(forced[i], np.float64)
        items.append(it); vals.append(v)
        idx[i + 1] = idx[i] + n
    return CSR(len(lengths), d2, idx, np.concatenate(items) if items else np.zeros(0, np.int64), np.concatenate(vals) if vals else np.zeros(0))


def csr_args(X):
    """(index, item, val) as primalcr_amd.fold_in takes them."""
    return X.idx, X.item.astype(np.int32), X.val
