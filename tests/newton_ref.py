"""The exact-Newton U step of one user from its definition, in numpy fp64 and with no window logic: the plain reference of
tests/test_newton_exact.py.  Nothing here sorts, searches or keeps prefix sums; every pair of the user's ratings is looked at.

    m = X u                                     X: the user's rows of V, in CSR order
    pair (j, k) is comparable when level_j > level_k, and then ACTIVE when m_j - m_k <= 1 (PrimalCR++) or < 1 (PrimalCR)
    objective   lambda / 2 |u|^2 + sum over comparable pairs of max(0, 1 - (m_j - m_k))^2
    g = lambda u + X^T c,   c_j = -2 sum_k h_jk + 2 sum_i h_ij,   h_jk = max(0, 1 - (m_j - m_k)) over comparable pairs
    A: the symmetric adjacency of the active pairs,   L = diag(A 1) - A,   H = lambda I + 2 X^T L X
    delta = solve(H, g);  try u - s delta for s = 1, 1/2, ... (at most 20 tries), accept the first objective < the old one
    skipped (u kept, no try): no rating, |g|^2 < 1e-4, PrimalCR with at most one level

H is formed as lambda I + 2 X^T (diag(deg) X - A X), the shape in which the mutants below can take one mechanism of k_unewton away.

MUTANTS: each is a way in which the kernel could be wrong at one of its edges, applied to the REFERENCE alone (tests on the CPU
prove that the per-user bound sees it, and that it touches nobody outside its group).  They model the kernel, so they apply to
covered users only (1..NEWTON_MAX_N ratings, ld <= NEWTON_MAX_LD).
    slots4to7    the partners inside the fifth to eighth OTHER level are missing from A X (the unprefetched window slots); users
                 of 6..9 levels
    strictness   boundary pairs (m_j - m_k = 1 exactly) counted under PrimalCR and not under PrimalCR++; users that have one
    chunk_tail   the last n mod 16 rows of the sorted order are missing from X^T (L X); users whose n is no multiple of 16
    degree       one rating's degree term is missing; users with an active pair
    beyond64     H's off-diagonal entries in rows and columns from 64 up are zero (the diagonal stays: a zero row would make the
                 mutant singular, not wrong); users with an active pair at ranks above 64
"""
import numpy as np

MUTANTS = ("slots4to7", "strictness", "chunk_tail", "degree", "beyond64")
MAX_TRIES = 20


def objective(X, u, above, lam):
    m = X @ u
    h = np.where(above, np.maximum(0.0, 1.0 - (m[:, None] - m[None, :])), 0.0)
    return lam / 2.0 * float(u @ u) + float((h * h).sum())


def user_step(X, u, lev, lam, solver, covered=True, mutant=None):
    """One user's step.  X: n x r, u: r, lev: the n levels the solver compares.  Returns a dict: row, delta, s (0.0: skipped or never
    accepted), tries, accepted, cond, margins (|obj_try - prev_obj| / prev_obj of every try), levels, n, boundary (comparable pairs
    with m_j - m_k = 1 exactly), active (active pairs), in_group (the mutant's targeted group contains this user)."""
    n, r = X.shape
    u = np.asarray(u, np.float64)
    out = dict(row=u.copy(), delta=np.zeros(r), s=0.0, tries=0, accepted=False, cond=1.0, margins=[], levels=0, n=n, boundary=0,
               active=0, in_group=False)
    if n == 0:
        return out
    li = np.unique(lev, return_inverse=True)[1].astype(np.int64)
    nlev = out["levels"] = int(li.max()) + 1
    m = X @ u
    above = li[:, None] > li[None, :]                                # [j, k]: j's level above k's
    D = m[:, None] - m[None, :]
    h = np.where(above, np.maximum(0.0, 1.0 - D), 0.0)
    prev = lam / 2.0 * float(u @ u) + float((h * h).sum())
    g = lam * u + X.T @ (-2.0 * h.sum(1) + 2.0 * h.sum(0))
    edge = above & (D == 1.0)
    out["boundary"] = int(edge.sum())
    inclusive = solver == 2
    if mutant == "strictness" and covered:
        inclusive = not inclusive
        out["in_group"] = out["boundary"] > 0
    act = above & ((D <= 1.0) if inclusive else (D < 1.0))
    A = (act | act.T).astype(np.float64)
    out["active"] = int(act.sum())
    deg = A.sum(1)
    if mutant == "degree" and covered and out["active"] > 0:
        deg[np.flatnonzero(deg)[0]] = 0.0
        out["in_group"] = True
    if mutant == "slots4to7" and covered and 6 <= nlev <= 9:
        slot = li[None, :] - (li[None, :] > li[:, None])              # [p, q]: q's level as one of p's other levels
        A = np.where((slot >= 4) & (slot <= 7), 0.0, A)
        out["in_group"] = True
    Y = deg[:, None] * X - A @ X
    Xt = X
    if mutant == "chunk_tail" and covered and n % 16:
        keep = np.lexsort((m, li))[:n - n % 16]                      # the sorted order: by level, then by score
        Xt, Y = X[keep], Y[keep]
        out["in_group"] = True
    H = lam * np.eye(r) + 2.0 * Xt.T @ Y
    if mutant == "beyond64" and covered and r > 64 and out["active"] > 0:
        d = np.diag(H).copy()
        H[64:, :] = 0.0; H[:, 64:] = 0.0
        H[np.arange(64, r), np.arange(64, r)] = d[64:]
        out["in_group"] = True
    if float(g @ g) < 1e-4 or (solver != 2 and nlev <= 1):
        return out
    w = np.linalg.eigvalsh((H + H.T) / 2.0)                          # H is symmetric positive definite (a mutant's may not be: unused there)
    out["cond"] = float(w[-1] / w[0]) if w[0] > 0 else np.inf
    delta = out["delta"] = np.linalg.solve(H, g)
    s = 1.0
    for _ in range(MAX_TRIES):
        row = u - s * delta
        obj = objective(X, row, above, lam)
        out["tries"] += 1
        out["margins"].append(abs(obj - prev) / prev)
        out["row"] = row
        if obj < prev:
            out["accepted"] = True
            out["s"] = s
            break
        s /= 2.0
    return out


def shard_step(c, U, V, lev, covered, mutant=None):
    """user_step for every user of the case c (d1, idx, item, lam, solver) from the factors (U, V).  lev: every rating's level in
    CSR order; covered: bool per user.  Returns (U_new, list of the per-user dicts)."""
    Un = np.array(U, np.float64)
    info = []
    for u in range(c.d1):
        s, e = int(c.idx[u]), int(c.idx[u + 1])
        o = user_step(V[c.item[s:e]], U[u], lev[s:e], c.lam, c.solver, bool(covered[u]), mutant)
        Un[u] = o["row"]
        info.append(o)
    return Un, info
