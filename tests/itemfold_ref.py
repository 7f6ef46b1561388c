"""Plain-numpy fp64 reference of the item fold-in (include/primalcr.h, "item fold-in") for tests/test_foldin_items.py.

``Model``          U, V, the training CSR and its scores m = u_i . v_k.
``Item``           one new item: F_j, its gradient and its Hessian-vector product BY ALL PAIRS (every training rating of every
                   rater against the new rating), vectorised over the flattened rows of its raters.
``fold_in_item``   the loop of rules 1-6, restated from the header.
``minimise``       v* by a full Newton iteration to |g| < 1e-12 (the strong-convexity anchor).
``appended``       the training CSR with one new item appended, for the anchors on the in-tree oracle.
``make_fixture``   the fixture: training rows with planted lengths, one new item per rater count, the special cases.
"""
import numpy as np

from foldin_ref import CONVERGED, STALLED, STEP_CAP, levels_of
from oracle.oracle_py import CSR

__all__ = ["CONVERGED", "STEP_CAP", "STALLED", "Model", "Item", "fold_in_item", "fold_in_items", "minimise", "appended", "make_fixture"]


class Model:
    def __init__(self, U, V, X, solver, lam):
        self.U, self.V, self.X = np.ascontiguousarray(U, np.float64), np.ascontiguousarray(V, np.float64), X
        self.solver, self.lam = int(solver), float(lam)
        rows = np.repeat(np.arange(X.d1), np.diff(X.idx))
        self.m = np.einsum("ij,ij->i", self.U[rows], self.V[X.item]) if X.nnz else np.zeros(0)
        self.lev = levels_of(X.val, solver)


class Item:
    """New item with raters `users` (ids of U's rows) and their ratings `vals`; the raters are taken in ascending user order."""

    def __init__(self, M, users, vals, table_dtype=np.float64):
        users = np.asarray(users, np.int64); vals = np.asarray(vals, np.float64)
        o = np.argsort(users, kind="stable")
        self.users, self.vals, self.M = users[o], vals[o], M
        n = self.n = len(users)
        lens = np.diff(M.X.idx)[self.users] if n else np.zeros(0, np.int64)
        self.seg = np.repeat(np.arange(n), lens)
        starts = np.concatenate([[0], np.cumsum(lens)])[:-1] if n else np.zeros(0, np.int64)
        self.flat = (M.X.idx[self.users][self.seg] + (np.arange(int(lens.sum())) - starts[self.seg])).astype(np.int64)
        lev = M.lev[self.flat]
        lr = levels_of(self.vals, M.solver)[self.seg] if n else np.zeros(0)
        self.sg = np.where(lev < lr, 1.0, np.where(lev > lr, -1.0, 0.0))          # +1: the new item is to score above that rating
        self.m = M.m[self.flat].astype(table_dtype).astype(np.float64)
        self.UR = M.U[self.users]
        self.anypair = bool((self.sg != 0).any())

    def state(self, s):
        """(phi, c[i], h[i]) at the raters' scores s, in the type of s (float64; minimise() passes long doubles)."""
        d = 1.0 - self.sg * (s[self.seg] - self.m)
        act = (self.sg != 0) & ((d > 0) if self.M.solver == 1 else (d >= 0))
        dd = np.where(act, d, 0.0)
        phi = dd @ dd
        h = 2.0 * np.bincount(self.seg, weights=act.astype(np.float64), minlength=self.n)
        if s.dtype == np.float64:
            return float(phi), np.bincount(self.seg, weights=-2.0 * self.sg * dd, minlength=self.n), h
        c = np.zeros(self.n, s.dtype)
        np.add.at(c, self.seg, -2.0 * self.sg * dd)
        return phi, c, h

    def F(self, v):
        return self.M.lam / 2.0 * float(v @ v) + self.state(self.UR @ v)[0]

    def grad(self, v):
        return self.M.lam * v + self.UR.T @ self.state(self.UR @ v)[1]

    def Hv(self, v, a):
        return self.M.lam * a + self.UR.T @ (self.state(self.UR @ v)[2] * (self.UR @ a))


def fold_in_item(it, v0, steps, stepsize=1.0, cg_max=10, cg_tol=0.01, dtype=np.float64):
    """Rules 1-6 of the header.  dtype: the storage type the point, the scores and c are rounded to (float32 imitates the fp32
    call's roundings in fp64 sums; the comparisons with the device use float64).  Returns (v, per) with per a dict of
    PCR_ITEMFOLD_FIELDS, plus gn2_seen (|g|^2 at every point where the end test ran) and min_dec (the smallest relative decrease of
    an accepted try)."""
    T = lambda x: np.asarray(x, np.float64).astype(dtype).astype(np.float64)
    lam = it.M.lam
    v = T(v0)
    per = dict(raters=it.n, steps=0, cg=0, ls=0, obj0=0.0, obj=0.0, gnorm2=0.0, status=STEP_CAP, gn2_seen=[], min_dec=np.inf)

    def evaluate(x):
        phi, c, h = it.state(T(it.UR @ x)) if it.n else (0.0, np.zeros(0), np.zeros(0))
        return phi, T(c), h

    loss, c, h = evaluate(v)
    for step in range(steps):
        g = lam * v + it.UR.T @ c if it.n else np.zeros_like(v)
        gn2 = float(g @ g)
        prev = lam / 2.0 * float(v @ v) + loss
        if step == 0:
            per["obj0"] = prev
        per["gnorm2"] = gn2
        per["gn2_seen"].append(gn2)
        if it.n == 0 or gn2 < 1e-4 or (it.M.solver == 1 and not it.anypair):
            per["status"] = CONVERGED
            break
        delta = np.zeros_like(v); r = -g; p = g.copy()
        err = np.sqrt(gn2) * cg_tol
        for _ in range(cg_max):
            pT = T(p)
            Hp = lam * p + it.UR.T @ T(h * T(it.UR @ pT))
            per["cg"] += 1
            pHp = float(p @ Hp)
            alpha = -float(r @ p) / pHp
            delta = delta + alpha * p
            r = r + alpha * Hp
            if np.sqrt(float(r @ r)) < err:
                break
            p = -r + (float(r @ Hp) / pHp) * p
        sl, accepted = stepsize, False
        for _ in range(20):
            vn = T(v - sl * delta)
            ln, cn, hn = evaluate(vn)
            per["ls"] += 1
            if lam / 2.0 * float(vn @ vn) + ln < prev:
                accepted = True
                break
            sl /= 2.0
        if not accepted:
            per["status"] = STALLED
            break
        per["min_dec"] = min(per["min_dec"], (prev - (lam / 2.0 * float(vn @ vn) + ln)) / abs(prev))
        v, loss, c, h = vn, ln, cn, hn
        per["steps"] += 1
    per["obj"] = lam / 2.0 * float(v @ v) + loss
    return v, per


def fold_in_items(M, items, V0, steps, want_per=False, **kw):
    """fold_in_item over (users, vals) pairs: returns (rows [n, k], table [n, 8] in PCR_ITEMFOLD_FIELDS order[, the per dicts])."""
    rows = np.zeros((len(items), M.U.shape[1]))
    tab = np.zeros((len(items), 8))
    pers = []
    for j, (users, vals) in enumerate(items):
        rows[j], per = fold_in_item(Item(M, users, vals), V0[j], steps, **kw)
        tab[j] = [per[f] for f in ("raters", "steps", "cg", "ls", "obj0", "obj", "gnorm2", "status")]
        pers.append(per)
    return (rows, tab, pers) if want_per else (rows, tab)


def minimise(it, v0=None, tol=1e-12, max_iter=200):
    """v* = argmin F_j by Newton steps on the explicit generalised Hessian with a halving line search, to |g| < tol.  The point,
    F_j and its gradient are held in long double (an item of 2000 raters has an fp64 gradient noise of about tol); the Newton
    direction is solved in fp64.  Returns (v* as float64, |g| there)."""
    L = np.longdouble
    k = it.M.U.shape[1]
    lam, UR = L(it.M.lam), it.UR.astype(L)
    v = np.zeros(k, L) if v0 is None else np.array(v0, L)
    gn = L(np.inf)
    for _ in range(max_iter):
        phi, c, h = it.state(UR @ v)
        g = lam * v + UR.T @ c
        gn = np.sqrt(g @ g)
        if gn < tol:
            break
        H = it.M.lam * np.eye(k) + (it.UR.T * h) @ it.UR
        d = np.linalg.solve(H, g.astype(np.float64)).astype(L)
        f0, sl = lam / 2 * (v @ v) + phi, L(1.0)
        for _ in range(60):                                         # (near v* a decrease of F_j is below its resolution: |g| decides)
            vn = v - sl * d
            phin, cn, _ = it.state(UR @ vn)
            gv = lam * vn + UR.T @ cn
            if lam / 2 * (vn @ vn) + phin < f0 or np.sqrt(gv @ gv) < gn:
                break
            sl /= 2
        else:
            break
        v = vn
    return v.astype(np.float64), float(gn)


def appended(X, users, vals):
    """X with a new item d2 appended at the end of the row of every rater (a rater listed twice gets it twice)."""
    users = np.asarray(users, np.int64)
    add = np.bincount(users, minlength=X.d1)
    idx = np.concatenate([[0], np.cumsum(np.diff(X.idx) + add)])
    item = np.empty(int(idx[-1]), np.int64); val = np.empty(int(idx[-1]))
    fill = idx[:-1] + np.diff(X.idx)
    for i in range(X.d1):
        a, b = int(X.idx[i]), int(X.idx[i + 1])
        item[idx[i]:idx[i] + b - a] = X.item[a:b]; val[idx[i]:idx[i] + b - a] = X.val[a:b]
    fill = fill.copy()
    for u, r in zip(users, vals):
        item[fill[u]] = X.d2; val[fill[u]] = r
        fill[u] += 1
    return CSR(X.d1, X.d2 + 1, idx, item, val)


# ------------------------------------------------------------------------------------------------------------------------------
# the fixture
# ------------------------------------------------------------------------------------------------------------------------------
D2 = 300
EMPTY_USER, ONE_RATING_USER, ONE_LEVEL_USER = 0, 1, 2
GAP_USERS = (3, 4, 5)                                  # rows that hold two levels with a free level between them
LONG_USERS = {10: 63, 11: 64, 12: 65, 13: 300, 14: 2100}


def draw_ratings(rng, n, solver):
    """As foldin_ref.make_users draws them: integers 1..5 for PrimalCR++, quarter steps + 0.125 for PrimalCR."""
    return rng.integers(1, 6, size=n).astype(np.float64) if solver == 2 else 1.125 + 0.25 * rng.integers(0, 20, size=n)


def make_fixture(solver, d1, rater_counts, seed=7):
    """Returns (X, items, names): the training CSR of d1 users over D2 items (most rows 1-8 ratings; the planted rows above; a
    row longer than D2 repeats items: the same item twice is two ratings) and the new items as (users, vals) pairs -- one per
    rater count, then the special cases named in `names` ("restart" repeats the item of the most raters: the tests start it
    where the reference's loop left that item)."""
    rng = np.random.default_rng(seed)
    lo, hi, mid = (2.0, 4.0, 3.0) if solver == 2 else (1.625, 2.625, 2.125)
    idx, items_, vals_ = [0], [], []
    for u in range(d1):
        n = LONG_USERS.get(u, int(rng.integers(1, 9)))
        if u == EMPTY_USER:
            n = 0
        elif u == ONE_RATING_USER:
            n = 1
        elif u == ONE_LEVEL_USER:
            n = 3
        elif u in GAP_USERS:
            n = 6
        it = np.sort(rng.choice(D2, size=n, replace=n > D2))
        v = draw_ratings(rng, n, solver)
        if u == ONE_LEVEL_USER:
            v[:] = v[0]
        elif u in GAP_USERS:
            v = np.array([lo, hi, lo, hi, hi, lo])
        items_.append(it); vals_.append(v); idx.append(idx[-1] + n)
    X = CSR(d1, D2, np.array(idx), np.concatenate(items_), np.concatenate(vals_))
    items, names = [], []
    for c in rater_counts:
        users = rng.choice(d1, size=c, replace=False)
        items.append((users, draw_ratings(rng, c, solver))); names.append(f"count{c}")
    tie_users = np.array([ONE_LEVEL_USER, ONE_RATING_USER])
    items.append((tie_users, np.array([X.val[X.idx[u]] for u in tie_users]))); names.append("ties")
    items.append((np.array([13, 40, 13]), draw_ratings(rng, 3, solver) + np.array([0.0, 0.0, 1.0]))); names.append("dup")
    items.append((np.array([EMPTY_USER]), draw_ratings(rng, 1, solver))); names.append("empty_rater")
    items.append((np.array(GAP_USERS), np.full(len(GAP_USERS), mid))); names.append("gap")
    items.append((np.array(sorted(LONG_USERS)), draw_ratings(rng, len(LONG_USERS), solver))); names.append("long_raters")
    items.append(items[names.index(f"count{max(rater_counts)}")]); names.append("restart")      # the longest item again, for a start of its own
    return X, items, names


def item_csr(items):
    """(index int64, user int32, val float64) as primalcr_amd.fold_in_items takes the new items."""
    index = np.concatenate([[0], np.cumsum([len(u) for u, _ in items])]).astype(np.int64)
    user = np.concatenate([np.asarray(u, np.int64) for u, _ in items]).astype(np.int32) if items else np.zeros(0, np.int32)
    val = np.concatenate([np.asarray(v, np.float64) for _, v in items]) if items else np.zeros(0)
    return index, user, val
