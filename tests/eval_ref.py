"""The evaluator's definition in plain numpy (tests/test_eval_exact.py): compute_pairwise_error_ndcg (util.cpp:434-542) with the
tie convention this project has chosen, so that a result is integer counts and a defined order, not a summation order.

Per user, from the scores s (CSR order), the raw ratings v and ndcg_k:
    bad    = #{ordered (a, b): s_a >= s_b and v_a < v_b}           a score tie counts as an error
    npairs = n (n - 1) / 2
    top    = the min(k, n) indices by (score descending, index ascending)
    dcg    = sum_pos (2^v[top[pos-1]] - 1) / log2(pos + 1),  idcg the same over the ratings sorted descending
    error  = mean bad / npairs over the users with n >= 2,  ndcg = mean dcg / idcg over the users with n >= 1
bad is a Python int, the error mean is a Fraction rounded once, every floating sum is math.fsum: the reference's own summation
order is not a variable.

Mutants (CPU precondition test only -- they show that the fixture can tell a wrong kernel from a right one):
    tie_high   ties in the top-k broken by the HIGHER index
    strict     s_a > s_b instead of s_a >= s_b
    lround     ratings bucketed by lround (the solver's PrimalCR++ levels) instead of compared raw
"""
import math
from fractions import Fraction

import numpy as np

MUTANTS = (None, "tie_high", "strict", "lround")


class UserTerms:
    """One user's terms: n, bad, npairs (ints), and per k the top indices, dcg and idcg."""

    def __init__(self, u, n, bad, npairs):
        self.u, self.n, self.bad, self.npairs = u, n, bad, npairs
        self.top, self.dcg, self.idcg = {}, {}, {}

    def line(self, k):
        err = f"{self.bad}/{self.npairs}" if self.npairs else "-"
        return f"user {self.u}: n {self.n} bad/npairs {err} dcg {self.dcg[k]!r} idcg {self.idcg[k]!r} top {self.top[k][:8].tolist()}"


class Result:
    """error, ndcg (floats; nan for 0/0), the counts of users behind each mean, and the per-user terms."""

    def __init__(self, k, users):
        self.k, self.users = k, users
        pairs = [t for t in users if t.npairs > 0]
        rated = [t for t in users if t.n > 0]
        self.n_err, self.n_ndcg = len(pairs), len(rated)
        self.error = float(sum(Fraction(t.bad, t.npairs) for t in pairs) / len(pairs)) if pairs else math.nan
        self.ndcg = math.fsum(t.dcg[k] / t.idcg[k] for t in rated) / len(rated) if rated else math.nan

    def detail(self):
        return "\n".join(t.line(self.k) for t in self.users if t.n > 0)


def count_bad(s, v, strict=False, block=512):
    """#{ordered (a, b): s_a >= s_b and v_a < v_b}, block by block, as a Python int."""
    n = s.shape[0]
    bad = 0
    for b0 in range(0, n, block):
        sa, va = s[b0:b0 + block, None], v[b0:b0 + block, None]
        ge = (sa > s[None, :]) if strict else (sa >= s[None, :])
        bad += int((ge & (va < v[None, :])).sum())
    return bad


def top_indices(s, k, tie_high=False):
    """The min(k, n) indices by (score descending, index ascending); tie_high: index descending."""
    idx = np.arange(s.shape[0])
    order = np.lexsort((-idx if tie_high else idx, -s))                    # last key is the primary one
    return order[:min(k, s.shape[0])]


def dcg_of(gains):
    return math.fsum(float(g) / math.log2(pos + 2.0) for pos, g in enumerate(gains))


def scores(U, V, idx, item):
    """s[z] = U[user of z] . V[item[z]] in fp64, CSR order."""
    U = np.asarray(U, np.float64); V = np.asarray(V, np.float64)
    rows = np.repeat(np.arange(idx.shape[0] - 1), np.diff(idx))
    return (U[rows] * V[np.asarray(item, np.int64)]).sum(1)


def evaluate(U, V, idx, item, val, ks, mutant=None, users=None):
    """{k: Result} over the users `users` (default: all) of the CSR (idx, item, val)."""
    assert mutant in MUTANTS
    idx = np.asarray(idx, np.int64); val = np.asarray(val, np.float64)
    s_all = scores(U, V, idx, item)
    v_all = np.rint(val) if mutant == "lround" else val
    ks = tuple(ks)
    terms = []
    for u in (range(idx.shape[0] - 1) if users is None else users):
        a, b = int(idx[u]), int(idx[u + 1])
        s, v, n = s_all[a:b], v_all[a:b], b - a
        t = UserTerms(int(u), n, count_bad(s, v, strict=mutant == "strict") if n >= 2 else 0, n * (n - 1) // 2)
        if n:
            order = top_indices(s, max(ks), tie_high=mutant == "tie_high")
            ideal = np.sort(v)[::-1]
            for k in ks:
                t.top[k] = order[:k]
                t.dcg[k] = dcg_of(2.0 ** v[order[:k]] - 1.0)
                t.idcg[k] = dcg_of(2.0 ** ideal[:k] - 1.0)
        terms.append(t)
    return {k: Result(k, terms) for k in ks}
