"""Beyond-accuracy top-N metrics (pcr_evaluate_diversity_model / pcr_evaluate_diversity / pcr_exposure_stats,
omp-pmf-recommend --diversity, Python evaluate_diversity()): catalogue coverage, Gini index of item exposure, novelty, ILD.

CPU part: argument checks of the C ABI, the "no device" error, exposure_stats against Python big-integer arithmetic (==), the
CLI's usage text and argument errors, the header's field count.
GPU part (-m gpu): in every test the lists come from recommend() with the same arguments (its exactness is held by
test_recommend.py / test_recommend_grid.py) and numpy applies the contract of include/primalcr.h to those lists.  len, exposure,
recs, items_covered, coverage and gini must be equal (==); novelty is held to 1e-12 relative; ILD to 1e-10 absolute (the kernel's
error is bounded by about 6 (k + 2) 2^-52 = 3e-13 at k = 256 and the pairwise numpy reference carries about the same, while one
missing pair at K = 1024 moves ILD by about 2e-6).
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import BIN_DIR, ROOT
from test_recommend import special_csr
from test_recommend_grid import D_CASES, boundary_row, int_factors, random_csr, rec_geometry, splits_of

RECOMMEND = os.path.join(BIN_DIR, "omp-pmf-recommend")
TRAIN = os.path.join(BIN_DIR, "omp-pmf-train")
ERR_ARG, ERR_DEVICE, ERR_UNSUPPORTED = -1, -4, -7
NOV_RTOL, ILD_ATOL = 1e-12, 1e-10


def run(cmd, cwd, timeout=600):
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=timeout)


def _model_call(U, V, index, item, users, cutoffs, dtype=1, n=None, stats=True):
    """pcr_evaluate_diversity_model through ctypes, arrays as given (None = NULL); returns the status code."""
    import primalcr_amd as pcr
    n = (len(users) if users is not None else U.shape[0]) if n is None else n
    cuts = None if cutoffs is None else np.asarray(cutoffs, np.int32)
    st = (pcr.DiversityStats * 16)()
    ptr = lambda a: None if a is None else a.ctypes.data
    return pcr.lib().pcr_evaluate_diversity_model(ptr(U), U.shape[0], ptr(V), V.shape[0], U.shape[1], ptr(index), ptr(item), n, ptr(users),
                                                  0 if cuts is None else len(cuts), ptr(cuts), dtype, C.cast(st, C.c_void_p) if stats else None,
                                                  None, None, 0)


def ref_exposure_stats(x):
    """The contract's closing arithmetic in Python integers: (recs, items_covered, coverage, gini)."""
    xs = sorted(int(v) for v in x)
    d2 = len(xs)
    tot = sum(xs)
    cov = sum(1 for v in xs if v > 0)
    num = sum((2 * (i + 1) - d2 - 1) * v for i, v in enumerate(xs))
    return tot, cov, float(cov) / float(d2), (float(num) / float(d2 * tot) if tot else 0.0)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_model_entry_argument_checks():
    import primalcr_amd as pcr
    rng = np.random.default_rng(1)
    U, V = rng.standard_normal((20, 5)), rng.standard_normal((30, 5))
    index = np.array([0] + [2] * 20, np.int64)
    item = np.array([3, 7], np.int32)
    users = np.arange(20, dtype=np.int32)

    def bad(*a, **kw):
        assert _model_call(*a, **kw) == ERR_ARG
        assert b"pcr_evaluate_diversity_model" in pcr.lib().pcr_last_error()

    bad(U, V, index, item, users, [0])
    bad(U, V, index, item, users, [])
    bad(U, V, index, item, users, None)
    bad(U, V, index, item, users, list(range(1, 10)))                  # more than 8
    bad(U, V, index, item, users, [10, 5])
    bad(U, V, index, item, users, [5, 5])
    bad(U, V, index, item, users, [10, 1025])
    bad(U, V, index, item, users, [10], dtype=5)
    bad(U, V, index, item, users, [10], stats=False)
    bad(U, V, index, item, np.array([0, 20], np.int32), [10])
    bad(U, V, index, item, np.array([-1], np.int32), [10])
    bad(U, V, index, item, None, [10], n=21)                           # more users than the model without a list
    nm = index.copy(); nm[5] = 1                                        # not monotone
    bad(U, V, nm, item, users, [10])
    bad(U, V, index, np.array([3, 30], np.int32), users, [10])         # item outside the model
    bad(U, V, index, None, users, [10])                                # index without item
    nz = index.copy(); nz[0] = 1
    bad(U, V, nz, item, users, [10])
    with pytest.raises(pcr.PcrError):
        pcr.evaluate_diversity(U, V, cutoffs=(0,))
    with pytest.raises(ValueError):
        pcr.evaluate_diversity(U, V, exclude=(index, np.array([3, 7, 9], np.int32)))
    # the solver entry checks its solver first
    st = (pcr.DiversityStats * 1)()
    one = np.array([5], np.int32)
    assert pcr.lib().pcr_evaluate_diversity(None, 0, None, 1, one.ctypes.data, 0, C.cast(st, C.c_void_p), None, None) == ERR_ARG


def test_model_entry_without_a_device_is_a_device_error():
    code = ("import sys, numpy as np; sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')\n"
            "from test_diversity import _model_call\n"
            "U = np.ones((4, 3)); V = np.ones((6, 3))\n"
            "print(_model_call(U, V, np.array([0, 1, 1, 1, 1], np.int64), np.array([2], np.int32), np.arange(4, dtype=np.int32), [1, 3]))\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    assert int(out.stdout.strip().splitlines()[-1]) == ERR_DEVICE


def test_exposure_stats_against_big_integers():
    import primalcr_amd as pcr
    rng = np.random.default_rng(5)

    def same(x):
        got = pcr.exposure_stats(x)
        assert (got["recs"], got["items_covered"], got["coverage"], got["gini"]) == ref_exposure_stats(x)
        return got

    for d2 in (1, 2, 7, 3706):
        g = same(np.full(d2, 11, np.int64))                            # uniform
        assert g["gini"] == 0.0 and g["coverage"] == 1.0 and g["recs"] == 11 * d2
        x = np.zeros(d2, np.int64); x[d2 // 2] = 12345                 # one item only
        g = same(x)
        assert g["gini"] == (d2 - 1) / d2 and g["items_covered"] == 1
        g = same(np.zeros(d2, np.int64))
        assert (g["recs"], g["items_covered"], g["coverage"], g["gini"]) == (0, 0, 0.0, 0.0)
        same(rng.integers(0, 1000, d2))
        same(rng.integers(0, 3, d2))
    same(rng.integers(0, 1 << 40, 17770))                               # sums beyond 2^53, products beyond 2^64
    same(np.full(100000, (1 << 62) // 100000, np.int64))
    with pytest.raises(pcr.PcrError):
        pcr.exposure_stats(np.array([1, -1], np.int64))


def test_exposure_stats_refuses_a_total_beyond_int64():
    """recs is an int64: a caller-summed row whose total does not fit is an argument error, not a wrapped count; the largest
    total that fits is still exact."""
    import primalcr_amd as pcr
    top = (1 << 63) - 1
    for x in ([top, 1], [1 << 62, 1 << 62], [top // 3 + 1] * 3):
        with pytest.raises(pcr.PcrError, match="pcr_exposure_stats"):
            pcr.exposure_stats(np.array(x, np.int64))
    for x in ([top], [top - 5, 0, 5], [1 << 62, (1 << 62) - 1]):
        got = pcr.exposure_stats(np.array(x, np.int64))
        assert (got["recs"], got["items_covered"], got["coverage"], got["gini"]) == ref_exposure_stats(x) and got["recs"] == top


def test_cli_usage_and_argument_errors(tmp_path):
    import primalcr_amd as pcr
    from primalcr_amd import synth
    r = run([RECOMMEND], tmp_path)
    assert r.returncode == 1 and "--diversity" in r.stdout and r.stdout.startswith("Usage: omp-pmf-recommend [-K topk]")
    R = synth.generate("tiny", seed=3)
    d = synth.write_dir(R, str(tmp_path / "data"))
    r = run([RECOMMEND, "--diversity", "--eval", d, str(tmp_path / "missing.model")], tmp_path)   # before the model is read
    assert r.returncode == 1 and "--diversity" in r.stderr and "can't open" not in r.stderr
    rng = np.random.default_rng(2)
    pcr.model_save(str(tmp_path / "ok.model"), rng.standard_normal((R.d1, 4)), rng.standard_normal((R.d2, 4)))
    r = run([RECOMMEND, "--diversity", "-x", str(tmp_path / "missing_dir"), "ok.model"], tmp_path)
    assert r.returncode == 1 and r.stderr
    r = run([RECOMMEND, "--diversity", "-c", "10,5", "ok.model"], tmp_path)
    assert r.returncode == 1 and "-c" in r.stderr
    r = run([RECOMMEND, "--diversity"], tmp_path)
    assert r.returncode == 1 and r.stdout.startswith("Usage: omp-pmf-recommend")
    r = run([RECOMMEND, "--diversity", "--scores", "ok.model"], tmp_path)
    assert r.returncode == 1 and "--diversity" in r.stderr


def test_header_field_count():
    import primalcr_amd as pcr
    hdr = open(os.path.join(ROOT, "include", "primalcr.h")).read()
    m = re.search(r"#define PCR_DIVERSITY_FIELDS (\d+)", hdr)
    assert m and int(m.group(1)) == len(pcr.DIVERSITY_FIELDS) == 3
    assert pcr.DIVERSITY_FIELDS == ("len", "novelty", "ild")
    assert [f for f, _ in pcr.DiversityStats._fields_] == ["cutoff", "users", "users_ild", "recs", "items_covered", "coverage", "gini",
                                                           "novelty", "ild"]


# ---------------------------------------------------------------------------------------------------------------- GPU helpers
def ref_info(d1, d2, item):
    pop = np.bincount(item, minlength=d2).astype(np.float64) if item is not None else np.zeros(d2)
    return np.log2(float(d1 + 1) / (pop + 1.0))


def unit_rows(V, f32):
    Vd = V.astype(np.float32).astype(np.float64) if f32 else np.asarray(V, np.float64)
    nrm = np.sqrt((Vd * Vd).sum(1))
    return np.where(nrm[:, None] > 0, Vd / np.where(nrm > 0, nrm, 1.0)[:, None], 0.0)


def ref_diversity(items, V, info, cutoffs, f32, want_rows=True):
    """The contract on the lists `items` [n, K]: (per_user [n, ncut, 3], exposure int64 [ncut, d2], summary dicts)."""
    n, d2 = items.shape[0], V.shape[0]
    Vh = unit_rows(V, f32)
    per = np.full((n, len(cutoffs), 3), np.nan)
    expo = np.zeros((len(cutoffs), d2), np.int64)
    for ci, c in enumerate(cutoffs):
        head = items[:, :c]
        expo[ci] = np.bincount(head[head >= 0], minlength=d2)
        per[:, ci, 0] = (head >= 0).sum(1)
    for i in range(n if want_rows else 0):
        l = items[i][items[i] >= 0]
        G = np.triu(Vh[l] @ Vh[l].T, 1)
        for ci, c in enumerate(cutoffs):
            m = min(c, l.shape[0])
            if m >= 1:
                per[i, ci, 1] = info[l[:m]].sum() / m
            if m >= 2:
                per[i, ci, 2] = 1.0 - G[:m, :m].sum() / (m * (m - 1) / 2)
    out = []
    for ci, c in enumerate(cutoffs):
        recs, cov, coverage, gini = ref_exposure_stats(expo[ci])
        nov, ild = per[:, ci, 1], per[:, ci, 2]
        out.append(dict(cutoff=c, users=n, users_ild=int((~np.isnan(ild)).sum()), recs=recs, items_covered=cov, coverage=coverage, gini=gini,
                        novelty=float(np.nanmean(nov)) if (~np.isnan(nov)).any() else 0.0,
                        ild=float(np.nanmean(ild)) if (~np.isnan(ild)).any() else 0.0))
    return per, expo, out


def check_rows(pu, want, what=None):
    assert np.array_equal(pu[..., 0], want[..., 0]), what
    for f, (rtol, atol) in ((1, (NOV_RTOL, 0.0)), (2, (0.0, ILD_ATOL))):
        assert np.array_equal(np.isnan(pu[..., f]), np.isnan(want[..., f])), (what, f)
        ok = ~np.isnan(want[..., f])
        err = np.abs(pu[..., f][ok] - want[..., f][ok])
        assert np.all(err <= atol + rtol * np.abs(want[..., f][ok])), (what, f, err.max() if err.size else 0.0)


def check_summary(got, want, rows=True, what=None):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for f in ("cutoff", "users", "recs", "items_covered", "coverage", "gini"):
            assert g[f] == w[f], (what, f, g, w)
        if rows:
            assert g["users_ild"] == w["users_ild"], (what, g, w)
            assert abs(g["novelty"] - w["novelty"]) <= NOV_RTOL * abs(w["novelty"]) + 1e-300, (what, g, w)
            assert abs(g["ild"] - w["ild"]) <= ILD_ATOL, (what, g, w)


def check_call(U, V, cutoffs, exclude, users, dtype, what=None):
    """evaluate_diversity against numpy on recommend()'s lists; returns (summary, per_user, exposure)."""
    import primalcr_amd as pcr
    items, _ = pcr.recommend(U, V, cutoffs[-1], exclude=exclude, users=users, dtype=dtype)
    info = ref_info(U.shape[0], V.shape[0], None if exclude is None else exclude[1])
    want_pu, want_ex, want = ref_diversity(items, V, info, cutoffs, dtype == 0)
    got, pu, ex = pcr.evaluate_diversity(U, V, cutoffs=cutoffs, exclude=exclude, users=users, dtype=dtype, per_user=True, exposure=True)
    assert ex.dtype == np.int64 and np.array_equal(ex, want_ex), what
    check_rows(pu, want_pu, what)
    check_summary(got, want, what=what)
    return got, pu, ex


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.timeout(1200)
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
def test_integer_factors_against_numpy(dtype):
    rng = np.random.default_rng(111 + dtype)
    d1, cutoffs = 150, (1, 10, 100, 1024)
    zero_rows = False
    for k in (1, 7, 64, 100, 130):
        for d2 in (1, 63, 64, 65, 1000, 3706):
            U = rng.integers(-2, 3, (d1, k)).astype(np.float64)
            V = rng.integers(-2, 3, (d2, k)).astype(np.float64)
            zero_rows |= bool((np.abs(V).sum(1) == 0).any()) and d2 > 1
            index, item = special_csr(rng, d1, d2)
            check_call(U, V, cutoffs, (index, item), None, dtype, (k, d2))
            if d2 in (65, 3706):
                check_call(U, V, (10,), None, None, dtype, (k, d2, "no exclusion"))
                users = rng.integers(0, d1, 70).astype(np.int32)          # ids listed twice count twice
                check_call(U, V, (3, 1000), (index, item), users, dtype, (k, d2, "users"))
    assert zero_rows                                                       # k = 1: rows of norm 0 were listed


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
def test_real_valued_factors_against_numpy(dtype):
    import primalcr_amd as pcr
    rng = np.random.default_rng(121 + dtype)
    for d1, d2, k in ((300, 3706, 100), (200, 1000, 7), (64, 500, 130), (130, 2000, 256)):
        U, V = pcr.initial(d1, k), pcr.initial(d2, k) * 0.5
        index, item = special_csr(rng, d1, d2)
        check_call(U, V, (1, 10, 100, 1024), (index, item), None, dtype, (d1, d2, k))
        check_call(U, V, (5, 50), None, None, dtype, (d1, d2, k, "no exclusion"))


@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
def test_closed_forms(dtype):
    import primalcr_amd as pcr
    rng = np.random.default_rng(131 + dtype)
    d1, d2, k = 90, 40, 48
    U = rng.standard_normal((d1, k))
    # all rows of V parallel: every cosine is 1, ild = 0
    V = np.outer(rng.uniform(0.5, 3.0, d2), rng.standard_normal(k))
    got, pu = pcr.evaluate_diversity(U, V, cutoffs=(2, 10, 40), dtype=dtype, per_user=True)
    assert np.all(np.abs(pu[..., 2]) <= ILD_ATOL) and all(abs(g["ild"]) <= ILD_ATOL and g["users_ild"] == d1 for g in got)
    # rows of V distinct unit vectors: every cosine is 0, ild = 1 exactly
    V = np.zeros((d2, k)); V[np.arange(d2), rng.permutation(k)[:d2]] = 1.0
    got, pu = pcr.evaluate_diversity(U, V, cutoffs=(2, 10, 40), dtype=dtype, per_user=True)
    assert np.all(pu[..., 2] == 1.0) and all(g["ild"] == 1.0 for g in got)
    # K = d2 without exclusion: every user lists every item
    V = rng.standard_normal((d2, k))
    got, pu, ex = pcr.evaluate_diversity(U, V, cutoffs=(7, d2), dtype=dtype, per_user=True, exposure=True)
    assert np.all(ex[1] == d1) and got[1]["gini"] == 0.0 and got[1]["coverage"] == 1.0 and got[1]["recs"] == d1 * d2
    assert got[1]["items_covered"] == d2 and np.all(pu[:, 1, 0] == d2) and ex[0].sum() == 7 * d1
    # pop = 0 without a CSR: info = log2(d1 + 1) for every item
    assert all(abs(g["novelty"] - np.log2(d1 + 1.0)) <= NOV_RTOL * np.log2(d1 + 1.0) for g in got)
    # users with 0 and 1 eligible items: NaN ild, not counted in users_ild; the empty list has NaN novelty too and is still a user
    rows = [np.arange(d2, dtype=np.int32), np.arange(1, d2, dtype=np.int32)] + [np.array([u % d2], np.int32) for u in range(2, d1)]
    index = np.zeros(d1 + 1, np.int64); index[1:] = np.cumsum([r.shape[0] for r in rows])
    item = np.concatenate(rows)
    got, pu, ex = check_call(U, V, (1, 5, 40), (index, item), None, dtype, "short lists")
    assert np.isnan(pu[0]).sum() == 6 and np.all(pu[0, :, 0] == 0) and np.all(pu[1, :, 0] == 1)
    assert np.isnan(pu[1, :, 2]).all() and not np.isnan(pu[1, :, 1]).any()
    assert [g["users"] for g in got] == [d1] * 3 and [g["users_ild"] for g in got] == [0, d1 - 2, d1 - 2]
    only = np.array([0, 1, 0], np.int32)
    got = pcr.evaluate_diversity(U, V, cutoffs=(5,), exclude=(index, item), users=only, dtype=dtype)
    assert got[0]["users"] == 3 and got[0]["users_ild"] == 0 and got[0]["ild"] == 0.0 and got[0]["recs"] == 1


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
def test_split_counts_determinism_and_invariance(dtype):
    """Split counts 1, 2 and 16; two identical calls bitwise identical; a user's row bitwise the same alone, in a permuted user
    list and as part of the whole set."""
    import primalcr_amd as pcr
    rng = np.random.default_rng(141 + dtype)
    cutoffs = (1, 10, 100, 1024)
    seen = set()
    for d2, k, n in ((2047, 7, 65), (2048, 16, 65), (17770, 9, 40)):
        d1 = 120
        seen.add(splits_of(n, d2, cutoffs[-1], dtype))
        per = rec_geometry(1, d2, cutoffs[-1], dtype)[0].per
        U, V = int_factors(rng, d1, k), int_factors(rng, d2, k)
        index, item = random_csr(rng, d1, d2, {u: boundary_row(u, d2, per) for u in range(0, d1, 5)})
        users = rng.permutation(d1)[:n].astype(np.int32)
        check_call(U, V, cutoffs, (index, item), users, dtype, (d2, "splits"))
    assert seen == {1, 2, 16}
    d1, d2, k = 700, 3706, 40
    U, V = pcr.initial(d1, k), pcr.initial(d2, k) * 0.5
    index, item = special_csr(rng, d1, d2)
    kw = dict(cutoffs=cutoffs, exclude=(index, item), dtype=dtype, per_user=True, exposure=True)
    a, apu, aex = pcr.evaluate_diversity(U, V, **kw)
    b, bpu, bex = pcr.evaluate_diversity(U, V, **kw)
    assert a == b and np.array_equal(bits(apu), bits(bpu)) and np.array_equal(aex, bex)
    perm = rng.permutation(d1).astype(np.int32)
    c, cpu_, cex = pcr.evaluate_diversity(U, V, users=perm, **kw)
    assert np.array_equal(bits(cpu_), bits(apu[perm])) and np.array_equal(cex, aex)
    for f in ("users", "users_ild", "recs", "items_covered", "coverage", "gini"):
        assert [x[f] for x in c] == [x[f] for x in a]
    for u in (0, 3, 5, 699):
        _, one = pcr.evaluate_diversity(U, V, users=np.array([u], np.int32), cutoffs=cutoffs, exclude=(index, item), dtype=dtype, per_user=True)
        assert np.array_equal(bits(one[0]), bits(apu[u])), u


@pytest.mark.gpu
@pytest.mark.timeout(1200)
def test_exposure_accumulates_across_user_batches():
    """Two user batches (D_CASES' shrink-loop shape): exposure and its summaries over all users equal numpy's on recommend()'s
    lists; rows around the batch boundary equal a single-batch call bitwise and numpy."""
    import primalcr_amd as pcr
    n, batches = D_CASES[0]
    rng = np.random.default_rng(n + 1)
    d2, k, dtype, cutoffs = 5120, 8, 1, (1, 10, 100, 1024)
    g = rec_geometry(n, d2, cutoffs[-1], dtype)
    assert [(b.b0, b.users, b.fit, b.splits) for b in g] == batches and len(g) >= 2
    U, V = int_factors(rng, n, k), int_factors(rng, d2, k)
    index, item = random_csr(rng, n, d2)
    ex = (index, item)
    items, _ = pcr.recommend(U, V, cutoffs[-1], exclude=ex, dtype=dtype)
    info = ref_info(n, d2, item)
    _, want_ex, want = ref_diversity(items, V, info, cutoffs, False, want_rows=False)
    got, pu, gex = pcr.evaluate_diversity(U, V, cutoffs=cutoffs, exclude=ex, dtype=dtype, per_user=True, exposure=True)
    assert np.array_equal(gex, want_ex)
    check_summary(got, want, rows=False)
    assert all(x["users_ild"] == n for x in got[1:])
    rows = np.concatenate([np.arange(10), np.arange(g[1].b0 - 10, g[1].b0 + 10), np.arange(n - 10, n)]).astype(np.int32)
    one, opu = pcr.evaluate_diversity(U, V, cutoffs=cutoffs, exclude=ex, users=rows, dtype=dtype, per_user=True)
    assert np.array_equal(bits(opu), bits(pu[rows]))
    want_pu, _, _ = ref_diversity(items[rows], V, info, cutoffs, False)
    check_rows(pu[rows], want_pu)


def _exposure_totals(ex):
    import primalcr_amd as pcr
    return [pcr.exposure_stats(r) for r in ex]


@pytest.mark.gpu
@pytest.mark.timeout(1200)
def test_live_solvers():
    """Solver.evaluate_diversity on PCR++, PCR and CCDR1 against the model entry on get_factors() (bitwise, in the solver's
    storage type), the profile slot, training afterwards, two local-only shards and a 1-rank RCCL communicator."""
    import primalcr_amd as pcr
    from primalcr_amd import synth
    R = synth.generate("small", seed=17)
    ds = pcr.Dataset.from_ratings(R)
    idx, it, val = ds.csr(0)
    tidx, tit, tval = ds.csr(1)
    rng = np.random.default_rng(9)
    r, cutoffs = 16, (1, 10, 100)
    for solver_type in (pcr.PCR_SOLVER_PCRPP, pcr.PCR_SOLVER_PCR, pcr.PCR_SOLVER_CCDR1):
        for prec in (pcr.PCR_F32, pcr.PCR_F64):
            what = (solver_type, prec)
            p = pcr.Parameter(k=r, precision=prec, solver_type=solver_type, **{"lambda": 100.0})
            s, t = pcr.Solver(ds, p), pcr.Solver(ds, p)
            if solver_type == pcr.PCR_SOLVER_CCDR1:
                U0, V0 = pcr.initial_col(R.d1, r), np.zeros((R.d2, r))
            else:
                U0, V0 = pcr.initial(R.d1, r), pcr.initial(R.d2, r)
            s.set_factors(U0, V0); t.set_factors(U0, V0)
            s.iterate(1); t.iterate(1)
            U, V = s.get_factors()
            s.profile(True)
            a, apu, aex = s.evaluate_diversity(cutoffs, per_user=True, exposure=True)
            prof = s.profile_all()
            assert "recommend/diversity" in prof and prof["recommend/diversity"][1] >= 3 and "recommend/score" in prof, prof
            s.profile(False)
            b, bpu, bex = pcr.evaluate_diversity(U, V, cutoffs=cutoffs, exclude=ds, dtype=prec, per_user=True, exposure=True)
            assert a == b and np.array_equal(bits(apu), bits(bpu)) and np.array_equal(aex, bex), what
            assert a[0]["users"] == R.d1
            users = rng.choice(R.d1, 33, replace=False).astype(np.int32)
            c, cpu_ = s.evaluate_diversity(cutoffs, users=users, exclude_train=False, per_user=True)
            d, dpu = pcr.evaluate_diversity(U, V, cutoffs=cutoffs, users=users, dtype=prec, per_user=True)
            assert np.array_equal(bits(cpu_[..., 0]), bits(dpu[..., 0])) and np.array_equal(bits(cpu_[..., 2]), bits(dpu[..., 2])), what
            for f in ("users", "users_ild", "recs", "items_covered", "coverage", "gini", "ild"):
                assert [x[f] for x in c] == [x[f] for x in d], (what, f)
            # (popularity comes from the solver's training ratings also without exclusion; the model entry without a CSR has pop = 0,
            # so novelty is compared exactly only in the call above, where both entries count the same ratings)
            assert all(x["novelty"] < y["novelty"] for x, y in zip(c, d))
            if solver_type == pcr.PCR_SOLVER_PCRPP:
                cut = [0, R.d1 // 3, R.d1]
                rows, expo = [], np.zeros_like(aex)
                for rank in range(2):
                    lo, hi = cut[rank], cut[rank + 1]
                    dsl = pcr.Dataset.from_csr(hi - lo, R.d2, idx[lo:hi + 1] - idx[lo], it[idx[lo]:idx[hi]], val[idx[lo]:idx[hi]].copy(),
                                               tidx[lo:hi + 1] - tidx[lo], tit[tidx[lo]:tidx[hi]], tval[tidx[lo]:tidx[hi]].copy())
                    sh = pcr.Solver(dsl, p, rank=rank, nranks=2, shard=(lo, R.d1))
                    sh.set_local_only(True)
                    sh.set_factors_local(U[lo:hi], V)
                    st, pu, ex = sh.evaluate_diversity(cutoffs, per_user=True, exposure=True)
                    assert st[0]["users"] == hi - lo
                    rows.append(pu); expo += ex
                    with pytest.raises(pcr.PcrError):
                        sh.evaluate_diversity(cutoffs, users=np.array([cut[1] if rank == 0 else 0], np.int32))   # outside the shard
                    sh.close()
                # (a local-only shard's pop comes from its own ratings, by contract: its novelty differs from the one-rank
                # figure and is not compared; len and ild do not depend on pop)
                rows = np.concatenate(rows)
                assert np.array_equal(bits(rows[..., 0]), bits(apu[..., 0])) and np.array_equal(bits(rows[..., 2]), bits(apu[..., 2])), what
                assert np.array_equal(expo, aex)
                for c_, tot in enumerate(_exposure_totals(expo)):
                    for f in ("recs", "items_covered", "coverage", "gini"):
                        assert tot[f] == a[c_][f], (what, f)
                # a 1-rank RCCL communicator: the all-reduces run, the totals are the one-rank result
                w = pcr.Solver(ds, p)
                w.comm_init(pcr.comm_unique_id())
                assert w.comm_nranks() == 1
                w.set_factors(U, V)
                e, epu, eex = w.evaluate_diversity(cutoffs, per_user=True, exposure=True)
                assert e == a and np.array_equal(bits(epu), bits(apu)) and np.array_equal(eex, aex), what
                w.close()
            # training after the calls: bitwise the factors of training without them
            s.iterate(1); t.iterate(1)
            Us, Vs = s.get_factors(); Ut, Vt = t.get_factors()
            assert np.array_equal(Us, Ut) and np.array_equal(Vs, Vt), what
            s.close(); t.close()


P2P_WORKER = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import primalcr_amd as pcr
from primalcr_amd import synth
rank, name = int(sys.argv[2]), sys.argv[3]
R = synth.generate("small", seed=17)
idx, it, val = pcr.Dataset.from_ratings(R).csr(0)
cut = [0, R.d1 // 3, R.d1]
lo, hi = cut[rank], cut[rank + 1]
none = np.zeros(hi - lo + 1, np.int64)
ds = pcr.Dataset.from_csr(hi - lo, R.d2, idx[lo:hi + 1] - idx[lo], it[idx[lo]:idx[hi]], val[idx[lo]:idx[hi]].copy(),
                          none, np.zeros(0, np.int32), np.zeros(0))
s = pcr.Solver(ds, pcr.Parameter(k=8, precision=pcr.PCR_F64, do_predict=0, **{"lambda": 100.0}), rank=rank, nranks=2, shard=(lo, R.d1))
s.comm_init_p2p(name)
assert s.comm_nranks() == 2
s.set_factors_local(pcr.initial_rows(R.d1, 8, lo, hi - lo), pcr.initial(R.d2, 8))
try:
    s.evaluate_diversity((5, 10))
    print("RESULT returned")
except pcr.PcrError as e:
    print("RESULT", str(e))
# the refusal leaves the solver usable: the shard's partials are still to be had
s.set_local_only(True)
st = s.evaluate_diversity((5, 10))
print("LOCAL", st[0]["users"], hi - lo)
s.close()
"""


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_peer_to_peer_communicator_is_refused(tmp_path):
    """Two ranks on the one GPU through the peer-to-peer communicator (RCCL refuses two ranks on one device): its fp64 exchange
    is a 64-double slot that the d2-sized tables do not fit, so pcr_evaluate_diversity answers PCR_ERR_UNSUPPORTED on every rank,
    before anything is exchanged, and names the ways out; the same solvers then give their partials as local-only shards."""
    (tmp_path / "worker.py").write_text(P2P_WORKER)
    name = f"/pcr_div_p2p_{os.getpid()}"
    procs = [subprocess.Popen([sys.executable, str(tmp_path / "worker.py"), ROOT, str(rank), name], stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True, cwd=str(tmp_path)) for rank in range(2)]
    try:
        outs = [p.communicate(timeout=300) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, (out, err) in zip(procs, outs):
        assert p.returncode == 0, err
        res = [l for l in out.splitlines() if l.startswith("RESULT")]
        assert len(res) == 1 and f"libprimalcr error {ERR_UNSUPPORTED}:" in res[0], out
        assert "pcr_evaluate_diversity" in res[0] and "peer-to-peer" in res[0] and "pcr_exposure_stats" in res[0], out
        loc = [l for l in out.splitlines() if l.startswith("LOCAL")][0].split()
        assert loc[1] == loc[2]


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_cli_end_to_end(tmp_path):
    import primalcr_amd as pcr
    from primalcr_amd import synth
    R = synth.generate("small", seed=13)
    d = synth.write_dir(R, str(tmp_path / "data"))
    out = run([TRAIN, "-k", "8", "-t", "2", "-l", "100", d, "m.model"], tmp_path)
    assert out.returncode == 0, out.stderr
    U, V = pcr.model_load(str(tmp_path / "m.model"))
    ds = pcr.Dataset.from_ratings(R)

    def parse(text):
        rows = []
        for line in text.strip().splitlines():
            f = line.split()
            assert f[0].startswith("diversity@")
            rows.append(dict(cutoff=int(f[0][len("diversity@"):]), **{f[i]: float(f[i + 1]) for i in range(1, len(f), 2)}))
        return rows

    def same(got, want):
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert set(g) == set(w)
            for key, v in w.items():
                assert (float(v) if isinstance(v, int) else float(f"{v:g}")) == g[key], (key, g, w)   # counts are printed in full

    r = run([RECOMMEND, "--diversity", "-x", d, "-c", "5,10", "m.model", "per_user.txt"], tmp_path)
    assert r.returncode == 0, r.stderr
    want, pu = pcr.evaluate_diversity(U, V, cutoffs=(5, 10), exclude=ds, per_user=True)
    same(parse(r.stdout), want)
    lines = (tmp_path / "per_user.txt").read_text().strip().splitlines()
    assert len(lines) == R.d1
    for u, line in enumerate(lines):
        f = line.split()
        assert int(f[0]) == u + 1
        assert [float(x) for x in f[1:]] == [float(f"{v:g}") for v in pu[u, -1]]
    (tmp_path / "users").write_text("3\n1\n3\n")
    r = run([RECOMMEND, "--diversity", "-K", "7", "--f32", "-u", "users", "m.model", "three.txt"], tmp_path)
    assert r.returncode == 0, r.stderr
    want, pu = pcr.evaluate_diversity(U, V, cutoffs=(7,), users=np.array([2, 0, 2], np.int32), dtype=pcr.PCR_F32, per_user=True)
    same(parse(r.stdout), want)
    lines = (tmp_path / "three.txt").read_text().strip().splitlines()
    assert [int(l.split()[0]) for l in lines] == [3, 1, 3]
