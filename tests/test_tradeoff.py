"""The theta sweep of the MMR re-ranking (pcr_evaluate_rerank_model / pcr_evaluate_rerank, omp-pmf-recommend --tradeoff, Python
evaluate_rerank() and Solver.evaluate_rerank()): one scoring sweep, then per theta the lists recommend_diverse() returns and
their metrics as evaluate_lists() computes them.

CPU part: the argument checks of both entries (before a device is looked for), the "no device" error, the NULL solver, the
wrappers' ValueErrors, the CLI's new usage lines and refusals.
GPU part (-m gpu): sweep = re-rank, then evaluate, bit for bit per user, under both kernel forms; theta = 0 against evaluate_topn
/ evaluate_diversity; independence of the other thetas; one score launch per user batch whatever nth is; several user batches;
the summaries against the returned per-user rows (integer fields exact; means within 1e-12 relative: a fixed-order fp64 sum
of n <= 4096 non-negative terms errs by at most (n - 1) 2^-53 < 4.6e-13 relative, and so does numpy's); live solvers, shards;
the CLI end to end.
"""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import BIN_DIR, ROOT
from test_recommend_grid import int_factors, random_csr, rec_geometry
from test_rerank import cosines, dyadic_V, lds_form_fits, ref_mmr, stored
from test_topn_eval import make_test_csr

RECOMMEND = os.path.join(BIN_DIR, "omp-pmf-recommend")
ERR_ARG, ERR_DEVICE = -1, -4
THETAS = (0.0, 0.25, 0.5, 0.75, 1.0)
MEAN_RTOL = 1e-12
DTYPES = pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])


def run(cmd, cwd, timeout=600):
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=timeout)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _sweep_call(U, V, index, item, tindex, titem, tval, users, thetas, pool, cutoffs, threshold=-math.inf, dtype=1, n=None, nth=None,
                topn=True, per_user_topn=False, div=True):
    """pcr_evaluate_rerank_model through ctypes, arrays as given (None = NULL); returns the status code."""
    import primalcr_amd as pcr
    from primalcr_amd.api import TopnStats
    n = (len(users) if users is not None else U.shape[0]) if n is None else n
    th = None if thetas is None else np.asarray(thetas, np.float64)
    nth = (0 if th is None else len(th)) if nth is None else nth
    cuts = None if cutoffs is None else np.asarray(cutoffs, np.int32)
    ts, ds = (TopnStats * 128)(), (pcr.DiversityStats * 128)()
    pu = np.empty((16, max(n, 1), 16, 6))
    ptr = lambda a: None if a is None else a.ctypes.data
    return pcr.lib().pcr_evaluate_rerank_model(ptr(U), U.shape[0], ptr(V), V.shape[0], U.shape[1], ptr(index), ptr(item), ptr(tindex), ptr(titem),
                                               ptr(tval), n, ptr(users), nth, ptr(th), pool, 0 if cuts is None else len(cuts), ptr(cuts),
                                               float(threshold), dtype, C.cast(ts, C.c_void_p) if topn else None,
                                               C.cast(ds, C.c_void_p) if div else None, ptr(pu) if per_user_topn else None, None, None, 0)


def _small():
    rng = np.random.default_rng(1)
    U, V = rng.standard_normal((20, 5)), rng.standard_normal((30, 5))
    index = np.array([0] + [2] * 20, np.int64)
    item = np.array([3, 7], np.int32)
    tindex = np.array([0, 3] + [4] * 19, np.int64)
    titem = np.array([9, 1, 9, 4], np.int32)
    tval = np.array([5.0, 3.0, 4.0, 1.0])
    users = np.arange(20, dtype=np.int32)
    return U, V, index, item, tindex, titem, tval, users


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_model_entry_argument_checks():
    import primalcr_amd as pcr
    U, V, index, item, tindex, titem, tval, users = _small()
    ok = (U, V, index, item, tindex, titem, tval, users)

    def bad(*a, **kw):
        assert _sweep_call(*a, **kw) == ERR_ARG
        assert b"pcr_evaluate_rerank_model" in pcr.lib().pcr_last_error(), pcr.lib().pcr_last_error()

    bad(*ok, [0.5], 4, [5])                                            # pool below topk = the last cutoff
    bad(*ok, [0.5], 1025, [5])
    bad(*ok, [0.5], 1025, [5, 1025])
    bad(*ok, [], 10, [5])                                              # nth outside [1, 8]
    bad(*ok, None, 10, [5], nth=1)
    bad(*ok, [0.1] * 9, 10, [5])
    bad(*ok, [0.5, math.nan], 10, [5])
    bad(*ok, [0.5, 1.01], 10, [5])
    bad(*ok, [-0.01], 10, [5])
    for cuts in ([0], [], None, list(range(1, 10)), [5, 3], [3, 3]):
        bad(*ok, [0.5], 10, cuts)
    bad(*ok, [0.5], 10, [5], threshold=math.nan)
    bad(*ok, [0.5], 10, [5], dtype=5)
    bad(*ok, [0.5], 10, [5], div=False)
    bad(*ok, [0.5], 10, [5], topn=False)                               # a test CSR wants its stats
    bad(U, V, index, item, None, None, None, users, [0.5], 10, [5])    # without a test CSR topn must be NULL
    bad(U, V, index, item, None, None, None, users, [0.5], 10, [5], topn=False, per_user_topn=True)
    # every argument error of pcr_recommend_model and of the test CSR
    bad(U, V, index, item, tindex, titem, tval, np.array([0, 20], np.int32), [0.5], 10, [5])
    bad(U, V, index, item, tindex, titem, tval, None, [0.5], 10, [5], n=21)
    bad(*ok, [0.5], 10, [5], n=-1)
    x = index.copy(); x[5] = 1
    bad(U, V, x, item, tindex, titem, tval, users, [0.5], 10, [5])
    bad(U, V, index, np.array([3, 30], np.int32), tindex, titem, tval, users, [0.5], 10, [5])
    bad(U, V, index, None, tindex, titem, tval, users, [0.5], 10, [5])
    bad(U, V, index, item, tindex, None, tval, users, [0.5], 10, [5])
    t = tindex.copy(); t[5] = 1
    bad(U, V, index, item, t, titem, tval, users, [0.5], 10, [5])
    bad(U, V, index, item, tindex, np.array([9, 1, -1, 4], np.int32), tval, users, [0.5], 10, [5])


def test_solver_entry_checks_its_solver_first():
    import primalcr_amd as pcr
    st = (pcr.DiversityStats * 2)()
    cuts, th = np.array([5], np.int32), np.array([0.5])
    assert pcr.lib().pcr_evaluate_rerank(None, 0, None, 1, th.ctypes.data, 10, 1, cuts.ctypes.data, -math.inf, 0, None, C.cast(st, C.c_void_p),
                                         None, None, None) == ERR_ARG
    assert b"null solver" in pcr.lib().pcr_last_error()


def test_model_entry_without_a_device_is_a_device_error():
    code = ("import sys, numpy as np; sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')\n"
            "from test_tradeoff import _sweep_call, _small\n"
            "U, V, index, item, tindex, titem, tval, users = _small()\n"
            "print(_sweep_call(U, V, index, item, tindex, titem, tval, users, [0.0, 0.5], 10, [1, 5]),\n"
            "      _sweep_call(U, V, None, None, None, None, None, None, [1.0], 5, [5], dtype=0, topn=False))\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    assert [int(x) for x in out.stdout.strip().splitlines()[-1].split()] == [ERR_DEVICE, ERR_DEVICE]


def test_python_wrappers_refuse_bad_arguments():
    import primalcr_amd as pcr
    U, V, index, item, tindex, titem, tval, users = _small()
    for thetas, kw in (((0.5,), dict(pool=4, cutoffs=(5,))), ((0.5,), dict(pool=1025)), ((), dict()), ((0.1,) * 9, dict()), ((0.5, 1.5), dict()),
                       ((-0.1,), dict()), ((math.nan,), dict()), ((0.5,), dict(cutoffs=(0,))), ((0.5,), dict(cutoffs=(5, 5))),
                       ((0.5,), dict(cutoffs=(5, 2000))), ((0.5,), dict(cutoffs=tuple(range(1, 10)))), ((0.5,), dict(threshold=math.nan))):
        with pytest.raises(ValueError):
            pcr.evaluate_rerank(U, V, thetas, **kw)
        with pytest.raises(ValueError):
            pcr.Solver.evaluate_rerank(None, thetas, **kw)                 # (checked before the solver is touched)
    with pytest.raises(ValueError):
        pcr.evaluate_rerank(U, V, (0.5,), test=(tindex, titem[:3], tval[:3]))
    with pytest.raises(ValueError):
        pcr.evaluate_rerank(U, V, (0.5,), exclude=(index[:4], item))
    from primalcr_amd.api import _tradeoff_args
    th, pool, cuts = _tradeoff_args((0, 1), None, (5, 10), -math.inf)
    assert pool == 100 and list(cuts) == [5, 10] and list(th) == [0.0, 1.0]                # pool None is _rerank_args' default
    assert _tradeoff_args(0.5, None, 200, 0.0)[1] == 1024
    assert pcr.evaluate_rerank is pcr.api.evaluate_rerank and "evaluate_rerank" in pcr.__all__


def test_cli_usage_and_refusals(tmp_path):
    import primalcr_amd as pcr
    from primalcr_amd import synth
    r = run([RECOMMEND], tmp_path)
    assert r.returncode == 1 and r.stdout.startswith("Usage: omp-pmf-recommend [-K topk]")
    assert "omp-pmf-recommend --tradeoff t1,t2,... [--pool P] [-K topk] [-c c1,...] [--eval data_dir [--threshold v]]" in r.stdout
    assert "    --tradeoff ts  " in r.stdout
    # the usage text only grows at its end: everything up to the last line of the parent's text comes first
    head = r.stdout.split("       omp-pmf-recommend --tradeoff")[0]
    assert head.rstrip().endswith("with --ranks: per counted user first_rank rr mean_rank auc mpr") and "--mmr theta" in head
    R = synth.generate("tiny", seed=3)
    d = synth.write_dir(R, str(tmp_path / "data"))
    missing = str(tmp_path / "missing.model")
    # refused before the model is read
    for extra in (["--mmr", "0.5"], ["--diversity"], ["--ranks"], ["--scores"]):
        r = run([RECOMMEND, "--tradeoff", "0,0.5"] + extra + [missing], tmp_path)
        assert r.returncode == 1 and "--tradeoff" in r.stderr and "can't open" not in r.stderr, extra
    r = run([RECOMMEND, "--tradeoff", "0,0.5", missing, "out.txt"], tmp_path)               # an output file
    assert r.returncode == 1 and "--tradeoff" in r.stderr and "can't open" not in r.stderr
    for v in ("1.5", "0,-0.1", "nan", "x", "", "0.5,", ",".join(["0.1"] * 9)):
        r = run([RECOMMEND, "--tradeoff", v, missing], tmp_path)
        assert r.returncode == 1 and "--tradeoff" in r.stderr and "can't open" not in r.stderr, v
    r = run([RECOMMEND, "--tradeoff"], tmp_path)
    assert r.returncode == 1 and "--tradeoff needs a value" in r.stderr and r.stdout.startswith("Usage: omp-pmf-recommend")
    r = run([RECOMMEND, "--tradeoff", "0.5", "--pool", "5", "-K", "10", missing], tmp_path)
    assert r.returncode == 1 and "--pool" in r.stderr and "can't open" not in r.stderr
    r = run([RECOMMEND, "--tradeoff", "0.5", "--threshold", "4", missing], tmp_path)        # --threshold needs --eval
    assert r.returncode == 1 and "--threshold" in r.stderr and "can't open" not in r.stderr
    r = run([RECOMMEND, "--tradeoff", "0.5"], tmp_path)                                      # no model
    assert r.returncode == 1 and r.stdout.startswith("Usage: omp-pmf-recommend")
    r = run([RECOMMEND, "--tradeoff", "0.5", "--eval", d, "-x", d, "-c", "5,10", "--pool", "20", missing], tmp_path)   # a full, valid line
    assert r.returncode == 1 and "can't open model file" in r.stderr
    # what the CLI refused before stays refused, word for word
    r = run([RECOMMEND, "--mmr", "0.5", "--eval", d, missing], tmp_path)
    assert r.returncode == 1 and r.stderr == "--mmr does not go with --eval or --diversity\n"
    r = run([RECOMMEND, "--mmr", "0.5", "--diversity", missing], tmp_path)
    assert r.returncode == 1 and r.stderr == "--mmr does not go with --eval or --diversity\n"
    r = run([RECOMMEND, "--pool", "50", missing, "out.txt"], tmp_path)
    assert r.returncode == 1 and r.stderr == "--pool goes with --mmr\n"
    r = run([RECOMMEND, "-c", "5", missing, "out.txt"], tmp_path)
    assert r.returncode == 1 and r.stderr == "-c and --threshold go with --eval\n"
    r = run([RECOMMEND, "--eval", d, "-u", "users", missing], tmp_path)
    assert r.returncode == 1 and r.stderr == "-u and --scores do not go with --eval\n"
    assert pcr.PCR_RERANK_MAX_THETAS == 8


# ---------------------------------------------------------------------------------------------------------------- GPU helpers
def same_result(a, b, what=None, keys=("per_user_topn", "per_user_diversity")):
    """Two result dicts of evaluate_lists() / evaluate_rerank(): per-user rows bit for bit, exposure and summaries equal."""
    for key in keys:
        assert (key in a) == (key in b), (what, key)
        if key in a:
            assert np.array_equal(bits(a[key]), bits(b[key])), (what, key)
    assert ("exposure" in a) == ("exposure" in b), what
    if "exposure" in a:
        assert np.array_equal(a["exposure"], b["exposure"]), what
    assert a["diversity"] == b["diversity"] and a.get("topn") == b.get("topn"), what


def check_summaries(res, what=None):
    """The summaries of one result against its own per-user rows and exposure."""
    import primalcr_amd as pcr

    def close(got, rows, count):
        want = float(np.sum(rows)) / count if count else 0.0
        assert abs(got - want) <= MEAN_RTOL * abs(want), (what, got, want)

    pud, ex = res["per_user_diversity"], res["exposure"]
    n = pud.shape[0]
    assert n <= 4096
    for c, s in enumerate(res["diversity"]):
        ln, nov, ild = pud[:, c, 0], pud[:, c, 1], pud[:, c, 2]
        tot = pcr.exposure_stats(ex[c])
        assert s["users"] == n and s["users_ild"] == int((~np.isnan(ild)).sum()) and s["recs"] == int(ln.sum()) == int(ex[c].sum()), what
        for f in ("recs", "items_covered", "coverage", "gini"):
            assert s[f] == tot[f], (what, f)
        close(s["novelty"], nov[ln > 0], int((ln > 0).sum()))
        close(s["ild"], ild[~np.isnan(ild)], s["users_ild"])
    if "topn" not in res:
        return
    put = res["per_user_topn"]
    counted = ~np.isnan(put[:, 0, 0])
    for c, s in enumerate(res["topn"]):
        P = put[counted, c]
        graded = ~np.isnan(P[:, 5])
        assert s["users"] == int(counted.sum()) and s["users_graded"] == int(graded.sum()) and s["hits"] == int(P[:, 0].sum()), what
        for f, col in (("precision", 1), ("recall", 2), ("map", 3), ("ndcg", 4)):
            close(s[f], P[:, col], s["users"])
        close(s["hit_rate"], (P[:, 0] > 0).astype(np.float64), s["users"])
        close(s["ndcg_graded"], P[graded, 5], s["users_graded"])


def _exact_inputs(seed, d1, d2, k):
    """int_factors / dyadic_V (test_rerank's _exact_case), an exclusion CSR in which user 3 keeps 4 eligible items and user 4 none,
    and a test CSR with empty rows and duplicated items."""
    rng = np.random.default_rng(seed)
    U, V = int_factors(rng, d1, k), dyadic_V(rng, d2, k)
    special = {3: np.setdiff1d(np.arange(d2), [0, 7, d2 // 2, d2 - 1]).astype(np.int32), 4: np.arange(d2, dtype=np.int32)}
    index, item = random_csr(rng, d1, d2, special)
    return U, V, index, item, make_test_csr(rng, d1, d2, index, item)


def per_list_route(U, V, ex, test, users, topk, pool, theta, cutoffs, thr, dtype):
    """recommend_diverse(), then evaluate_lists() on what it returned: (result, items)."""
    import primalcr_amd as pcr
    d1 = U.shape[0]
    items, _ = pcr.recommend_diverse(U, V, topk, pool=pool, theta=theta, exclude=ex, users=users, dtype=dtype)
    res = pcr.evaluate_lists(items, V, d1=d1, users=np.arange(d1, dtype=np.int32) if users is None else users, test=test, popularity=ex,
                             cutoffs=cutoffs, threshold=thr, dtype=dtype, per_user=True, exposure=True)
    return res, items


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.timeout(600)
@DTYPES
@pytest.mark.parametrize("d2,k", [(300, 7), (300, 100), (2100, 7), (2100, 100)])
def test_sweep_is_rerank_then_evaluate_bitwise(dtype, d2, k):
    import primalcr_amd as pcr
    d1 = 40
    U, V, index, item, test = _exact_inputs(7 + d2 + k, d1, d2, k)
    ex = (index, item)
    assert len(rec_geometry(d1, d2, 64, dtype)) == 1 and rec_geometry(d1, d2, 64, dtype)[0].splits == (2 if d2 == 2100 else 1)
    G = cosines(stored(V, dtype))
    eight = THETAS + (0.5, 0.0, 1.0)                                        # nth = 8: equal thetas are allowed
    for (topk, pool), thr in zip(((1, 1), (10, 64), (10, 65), (64, 64), (5, 300)), (-math.inf, 4.0, -math.inf, 4.0, -math.inf)):
        cutoffs = tuple(c for c in (1, 5, 10) if c < topk) + (topk,)
        what = (d2, k, topk, pool)
        kw = dict(pool=pool, cutoffs=cutoffs, test=test, exclude=ex, threshold=thr, dtype=dtype, per_user=True, exposure=True)
        with pcr.tuned(rerank_lds=0):
            sweep = pcr.evaluate_rerank(U, V, eight, **kw)
        assert [r["theta"] for r in sweep] == list(eight)
        if lds_form_fits(pool, k, dtype):
            with pcr.tuned(rerank_lds=1):
                for a, b in zip(pcr.evaluate_rerank(U, V, eight, **kw), sweep):
                    same_result(a, b, (what, "lds form"))
        pi, ps = pcr.recommend(U, V, pool, exclude=ex, dtype=dtype)
        if pool == 300 and d2 == 300:
            assert ((pi >= 0).sum(1) < pool).any() and (pi[3] >= 0).sum() == 4 and (pi[4] == -1).all()     # short pools
        for t, theta in enumerate(THETAS):
            want, items = per_list_route(U, V, ex, test, None, topk, pool, theta, cutoffs, thr, dtype)
            same_result(sweep[t], want, (what, theta))
            assert np.array_equal(items, ref_mmr(pi, ps, None, topk, theta, G=G)[0]), (what, theta)
            check_summaries(sweep[t], (what, theta))
        for t, src in ((5, 2), (6, 0), (7, 4)):                             # the repeated thetas repeat their results
            same_result(sweep[t], sweep[src], (what, "equal thetas", t))
        # theta = 0: the rows of evaluate_topn / evaluate_diversity
        ts, tpu = pcr.evaluate_topn(U, V, test, cutoffs=cutoffs, exclude=ex, threshold=thr, dtype=dtype, per_user=True)
        dv, dpu, dex = pcr.evaluate_diversity(U, V, cutoffs=cutoffs, exclude=ex, dtype=dtype, per_user=True, exposure=True)
        assert np.array_equal(bits(sweep[0]["per_user_topn"]), bits(tpu)) and np.array_equal(bits(sweep[0]["per_user_diversity"]), bits(dpu)), what
        assert np.array_equal(sweep[0]["exposure"], dex), what
        # nth = 1: one result does not depend on which other thetas are in the call
        for t in (1, 4):
            same_result(pcr.evaluate_rerank(U, V, (THETAS[t],), **kw)[0], sweep[t], (what, "alone", t))
    assert any((sweep[2]["per_user_diversity"] != sweep[0]["per_user_diversity"])[~np.isnan(sweep[0]["per_user_diversity"])].ravel())
    # a user list with a repeated id, no test CSR, no exclusion
    users = np.array([39, 3, 0, 3, 17], np.int32)
    part = pcr.evaluate_rerank(U, V, (0.5,), pool=64, cutoffs=(5, 10), users=users, dtype=dtype, per_user=True, exposure=True)[0]
    assert "topn" not in part and part["diversity"][0]["users"] == 5
    items, _ = pcr.recommend_diverse(U, V, 10, pool=64, theta=0.5, users=users, dtype=dtype)
    want = pcr.evaluate_lists(items, V, d1=d1, users=users, cutoffs=(5, 10), dtype=dtype, per_user=True, exposure=True)
    same_result(part, want, "users")
    assert np.array_equal(bits(part["per_user_diversity"][1]), bits(part["per_user_diversity"][3]))


def _train_data(seed=17):
    import primalcr_amd as pcr
    from primalcr_amd import synth
    R = synth.generate("small", seed=seed)
    return R, pcr.Dataset.from_ratings(R)


def _solver(ds, R, solver_type, prec, r=16):
    import primalcr_amd as pcr
    p = pcr.Parameter(k=r, precision=prec, solver_type=solver_type, **{"lambda": 100.0})
    s = pcr.Solver(ds, p)
    if solver_type == pcr.PCR_SOLVER_CCDR1:
        s.set_factors(pcr.initial_col(R.d1, r), np.zeros((R.d2, r)))
    else:
        s.set_factors(pcr.initial(R.d1, r), pcr.initial(R.d2, r))
    return s, p


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_one_score_pass_whatever_nth_is():
    import primalcr_amd as pcr
    R, ds = _train_data()
    s, _ = _solver(ds, R, pcr.PCR_SOLVER_PCRPP, pcr.PCR_F64)
    s.iterate(1)
    pool = 64
    batches = len(rec_geometry(s.n_users, s.d2, pool, 1))
    assert batches >= 1
    s.profile(True)
    for thetas in ((0.0, 0.3, 0.6, 1.0), (0.5,)):
        s.profile_reset()
        s.evaluate_rerank(thetas, pool=pool, cutoffs=(5, 10))
        assert s.profile_launches("recommend/score") == batches, thetas
        assert s.profile_launches("recommend/rerank") == len(thetas) * batches, thetas
        assert s.profile_launches("recommend/listmetrics") >= len(thetas) * batches + 1, thetas
        prof = s.profile_all()
        assert prof["recommend/listmetrics"][0] > 0.0 and "recommend/merge" not in prof and "recommend/diversity" not in prof, prof
    s.close()


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_more_than_one_user_batch():
    """test_recommend_grid's D_CASES shape: 44 000 requests at pool 1024 are two user batches; sweep and per-list route agree."""
    import primalcr_amd as pcr
    n, d1, d2, k, pool, topk, dtype = 44000, 500, 1100, 4, 1024, 2, 1
    g = rec_geometry(n, d2, pool, dtype)
    assert len(g) >= 2
    U, V, index, item, test = _exact_inputs(51, d1, d2, k)
    ex = (index, item)
    rng = np.random.default_rng(52)
    users = rng.integers(0, d1, n).astype(np.int32)
    sweep = pcr.evaluate_rerank(U, V, (0.5, 1.0), pool=pool, cutoffs=(1, topk), test=test, exclude=ex, users=users, threshold=4.0, dtype=dtype,
                                per_user=True, exposure=True)
    for t, theta in enumerate((0.5, 1.0)):
        want, _ = per_list_route(U, V, ex, test, users, topk, pool, theta, (1, topk), 4.0, dtype)
        same_result(sweep[t], want, theta)
        assert sweep[t]["diversity"][0]["users"] == n and 0 < sweep[t]["topn"][0]["users"] < n
    # every repeated id has the same row, whichever batch it sits in
    first = np.full(d1, -1, np.int64)
    first[users[::-1]] = np.arange(n - 1, -1, -1)
    for key in ("per_user_topn", "per_user_diversity"):
        assert np.array_equal(bits(sweep[0][key]), bits(sweep[0][key][first[users]])), key


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("solver", ["pcrpp", "ccdr1"])
def test_solver_entry(solver):
    """Solver.evaluate_rerank equals evaluate_rerank on get_factors() in the solver's storage type, bitwise per user; two calls
    are bitwise identical; training afterwards is that of a run without the calls; two local-only shards' partials add up."""
    import primalcr_amd as pcr
    R, ds = _train_data()
    idx, it, val = ds.csr(0)
    tidx, tit, tval = ds.csr(1)
    solver_type = pcr.PCR_SOLVER_PCRPP if solver == "pcrpp" else pcr.PCR_SOLVER_CCDR1
    thetas, cutoffs, pool = (0.0, 0.5, 1.0), (5, 10), 64
    rng = np.random.default_rng(9)
    for prec in (pcr.PCR_F32, pcr.PCR_F64):
        what = (solver, prec)
        (s, p), (t, _) = _solver(ds, R, solver_type, prec), _solver(ds, R, solver_type, prec)
        s.iterate(1); t.iterate(1)
        U, V = s.get_factors()
        a = s.evaluate_rerank(thetas, pool=pool, cutoffs=cutoffs, threshold=4.0, per_user=True, exposure=True)
        b = pcr.evaluate_rerank(U, V, thetas, pool=pool, cutoffs=cutoffs, test=ds, exclude=ds, threshold=4.0, dtype=prec, per_user=True, exposure=True)
        again = s.evaluate_rerank(thetas, pool=pool, cutoffs=cutoffs, threshold=4.0, per_user=True, exposure=True)
        for x, y, z in zip(a, b, again):
            same_result(x, y, what)
            same_result(x, z, (what, "again"))
            check_summaries(x, what)
        assert a[0]["diversity"][0]["users"] == R.d1 and 0 < a[0]["topn"][0]["users"] <= R.d1
        assert any(x["diversity"][-1]["ild"] != a[0]["diversity"][-1]["ild"] for x in a[1:])      # the re-ranking changes the lists
        users = rng.choice(R.d1, 33, replace=False).astype(np.int32)
        c = s.evaluate_rerank((0.7,), cutoffs=(3,), users=users, exclude_train=False, per_user=True)[0]
        d = pcr.evaluate_rerank(U, V, (0.7,), cutoffs=(3,), test=ds, users=users, dtype=prec, per_user=True)[0]
        # (popularity comes from the solver's training ratings also without exclusion: novelty is compared in the call above)
        assert np.array_equal(bits(c["per_user_topn"]), bits(d["per_user_topn"])) and c["topn"] == d["topn"], what
        assert np.array_equal(bits(c["per_user_diversity"][..., [0, 2]]), bits(d["per_user_diversity"][..., [0, 2]])), what
        if solver == "pcrpp":
            cut = [0, R.d1 // 3, R.d1]
            parts = []
            for rank in range(2):
                lo, hi = cut[rank], cut[rank + 1]
                dsl = pcr.Dataset.from_csr(hi - lo, R.d2, idx[lo:hi + 1] - idx[lo], it[idx[lo]:idx[hi]], val[idx[lo]:idx[hi]].copy(),
                                           tidx[lo:hi + 1] - tidx[lo], tit[tidx[lo]:tidx[hi]], tval[tidx[lo]:tidx[hi]].copy())
                sh = pcr.Solver(dsl, p, rank=rank, nranks=2, shard=(lo, R.d1))
                sh.set_local_only(True)
                sh.set_factors_local(U[lo:hi], V)
                parts.append(sh.evaluate_rerank(thetas, pool=pool, cutoffs=cutoffs, threshold=4.0, per_user=True, exposure=True))
                with pytest.raises(pcr.PcrError, match="pcr_evaluate_rerank"):
                    sh.evaluate_rerank(thetas, users=np.array([cut[1] if rank == 0 else 0], np.int32))   # outside the shard
                sh.close()
            for g, whole in enumerate(a):
                x, y = parts[0][g], parts[1][g]
                # (a local-only shard's pop comes from its own ratings: its novelty is not compared; the rest does not depend on pop)
                assert np.array_equal(bits(np.concatenate([x["per_user_topn"], y["per_user_topn"]])), bits(whole["per_user_topn"])), what
                for col in (0, 2):
                    both = np.concatenate([x["per_user_diversity"][..., col], y["per_user_diversity"][..., col]])
                    assert np.array_equal(bits(both), bits(whole["per_user_diversity"][..., col])), what
                expo = x["exposure"] + y["exposure"]
                assert np.array_equal(expo, whole["exposure"]), what
                for c_ in range(len(cutoffs)):
                    tot = pcr.exposure_stats(expo[c_])
                    for f in ("recs", "items_covered"):
                        assert tot[f] == whole["diversity"][c_][f], (what, f)
                    for f in ("users", "users_ild"):
                        assert x["diversity"][c_][f] + y["diversity"][c_][f] == whole["diversity"][c_][f], (what, f)
                    for f in ("users", "users_graded", "hits"):
                        assert x["topn"][c_][f] + y["topn"][c_][f] == whole["topn"][c_][f], (what, f)
        s.iterate(1); t.iterate(1)
        Us, Vs = s.get_factors(); Ut, Vt = t.get_factors()
        assert np.array_equal(Us, Ut) and np.array_equal(Vs, Vt), what
        s.close(); t.close()


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_cli_end_to_end(tmp_path):
    import primalcr_amd as pcr
    from primalcr_amd import synth
    R = synth.generate("tiny", seed=13)
    d = synth.write_dir(R, str(tmp_path / "data"))
    rng = np.random.default_rng(14)
    pcr.model_save(str(tmp_path / "m.model"), rng.standard_normal((R.d1, 6)), rng.standard_normal((R.d2, 6)))
    U, V = pcr.model_load(str(tmp_path / "m.model"))
    ds = pcr.Dataset.from_ratings(R)

    def parse(text, prefix):
        rows = []
        for line in text.strip().splitlines():
            f = line.split()
            assert f[0] == "theta"
            if f[2].startswith(prefix):
                name = [("cutoff", int(f[3]))] if prefix == "cutoff" else [("cutoff", int(f[2][len(prefix):]))]
                rest = f[4:] if prefix == "cutoff" else f[3:]
                rows.append(dict([("theta", float(f[1]))] + name, **{rest[i]: float(rest[i + 1]) for i in range(0, len(rest), 2)}))
        return rows

    def same(got, want, theta):
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g.pop("theta") == theta and set(g) == set(w)
            for key, v in w.items():
                assert (float(v) if isinstance(v, int) else float(f"{v:g}")) == g[key], (key, g, w)   # counts are printed in full

    r = run([RECOMMEND, "--tradeoff", "0,0.5", "--eval", d, "-x", d, "-c", "5,10", "m.model"], tmp_path)
    assert r.returncode == 0, r.stderr
    want = pcr.evaluate_rerank(U, V, (0.0, 0.5), cutoffs=(5, 10), test=ds, exclude=ds)
    assert len(r.stdout.strip().splitlines()) == 2 * 2 * 2
    for t, theta in enumerate((0.0, 0.5)):
        same([x for x in parse(r.stdout, "cutoff") if x["theta"] == theta], want[t]["topn"], theta)
        same([x for x in parse(r.stdout, "diversity@") if x["theta"] == theta], want[t]["diversity"], theta)
    (tmp_path / "users").write_text("3\n1\n3\n")
    r = run([RECOMMEND, "--tradeoff", "1", "--pool", "20", "-K", "7", "--f32", "-u", "users", "m.model"], tmp_path)
    assert r.returncode == 0, r.stderr
    want = pcr.evaluate_rerank(U, V, (1.0,), pool=20, cutoffs=(7,), users=np.array([2, 0, 2], np.int32), dtype=pcr.PCR_F32)
    assert parse(r.stdout, "cutoff") == []
    same(parse(r.stdout, "diversity@"), want[0]["diversity"], 1.0)
