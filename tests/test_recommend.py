"""Top-K recommendation of unrated items (pcr_recommend_model / pcr_recommend, omp-pmf-recommend, Python recommend()).

CPU part: argument checks of the C ABI, the CLI's usage text and its argument errors.
GPU part (-m gpu): exact rankings on integer factors (every score exact in f32 and fp64, ties everywhere) against a numpy
lexsort, real-valued factors against host fp64 scores, the solver entry against the model entry, invariance and determinism,
per-shard serving, the Netflix shape and the CLI end to end.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import BIN_DIR, ROOT

RECOMMEND = os.path.join(BIN_DIR, "omp-pmf-recommend")
TRAIN = os.path.join(BIN_DIR, "omp-pmf-train")
ERR_ARG, ERR_DEVICE = -1, -4


def run(cmd, cwd, timeout=600):
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=timeout)


def _model_call(U, V, index, item, users, K, dtype=1, n=None):
    """pcr_recommend_model through ctypes, arrays as given (None = NULL); returns the status code."""
    import primalcr_amd as pcr
    n = (len(users) if users is not None else U.shape[0]) if n is None else n
    items = np.empty(max(n, 1) * max(K, 1), np.int32); scores = np.empty(max(n, 1) * max(K, 1), np.float64)
    ptr = lambda a: None if a is None else a.ctypes.data
    return pcr.lib().pcr_recommend_model(ptr(U), U.shape[0], ptr(V), V.shape[0], U.shape[1], ptr(index), ptr(item), n, ptr(users),
                                         K, dtype, items.ctypes.data, scores.ctypes.data, 0)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_model_entry_argument_checks():
    rng = np.random.default_rng(1)
    U, V = rng.standard_normal((20, 5)), rng.standard_normal((30, 5))
    index = np.array([0] + [2] * 20, np.int64)
    item = np.array([3, 7], np.int32)
    users = np.arange(20, dtype=np.int32)
    assert _model_call(U, V, index, item, users, 0) == ERR_ARG
    assert _model_call(U, V, index, item, users, 1025) == ERR_ARG
    assert _model_call(U, V, index, item, np.array([0, 20], np.int32), 10) == ERR_ARG
    assert _model_call(U, V, index, item, np.array([-1], np.int32), 10) == ERR_ARG
    bad = index.copy(); bad[5] = 1                                                   # not monotone
    assert _model_call(U, V, bad, item, users, 10) == ERR_ARG
    assert _model_call(U, V, np.array([0] + [2] * 19 + [1], np.int64), item, users, 10) == ERR_ARG   # last entry below its predecessor
    assert _model_call(U, V, index, np.array([3, 30], np.int32), users, 10) == ERR_ARG   # item outside the model
    assert _model_call(U, V, index, None, users, 10) == ERR_ARG                      # index without item
    assert _model_call(U, V, index, item, None, 10, n=21) == ERR_ARG                 # more users than the model without a list
    assert _model_call(U, V, index, item, users, 10, dtype=5) == ERR_ARG
    import primalcr_amd as pcr
    with pytest.raises(pcr.PcrError):
        pcr.recommend(U, V, 0)
    with pytest.raises(ValueError):                                                  # last index entry != length of item
        pcr.recommend(U, V, 5, exclude=(index, np.array([3, 7, 9], np.int32)))


def test_model_entry_without_a_device_is_a_device_error():
    """Valid arguments on a process that sees no GPU: PCR_ERR_DEVICE (never a CPU path)."""
    code = ("import sys, numpy as np; sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')\n"
            "from test_recommend import _model_call\n"
            "U = np.ones((4, 3)); V = np.ones((6, 3))\n"
            "print(_model_call(U, V, np.array([0, 1, 1, 1, 1], np.int64), np.array([2], np.int32), np.arange(4, dtype=np.int32), 3))\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    assert int(out.stdout.strip().splitlines()[-1]) == ERR_DEVICE


def test_cli_usage(tmp_path):
    r = run([RECOMMEND], tmp_path)
    assert r.returncode == 1 and r.stdout.startswith("Usage: omp-pmf-recommend [-K topk] [-x data_dir] [-u users_file] [--f32] [--scores]")
    r = run([RECOMMEND, "only_one_arg"], tmp_path)
    assert r.returncode == 1 and r.stdout.startswith("Usage: omp-pmf-recommend")
    for bad in ("0", "1025", "abc"):
        r = run([RECOMMEND, "-K", bad, "m", "o"], tmp_path)
        assert r.returncode == 1 and "-K" in r.stderr
    r = run([RECOMMEND, "--bogus", "m", "o"], tmp_path)
    assert r.returncode == 1 and "unknown option" in r.stderr
    r = run([RECOMMEND, str(tmp_path / "missing.model"), "o"], tmp_path)
    assert r.returncode == 1 and "can't open model file" in r.stderr


def test_cli_argument_errors(tmp_path):
    import primalcr_amd as pcr
    from primalcr_amd import synth
    R = synth.generate("tiny", seed=3)                      # 60 x 40
    d = synth.write_dir(R, str(tmp_path / "data"))
    rng = np.random.default_rng(2)
    pcr.model_save(str(tmp_path / "wrong.model"), rng.standard_normal((R.d1 + 1, 4)), rng.standard_normal((R.d2, 4)))
    r = run([RECOMMEND, "-x", d, "wrong.model", "out"], tmp_path)
    assert r.returncode == 1 and "data set" in r.stderr and "the model" in r.stderr
    pcr.model_save(str(tmp_path / "ok.model"), rng.standard_normal((R.d1, 4)), rng.standard_normal((R.d2, 4)))
    for content, what in (("1\n2\nx\n", "not a user id"), ("1\n0\n", "outside"), (f"{R.d1 + 1}\n", "outside")):
        (tmp_path / "users").write_text(content)
        r = run([RECOMMEND, "-u", "users", "ok.model", "out"], tmp_path)
        assert r.returncode == 1 and what in r.stderr, (content, r.stderr)
    r = run([RECOMMEND, "-u", "missing_users", "ok.model", "out"], tmp_path)
    assert r.returncode == 1 and "can't open users file" in r.stderr


# ---------------------------------------------------------------------------------------------------------------- GPU helpers
def ref_topk(S, excl, K):
    """(items, scores) of the order rule: descending score, equal scores by ascending item id; padding (-1, -inf)."""
    n = S.shape[0]
    items = np.full((n, K), -1, np.int32); scores = np.full((n, K), -np.inf)
    for i in range(n):
        elig = np.nonzero(~excl[i])[0]
        s = S[i, elig]
        o = np.lexsort((elig, -s))[:K]
        items[i, :o.shape[0]] = elig[o]; scores[i, :o.shape[0]] = s[o]
    return items, scores


def excl_mask(d1, d2, index, item):
    M = np.zeros((d1, d2), bool)
    for u in range(d1):
        M[u, item[index[u]:index[u + 1]]] = True
    return M


def special_csr(rng, d1, d2):
    """Training CSR with users without ratings, a user who rated all but 3 items, duplicate pairs; rows item-ascending."""
    rows = []
    for u in range(d1):
        if u % 7 == 3:
            rows.append(np.zeros(0, np.int32))
        elif u == 5 and d2 > 3:
            rows.append(np.sort(rng.choice(d2, d2 - 3, replace=False)).astype(np.int32))
        else:
            r = rng.choice(d2, min(d2, int(rng.integers(1, 12))), replace=False)
            if u % 5 == 1:
                r = np.concatenate([r, r[:2]])                 # duplicated (user, item) pairs
            rows.append(np.sort(r).astype(np.int32))
    index = np.zeros(d1 + 1, np.int64)
    index[1:] = np.cumsum([r.shape[0] for r in rows])
    return index, np.concatenate(rows).astype(np.int32)


def check_real(U, V, excl, items, scores, K, f32):
    """Real-valued factors: scores within tolerance of host fp64 scores, lists non-increasing, nothing excluded returned, and no
    eligible item left out that scores above the K-th returned score by more than twice the tolerance."""
    S = U @ V.T
    A = np.abs(U) @ np.abs(V).T
    tol = (2e-6 if f32 else 1e-12) * A
    for i in range(U.shape[0]):
        got = items[i][items[i] >= 0]
        n_elig = int((~excl[i]).sum())
        assert got.shape[0] == min(K, n_elig)
        assert np.all(items[i][got.shape[0]:] == -1) and np.all(np.isneginf(scores[i][got.shape[0]:]))
        assert np.unique(got).shape[0] == got.shape[0]
        assert not excl[i, got].any()
        s = scores[i, :got.shape[0]]
        assert np.all(np.abs(s - S[i, got]) <= tol[i, got])
        assert np.all(np.diff(s) <= 0)
        if got.shape[0] == K:
            rest = ~excl[i].copy(); rest[got] = False
            kth = s[-1]
            assert not np.any(S[i, rest] > kth + 2 * tol[i, rest] + 2 * tol[i, got[-1]])


def lex_equal(items, scores, ri, rs):
    assert np.array_equal(items, ri)
    assert np.array_equal(scores, rs)


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
def test_exact_ranking_on_integer_factors(dtype):
    import primalcr_amd as pcr
    rng = np.random.default_rng(11 + dtype)
    d1 = 150
    for k in (1, 7, 64, 100, 130):
        for d2 in (1, 63, 64, 65, 1000, 3706):
            U = rng.integers(-2, 3, (d1, k)).astype(np.float64)
            V = rng.integers(-2, 3, (d2, k)).astype(np.float64)
            S = U @ V.T                                        # exact: |s| <= 4 k
            index, item = special_csr(rng, d1, d2)
            M = excl_mask(d1, d2, index, item)
            none = np.zeros_like(M)
            for K in (1, 10, 100, 1024):
                gi, gs = pcr.recommend(U, V, K, exclude=(index, item), dtype=dtype)
                ri, rs = ref_topk(S, M, K)
                assert np.array_equal(gi, ri), (k, d2, K)
                assert np.array_equal(gs, rs), (k, d2, K)
                if K == 10:
                    gi, gs = pcr.recommend(U, V, K, dtype=dtype)
                    ri, rs = ref_topk(S, none, K)
                    assert np.array_equal(gi, ri) and np.array_equal(gs, rs), (k, d2, K, "no exclusion")
    # a CSR whose rows are not item-ascending excludes the same items
    U = rng.integers(-2, 3, (d1, 9)).astype(np.float64); V = rng.integers(-2, 3, (500, 9)).astype(np.float64)
    index, item = special_csr(rng, d1, 500)
    shuffled = item.copy()
    for u in range(d1):
        rng.shuffle(shuffled[index[u]:index[u + 1]])
    a = pcr.recommend(U, V, 10, exclude=(index, item), dtype=dtype)
    b = pcr.recommend(U, V, 10, exclude=(index, shuffled), dtype=dtype)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
def test_real_valued_factors_against_host_scores(dtype):
    import primalcr_amd as pcr
    rng = np.random.default_rng(5)
    for d1, d2, k in ((300, 3706, 100), (200, 5000, 200), (130, 777, 13)):
        U, V = pcr.initial(d1, k), pcr.initial(d2, k) * 0.5
        if dtype == 0:
            U, V = U.astype(np.float32).astype(np.float64), V.astype(np.float32).astype(np.float64)
        index, item = special_csr(rng, d1, d2)
        M = excl_mask(d1, d2, index, item)
        for K in (10, 100, 1024):
            gi, gs = pcr.recommend(U, V, K, exclude=(index, item), dtype=dtype)
            check_real(U, V, M, gi, gs, K, dtype == 0)


def _train_data(seed=21):
    from primalcr_amd import synth
    import primalcr_amd as pcr
    R = synth.generate("small", seed=seed)
    return R, pcr.Dataset.from_ratings(R)


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_solver_entry_equals_model_entry():
    import primalcr_amd as pcr
    R, ds = _train_data()
    r = 16
    for solver_type, prec in ((pcr.PCR_SOLVER_PCRPP, pcr.PCR_F32), (pcr.PCR_SOLVER_PCRPP, pcr.PCR_F64), (pcr.PCR_SOLVER_CCDR1, pcr.PCR_F32),
                              (pcr.PCR_SOLVER_CCDR1, pcr.PCR_F64)):
        s = pcr.Solver(ds, pcr.Parameter(k=r, precision=prec, solver_type=solver_type, **{"lambda": 100.0}))
        if solver_type == pcr.PCR_SOLVER_CCDR1:
            s.set_factors(pcr.initial_col(R.d1, r), np.zeros((R.d2, r)))
        else:
            s.set_factors(pcr.initial(R.d1, r), pcr.initial(R.d2, r))
        s.iterate(2)
        U, V = s.get_factors()
        for K in (10, 100, 1024):
            a = s.recommend(K)
            b = pcr.recommend(U, V, K, exclude=ds, dtype=prec)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (solver_type, prec, K)
        a = s.recommend(10, exclude_train=False)
        b = pcr.recommend(U, V, 10, dtype=prec)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        idx, it, _ = ds.csr(0)
        M = excl_mask(R.d1, R.d2, idx, it)
        check_real(U, V, M, *s.recommend(50), 50, prec == pcr.PCR_F32)
        s.close()


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_recommend_and_evaluate_topn_profile_slots():
    import primalcr_amd as pcr
    R, ds = _train_data()
    s = pcr.Solver(ds, pcr.Parameter(k=8, **{"lambda": 100.0}))
    s.set_factors(pcr.initial(R.d1, 8), pcr.initial(R.d2, 8))
    s.profile(True)
    s.recommend(10)
    s.evaluate_topn((5, 10))
    prof = s.profile_all()
    for slot in ("recommend/score", "recommend/merge", "recommend/metrics"):
        assert slot in prof and prof[slot][1] > 0, prof
    s.close()


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_invariance_determinism_and_training_untouched():
    import primalcr_amd as pcr
    R, ds = _train_data(seed=4)
    rng = np.random.default_rng(9)
    for prec in (pcr.PCR_F32, pcr.PCR_F64):
        mk = lambda: pcr.Solver(ds, pcr.Parameter(k=12, precision=prec, **{"lambda": 100.0}))
        s, t = mk(), mk()
        U0, V0 = pcr.initial(R.d1, 12), pcr.initial(R.d2, 12)
        s.set_factors(U0, V0); t.set_factors(U0, V0)
        s.iterate(1); t.iterate(1)
        full = s.recommend(20)
        again = s.recommend(20)
        assert np.array_equal(full[0], again[0]) and np.array_equal(full[1].view(np.int64), again[1].view(np.int64))
        perm = rng.permutation(R.d1).astype(np.int32)
        for part in np.array_split(perm, 5):
            a = s.recommend(20, users=part)
            assert np.array_equal(a[0], full[0][part]) and np.array_equal(a[1], full[1][part])
        rev = np.arange(R.d1, dtype=np.int32)[::-1].copy()
        a = s.recommend(20, users=rev)
        assert np.array_equal(a[0], full[0][rev]) and np.array_equal(a[1], full[1][rev])
        U, V = s.get_factors()
        m = pcr.recommend(U, V, 20, exclude=ds, dtype=prec, users=perm[:37])
        assert np.array_equal(m[0], full[0][perm[:37]]) and np.array_equal(m[1], full[1][perm[:37]])
        # training after a recommend call: bitwise the factors of training without it
        s.iterate(2); t.iterate(2)
        Us, Vs = s.get_factors(); Ut, Vt = t.get_factors()
        assert np.array_equal(Us, Ut) and np.array_equal(Vs, Vt)
        s.close(); t.close()


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_shards_serve_their_own_users():
    import primalcr_amd as pcr
    R, ds = _train_data(seed=8)
    idx, it, val = ds.csr(0)
    r = 10
    U, V = pcr.initial(R.d1, r), pcr.initial(R.d2, r)
    for prec in (pcr.PCR_F32, pcr.PCR_F64):
        p = pcr.Parameter(k=r, precision=prec, **{"lambda": 100.0})
        one = pcr.Solver(ds, p)
        one.set_factors(U, V)
        want = one.recommend(25)
        one.close()
        cut = [0, 211, R.d1]
        got_i, got_s = [], []
        for rank in range(2):
            a, b = cut[rank], cut[rank + 1]
            li = (idx[a:b + 1] - idx[a]).astype(np.int64)
            dsl = pcr.Dataset.from_csr(b - a, R.d2, li, it[idx[a]:idx[b]].astype(np.int32), val[idx[a]:idx[b]].copy())
            s = pcr.Solver(dsl, p, rank=rank, nranks=2, shard=(a, R.d1))
            s.set_factors_local(U[a:b], V)
            gi, gs = s.recommend(25)
            sub = s.recommend(25, users=np.arange(b - 1, a - 1, -1, dtype=np.int32))
            assert np.array_equal(sub[0], gi[::-1]) and np.array_equal(sub[1], gs[::-1])
            got_i.append(gi); got_s.append(gs)
            outside = np.array([b % R.d1 if rank == 0 else 0], np.int32)
            with pytest.raises(pcr.PcrError, match="error -1"):
                s.recommend(25, users=outside)
            s.close()
        assert np.array_equal(np.concatenate(got_i), want[0]) and np.array_equal(np.concatenate(got_s), want[1])


@pytest.mark.gpu
@pytest.mark.timeout(1800)
def test_netflix_shape_f32():
    import primalcr_amd as pcr
    from primalcr_amd import synth
    R = synth.generate_fast("netflix")
    d1, d2, k, K = R.d1, R.d2, 100, 100
    U = pcr.initial(d1, k).astype(np.float32).astype(np.float64)
    V = (pcr.initial(d2, k) * 0.3).astype(np.float32).astype(np.float64)
    index = np.ascontiguousarray(R.index, np.int64); item = np.ascontiguousarray(R.item, np.int32)
    gi, gs = pcr.recommend(U, V, K, exclude=(index, item), dtype=pcr.PCR_F32)
    assert gi.shape == (d1, K)
    rng = np.random.default_rng(3)
    sample = np.sort(rng.choice(d1, 2000, replace=False))
    M = np.zeros((sample.shape[0], d2), bool)
    for i, u in enumerate(sample):
        M[i, item[index[u]:index[u + 1]]] = True
    check_real(U[sample], V, M, gi[sample], gs[sample], K, True)


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
    ds = pcr.Dataset.load(d)

    def lines(path):
        return open(path).read().splitlines()

    def fmt(users, it, sc, with_scores):
        res = []
        for u, row, srow in zip(users, it, sc):
            parts = [str(u + 1)]
            for j, s in zip(row, srow):
                if j < 0:
                    break
                parts.append(f"{j + 1}:{s:f}" if with_scores else str(j + 1))
            res.append(" ".join(parts))
        return res

    r = run([RECOMMEND, "-x", d, "m.model", "all.txt"], tmp_path)
    assert r.returncode == 0, r.stderr
    it, sc = pcr.recommend(U, V, 10, exclude=ds)
    assert lines(tmp_path / "all.txt") == fmt(range(R.d1), it, sc, False)

    users = np.array([7, 0, R.d1 - 1, 7, 42], np.int32)
    (tmp_path / "users").write_text("".join(f"{u + 1}\n" for u in users))
    r = run([RECOMMEND, "-K", "1024", "-u", "users", "--scores", "--f32", "-x", d, "m.model", "some.txt"], tmp_path)
    assert r.returncode == 0, r.stderr
    it, sc = pcr.recommend(U, V, 1024, exclude=ds, users=users, dtype=pcr.PCR_F32)
    assert lines(tmp_path / "some.txt") == fmt(users, it, sc, True)

    r = run([RECOMMEND, "-K", "5", "m.model", "nox.txt"], tmp_path)
    assert r.returncode == 0, r.stderr
    it, sc = pcr.recommend(U, V, 5)
    assert lines(tmp_path / "nox.txt") == fmt(range(R.d1), it, sc, False)
