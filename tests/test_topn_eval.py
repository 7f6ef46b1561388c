"""Full-catalogue top-N evaluation (pcr_evaluate_topn_model / pcr_evaluate_topn, omp-pmf-recommend --eval, Python evaluate_topn()).

CPU part: argument checks of the C ABI (before any device is looked for), the "no device" error, the CLI's usage text and its
argument errors.
GPU part (-m gpu): per-user metrics against a numpy evaluation of pcr.recommend's own lists on integer factors (ties
everywhere), the full-catalogue invariant, the solver entry against the model entry, determinism and untouched training,
per-shard rows, the Netflix shape and the CLI end to end.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import BIN_DIR, ROOT

RECOMMEND = os.path.join(BIN_DIR, "omp-pmf-recommend")
TRAIN = os.path.join(BIN_DIR, "omp-pmf-train")
ERR_ARG, ERR_DEVICE = -1, -4
SUMMARY = ("precision", "recall", "hit_rate", "map", "ndcg", "ndcg_graded")


def run(cmd, cwd, timeout=600):
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=timeout)


def _model_call(U, V, index, item, tindex, titem, tval, cutoffs, threshold=-math.inf, dtype=1, stats=True, ncut=None):
    """pcr_evaluate_topn_model through ctypes, arrays as given (None = NULL); returns the status code."""
    import primalcr_amd as pcr
    from primalcr_amd.api import TopnStats
    cuts = np.ascontiguousarray(cutoffs, np.int32)
    ncut = cuts.shape[0] if ncut is None else ncut
    st = (TopnStats * 8)()
    ptr = lambda a: None if a is None else a.ctypes.data
    return pcr.lib().pcr_evaluate_topn_model(ptr(U), U.shape[0], ptr(V), V.shape[0], U.shape[1], ptr(index), ptr(item), ptr(tindex),
                                             ptr(titem), ptr(tval), ncut, cuts.ctypes.data if cuts.shape[0] else None, float(threshold),
                                             dtype, st if stats else None, None, 0)


# ---------------------------------------------------------------------------------------------------------------- CPU
def _small():
    rng = np.random.default_rng(1)
    U, V = rng.standard_normal((20, 5)), rng.standard_normal((30, 5))
    index = np.array([0] + [2] * 20, np.int64)
    item = np.array([3, 7], np.int32)
    tindex = np.array([0, 3] + [4] * 19, np.int64)
    titem = np.array([9, 1, 9, 4], np.int32)
    tval = np.array([5.0, 3.0, 4.0, 1.0])
    return U, V, index, item, tindex, titem, tval


def test_model_entry_argument_checks():
    U, V, index, item, tindex, titem, tval = _small()
    ok = (U, V, index, item, tindex, titem, tval)
    assert _model_call(*ok, [10], ncut=0) == ERR_ARG
    assert _model_call(*ok, list(range(1, 10))) == ERR_ARG                       # 9 cutoffs
    assert _model_call(*ok, []) == ERR_ARG
    assert _model_call(*ok, [5, 5]) == ERR_ARG                                   # not strictly ascending
    assert _model_call(*ok, [10, 5]) == ERR_ARG
    assert _model_call(*ok, [0, 5]) == ERR_ARG
    assert _model_call(*ok, [5, 1025]) == ERR_ARG
    assert _model_call(*ok, [10], threshold=math.nan) == ERR_ARG
    bad = tindex.copy(); bad[5] = 1                                              # test CSR not monotone
    assert _model_call(U, V, index, item, bad, titem, tval, [10]) == ERR_ARG
    bad = tindex.copy(); bad[0] = 1
    assert _model_call(U, V, index, item, bad, titem, tval, [10]) == ERR_ARG
    assert _model_call(U, V, index, item, tindex, np.array([9, 1, 30, 4], np.int32), tval, [10]) == ERR_ARG   # item out of range
    assert _model_call(U, V, index, item, tindex, np.array([9, 1, -1, 4], np.int32), tval, [10]) == ERR_ARG
    assert _model_call(U, V, index, item, tindex, None, tval, [10]) == ERR_ARG
    assert _model_call(*ok, [10], stats=False) == ERR_ARG                        # NULL stats
    assert _model_call(*ok, [10], dtype=5) == ERR_ARG
    assert _model_call(U, V, index, None, tindex, titem, tval, [10]) == ERR_ARG  # exclusion index without item
    ex_bad = index.copy(); ex_bad[3] = 0
    assert _model_call(U, V, ex_bad, item, tindex, titem, tval, [10]) == ERR_ARG
    import primalcr_amd as pcr
    with pytest.raises(pcr.PcrError):
        pcr.evaluate_topn(U, V, (tindex, titem, tval), cutoffs=(10, 5))
    with pytest.raises(ValueError):                                              # last index entry != length of item
        pcr.evaluate_topn(U, V, (tindex, titem[:3], tval[:3]))


def test_model_entry_without_a_device_is_a_device_error():
    """Valid arguments on a process that sees no GPU: PCR_ERR_DEVICE (never a CPU path)."""
    code = ("import sys, math, numpy as np; sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')\n"
            "from test_topn_eval import _model_call, _small\n"
            "print(_model_call(*_small(), [1, 5, 10]), _model_call(*_small(), [3], threshold=4.0, dtype=0))\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    assert [int(x) for x in out.stdout.strip().splitlines()[-1].split()] == [ERR_DEVICE, ERR_DEVICE]


def test_cli_usage(tmp_path):
    r = run([RECOMMEND], tmp_path)
    assert r.returncode == 1
    for opt in ("--eval data_dir", "-c c1,c2,...", "--threshold v"):
        assert opt in r.stdout, opt
    r = run([RECOMMEND, "--eval"], tmp_path)                                     # --eval without a directory
    assert r.returncode == 1 and "--eval" in r.stderr and r.stdout.startswith("Usage: omp-pmf-recommend")


def test_cli_argument_errors(tmp_path):
    import primalcr_amd as pcr
    from primalcr_amd import synth
    R = synth.generate("tiny", seed=3)                      # 60 x 40
    d = synth.write_dir(R, str(tmp_path / "data"))
    rng = np.random.default_rng(2)
    pcr.model_save(str(tmp_path / "ok.model"), rng.standard_normal((R.d1, 4)), rng.standard_normal((R.d2, 4)))
    pcr.model_save(str(tmp_path / "wrong.model"), rng.standard_normal((R.d1 + 1, 4)), rng.standard_normal((R.d2, 4)))
    for bad in ("", "abc", "5,", ",5", "5,,10", "10,5", "5,5", "0", "1025", "1,2,3,4,5,6,7,8,9", "5;10"):
        r = run([RECOMMEND, "--eval", d, "-c", bad, "ok.model"], tmp_path)
        assert r.returncode == 1 and "-c" in r.stderr, (bad, r.stderr)
    for bad in ("abc", "nan", ""):
        r = run([RECOMMEND, "--eval", d, "--threshold", bad, "ok.model"], tmp_path)
        assert r.returncode == 1 and "--threshold" in r.stderr, (bad, r.stderr)
    r = run([RECOMMEND, "--eval", d, "wrong.model"], tmp_path)                   # dims of meta and model differ
    assert r.returncode == 1 and "data set" in r.stderr and "the model" in r.stderr
    r = run([RECOMMEND, "--eval", d], tmp_path)                                  # no model
    assert r.returncode == 1 and r.stdout.startswith("Usage: omp-pmf-recommend")
    r = run([RECOMMEND, "--eval", str(tmp_path / "missing_dir"), "ok.model"], tmp_path)
    assert r.returncode == 1 and r.stderr
    r = run([RECOMMEND, "-c", "5", "ok.model", "out"], tmp_path)                 # -c without --eval
    assert r.returncode == 1 and "--eval" in r.stderr


# ---------------------------------------------------------------------------------------------------------------- GPU helpers
def ref_metrics(items, tindex, titem, tval, cutoffs, threshold):
    """numpy/Python evaluation of given lists (rows = users) under the contract of include/primalcr.h: (per_user, summary)."""
    d1, ncut, K = items.shape[0], len(cutoffs), items.shape[1]
    disc = 1.0 / np.log2(np.arange(K, dtype=np.float64) + 2.0)
    per = np.full((d1, ncut, 6), np.nan)
    for u in range(d1):
        gains = {}
        for z in range(tindex[u], tindex[u + 1]):
            if tval[z] >= threshold:
                j = int(titem[z])
                gains[j] = max(gains.get(j, -math.inf), float(tval[z]))
        if not gains:
            continue
        g = {j: 2.0 ** v - 1.0 for j, v in gains.items()}
        gdesc = sorted(g.values(), reverse=True)
        nr = len(g)
        rel = np.array([int(j) in g for j in items[u]])
        cum = np.cumsum(rel)
        for c, cut in enumerate(cutoffs):
            m = min(cut, nr)
            pos = np.nonzero(rel[:cut])[0]
            hits = pos.shape[0]
            ap = sum(cum[i] / (i + 1) for i in pos) / m
            ndcg = sum(disc[i] for i in pos) / sum(disc[:m])
            gid = sum(gdesc[i] * disc[i] for i in range(m))
            gd = sum(g[int(items[u][i])] * disc[i] for i in pos)
            per[u, c] = (hits, hits / cut, hits / nr, ap, ndcg, gd / gid if gid > 0 else np.nan)
    summary = []
    counted = ~np.isnan(per[:, 0, 0])
    n = int(counted.sum())
    for c, cut in enumerate(cutoffs):
        P = per[counted, c]
        graded = ~np.isnan(P[:, 5])
        ng = int(graded.sum())
        mean = lambda x, k: float(x.sum()) / k if k else 0.0
        summary.append(dict(cutoff=cut, users=n, users_graded=ng, hits=int(P[:, 0].sum()), precision=mean(P[:, 1], n),
                            recall=mean(P[:, 2], n), hit_rate=mean(P[:, 0] > 0, n), map=mean(P[:, 3], n), ndcg=mean(P[:, 4], n),
                            ndcg_graded=mean(P[graded, 5], ng)))
    return per, summary


def check_per_user(got, want):
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want[..., 0])
    assert np.array_equal(got[..., 0][ok], want[..., 0][ok])                    # hits exactly
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)


def check_summary(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for f in ("cutoff", "users", "users_graded", "hits"):
            assert g[f] == w[f], (f, g, w)
        for f in SUMMARY:
            assert g[f] == pytest.approx(w[f], rel=1e-12, abs=0), (f, g, w)


def make_test_csr(rng, d1, d2, index, item, empty_every=6):
    """Test CSR (items in random order within a row) with: items also in training, duplicated items, users without test rows,
    users whose ratings all sit below 4; integer ratings 1..5."""
    rows, vals = [], []
    for u in range(d1):
        if u % empty_every == 2:
            rows.append(np.zeros(0, np.int32)); vals.append(np.zeros(0)); continue
        n = int(rng.integers(1, 15))
        r = rng.integers(0, d2, n).astype(np.int32)
        tr = item[index[u]:index[u + 1]]
        if tr.shape[0] and u % 3 == 0:
            r = np.concatenate([r, tr[:2]])                         # also in training
        if u % 4 == 1:
            r = np.concatenate([r, r[:2]])                          # duplicated (the duplicate gets its own rating)
        v = rng.integers(1, 6, r.shape[0]).astype(np.float64)
        if u % 5 == 4:
            v = np.minimum(v, 3.0)                                  # nothing at or above 4
        p = rng.permutation(r.shape[0])
        rows.append(r[p]); vals.append(v[p])
    tindex = np.zeros(d1 + 1, np.int64)
    tindex[1:] = np.cumsum([r.shape[0] for r in rows])
    return tindex, np.concatenate(rows).astype(np.int32), np.concatenate(vals)




def as_dicts(stats):
    return [dict(s) for s in stats]


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
def test_exact_metrics_on_integer_factors(dtype):
    import primalcr_amd as pcr
    from test_recommend import special_csr
    rng = np.random.default_rng(31 + dtype)
    d1, cutoffs = 150, (1, 5, 10, 37)
    for k, d2 in ((7, 30), (16, 500), (64, 3706)):
        U = rng.integers(-2, 3, (d1, k)).astype(np.float64)
        V = rng.integers(-2, 3, (d2, k)).astype(np.float64)
        index, item = special_csr(rng, d1, d2)                      # user 5 rated all but 3 items: fewer eligible than 37
        tindex, titem, tval = make_test_csr(rng, d1, d2, index, item)
        test = (tindex, titem, tval)
        for exclude in ((index, item), None):
            items, _ = pcr.recommend(U, V, cutoffs[-1], exclude=exclude, dtype=dtype)
            for thr in (-math.inf, 4.0):
                want_pu, want = ref_metrics(items, tindex, titem, tval, cutoffs, thr)
                got, pu = pcr.evaluate_topn(U, V, test, cutoffs=cutoffs, exclude=exclude, threshold=thr, dtype=dtype, per_user=True)
                check_per_user(pu, want_pu)
                check_summary(got, want)
                assert got[0]["users"] < d1                         # users without (relevant) test ratings are not counted
                if thr == 4.0:
                    assert got[0]["users"] < pcr.evaluate_topn(U, V, test, cutoffs=cutoffs, exclude=exclude, dtype=dtype)[0]["users"]
        # a single cutoff without per-user output gives the same summary
        items, _ = pcr.recommend(U, V, 10, exclude=(index, item), dtype=dtype)
        check_summary(pcr.evaluate_topn(U, V, test, cutoffs=10, exclude=(index, item), dtype=dtype),
                      ref_metrics(items, tindex, titem, tval, (10,), -math.inf)[1])


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_full_catalogue_cutoff_finds_every_relevant_item():
    """Cutoff = d2 without exclusion lists the whole catalogue: recall and hit_rate are 1 and precision is |R_u| / d2 whatever the
    factors.  NDCG and MAP are 1 only for a ranker that puts the relevant items first (by descending rating for the graded
    NDCG): factors U[u, j] = 2 + v_max(u, j) for relevant items, 0 else, and V = I give exactly that ranking."""
    import primalcr_amd as pcr
    from test_recommend import special_csr
    rng = np.random.default_rng(7)
    d1 = 120
    for d2 in (37, 1000, 1024):
        index, item = special_csr(rng, d1, d2)
        tindex, titem, tval = make_test_csr(rng, d1, d2, index, item)
        nrel = np.array([np.unique(titem[tindex[u]:tindex[u + 1]]).shape[0] for u in range(d1)])
        Up = np.zeros((d1, d2))
        for u in range(d1):
            for z in range(tindex[u], tindex[u + 1]):
                Up[u, titem[z]] = max(Up[u, titem[z]], 2.0 + tval[z])
        for U, V, perfect in ((rng.standard_normal((d1, 9)), rng.standard_normal((d2, 9)), False), (Up, np.eye(d2), True)):
            for dtype in (0, 1):
                got, pu = pcr.evaluate_topn(U, V, (tindex, titem, tval), cutoffs=(1, d2), dtype=dtype, per_user=True)
                ok = ~np.isnan(pu[:, 1, 0])
                assert np.array_equal(ok, nrel > 0)
                assert got[1]["users"] == got[1]["users_graded"] == int(ok.sum())
                assert np.array_equal(pu[ok, 1, 0], nrel[ok])                # hits
                np.testing.assert_allclose(pu[ok, 1, 1], nrel[ok] / d2, rtol=1e-12)
                np.testing.assert_allclose(pu[ok, 1, 2], 1.0, rtol=1e-12)   # recall
                assert got[1]["recall"] == pytest.approx(1.0, rel=1e-12) and got[1]["hit_rate"] == 1.0
                if perfect:
                    for f in (3, 4, 5):                                   # ap, ndcg, ndcg_graded (ratings >= 1: always defined)
                        np.testing.assert_allclose(pu[ok, 1, f], 1.0, rtol=1e-12)
                        np.testing.assert_allclose(pu[ok, 0, f], 1.0, rtol=1e-12)
                    for f in ("map", "ndcg", "ndcg_graded"):
                        assert got[1][f] == pytest.approx(1.0, rel=1e-12), f
                    assert got[0]["hit_rate"] == 1.0 and got[0]["precision"] == 1.0


def _train_data(seed=21):
    from primalcr_amd import synth
    import primalcr_amd as pcr
    R = synth.generate("small", seed=seed)
    return R, pcr.Dataset.from_ratings(R)


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_solver_entry_equals_model_entry_and_leaves_training_alone():
    import primalcr_amd as pcr
    R, ds = _train_data()
    r, cutoffs = 16, (5, 10, 50)
    for solver_type in (pcr.PCR_SOLVER_PCRPP, pcr.PCR_SOLVER_CCDR1):
        for prec in (pcr.PCR_F32, pcr.PCR_F64):
            p = pcr.Parameter(k=r, precision=prec, solver_type=solver_type, **{"lambda": 100.0})
            s, t = pcr.Solver(ds, p), pcr.Solver(ds, p)
            if solver_type == pcr.PCR_SOLVER_CCDR1:
                U0, V0 = pcr.initial_col(R.d1, r), np.zeros((R.d2, r))
            else:
                U0, V0 = pcr.initial(R.d1, r), pcr.initial(R.d2, r)
            s.set_factors(U0, V0); t.set_factors(U0, V0)
            s.iterate(2); t.iterate(2)
            U, V = s.get_factors()
            for thr in (-math.inf, 4.0):
                a, apu = s.evaluate_topn(cutoffs, threshold=thr, per_user=True)
                b, bpu = pcr.evaluate_topn(U, V, ds, cutoffs=cutoffs, exclude=ds, threshold=thr, dtype=prec, per_user=True)
                assert a == b, (solver_type, prec, thr)
                assert np.array_equal(apu.view(np.int64), bpu.view(np.int64))
                again, again_pu = s.evaluate_topn(cutoffs, threshold=thr, per_user=True)
                assert again == a and np.array_equal(again_pu.view(np.int64), apu.view(np.int64))
            a = s.evaluate_topn((10,), exclude_train=False)
            b = pcr.evaluate_topn(U, V, ds, cutoffs=(10,), dtype=prec)
            assert a == b
            items, _ = s.recommend(50)
            tidx, tit, tval = ds.csr(1)
            want_pu, want = ref_metrics(items, tidx, tit, tval, cutoffs, -math.inf)
            got, pu = s.evaluate_topn(cutoffs, per_user=True)
            check_per_user(pu, want_pu); check_summary(got, want)
            # training after the calls: bitwise the factors of training without them
            s.iterate(2); t.iterate(2)
            Us, Vs = s.get_factors(); Ut, Vt = t.get_factors()
            assert np.array_equal(Us, Ut) and np.array_equal(Vs, Vt), (solver_type, prec)
            s.close(); t.close()


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_shards_give_their_own_rows_and_partials():
    import primalcr_amd as pcr
    R, ds = _train_data(seed=8)
    idx, it, val = ds.csr(0)
    tidx, tit, tval = ds.csr(1)
    r, cutoffs = 10, (3, 20)
    U, V = pcr.initial(R.d1, r), pcr.initial(R.d2, r)
    for prec in (pcr.PCR_F32, pcr.PCR_F64):
        p = pcr.Parameter(k=r, precision=prec, **{"lambda": 100.0})
        one = pcr.Solver(ds, p)
        one.set_factors(U, V)
        want, want_pu = one.evaluate_topn(cutoffs, per_user=True)
        one.close()
        cut = [0, 211, R.d1]
        parts, rows = [], []
        for rank in range(2):
            a, b = cut[rank], cut[rank + 1]
            dsl = pcr.Dataset.from_csr(b - a, R.d2, idx[a:b + 1] - idx[a], it[idx[a]:idx[b]], val[idx[a]:idx[b]].copy(),
                                       tidx[a:b + 1] - tidx[a], tit[tidx[a]:tidx[b]], tval[tidx[a]:tidx[b]].copy())
            s = pcr.Solver(dsl, p, rank=rank, nranks=2, shard=(a, R.d1))
            s.set_local_only(True)
            s.set_factors_local(U[a:b], V)
            st, pu = s.evaluate_topn(cutoffs, per_user=True)
            parts.append(st); rows.append(pu)
            s.close()
        assert np.array_equal(np.concatenate(rows).view(np.int64), want_pu.view(np.int64))
        for c in range(len(cutoffs)):
            for f in ("users", "users_graded", "hits"):
                assert sum(q[c][f] for q in parts) == want[c][f]
            for f in SUMMARY:
                wk = "users_graded" if f == "ndcg_graded" else "users"
                tot = sum(q[c][f] * q[c][wk] for q in parts) / want[c][wk]
                assert tot == pytest.approx(want[c][f], rel=1e-12, abs=1e-15), f


@pytest.mark.gpu
@pytest.mark.timeout(1800)
def test_netflix_shape_f32():
    import primalcr_amd as pcr
    from primalcr_amd import synth
    R = synth.generate_fast("netflix")
    d1, d2, k, K = R.d1, R.d2, 100, 10
    U = pcr.initial(d1, k).astype(np.float32).astype(np.float64)
    V = (pcr.initial(d2, k) * 0.3).astype(np.float32).astype(np.float64)
    index = np.ascontiguousarray(R.index, np.int64); item = np.ascontiguousarray(R.item, np.int32)
    tindex = np.ascontiguousarray(R.tindex, np.int64); titem = np.ascontiguousarray(R.titem, np.int32)
    tval = np.ascontiguousarray(R.tval, np.float64)
    got, pu = pcr.evaluate_topn(U, V, (tindex, titem, tval), cutoffs=(1, 5, K), exclude=(index, item), dtype=pcr.PCR_F32, per_user=True)
    has_test = np.diff(tindex) > 0
    assert np.array_equal(~np.isnan(pu[:, 0, 0]), has_test)
    assert got[0]["users"] == int(has_test.sum())
    rng = np.random.default_rng(3)
    sample = np.sort(rng.choice(d1, 2000, replace=False)).astype(np.int32)
    items, _ = pcr.recommend(U, V, K, exclude=(index, item), users=sample, dtype=pcr.PCR_F32)
    sub_idx = np.zeros(sample.shape[0] + 1, np.int64)
    sub_idx[1:] = np.cumsum(tindex[sample + 1] - tindex[sample])
    sel = np.concatenate([np.arange(tindex[u], tindex[u + 1]) for u in sample])
    want_pu, _ = ref_metrics(items, sub_idx, titem[sel], tval[sel], (1, 5, K), -math.inf)
    check_per_user(pu[sample], want_pu)


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

    def parse(stdout):
        res = []
        for line in stdout.splitlines():
            f = line.split()
            res.append({f[i]: float(f[i + 1]) for i in range(0, len(f), 2)})
        return res

    def same(printed, want):
        assert len(printed) == len(want)
        for p, w in zip(printed, want):
            for key, v in w.items():
                assert float(f"{v:g}") == p[key], (key, p, w)

    r = run([RECOMMEND, "--eval", d, "-x", d, "-c", "5,10,20", "m.model", "per_user.txt"], tmp_path)
    assert r.returncode == 0, r.stderr
    want, pu = pcr.evaluate_topn(U, V, ds, cutoffs=(5, 10, 20), exclude=ds, per_user=True)
    same(parse(r.stdout), want)
    lines = (tmp_path / "per_user.txt").read_text().splitlines()
    counted = np.nonzero(~np.isnan(pu[:, -1, 0]))[0]
    assert len(lines) == counted.shape[0]
    for line, u in zip(lines, counted):
        f = line.split()
        assert int(f[0]) == u + 1
        assert [float(x) for x in f[1:]] == [float(f"{v:g}") for v in pu[u, -1]]

    r = run([RECOMMEND, "--eval", d, "-K", "7", "--threshold", "4", "--f32", "m.model"], tmp_path)
    assert r.returncode == 0, r.stderr
    same(parse(r.stdout), pcr.evaluate_topn(U, V, ds, cutoffs=(7,), threshold=4.0, dtype=pcr.PCR_F32))
