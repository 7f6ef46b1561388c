"""Filtered evaluation (pcr_evaluate_topn_filtered(_model), pcr_evaluate_ranks_filtered(_model), pcr_sample_negatives; Python
evaluate_topn / evaluate_ranks(allow=, candidates=), sample_negatives(); omp-pmf-recommend --eval --among / --eval-candidates /
--negatives): the top-N and the exact rank metrics within an allow set and within a candidate row per user.

CPU part: the argument checks of the four entries (before any device is looked for), the "no device" error, the sampler against a
restatement of its rule in Python integers, the CLI's refusals and usage text.
GPU part (-m gpu), on integer factors in -3..3 (every score exact, ties everywhere), fp32 and fp64: against the brute-force
definitions of tests/filtered_eval_ref.py -- ranks[] and the per-user tables with ==, the means over users to rel 1e-12 (their
order of summation differs from numpy's; the bound check_summary of tests/test_rank_metrics.py uses); against the composition
recommend(filter) + evaluate_lists(test restricted on the host), bit for bit; against the unfiltered entries with a filter that
lets everything through, bit for bit; the top-N hits from the ranks; the solver entry against the model entry; the CLI.
"""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import BIN_DIR, ROOT

import filtered_eval_ref as ref

RECOMMEND = os.path.join(BIN_DIR, "omp-pmf-recommend")
ERR_ARG, ERR_DEVICE = -1, -4
D1 = 37                  # three waves of 16 users in the sweeps: the last one has 5 active lanes


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def run(cmd, cwd, timeout=600):
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=timeout)


def _ptr(a):
    return None if a is None else a.ctypes.data


def _filter(allow, cand):
    import ctypes
    from primalcr_amd.api import ItemFilter
    f = ItemFilter()
    if allow is not None:
        f.allow = allow.ctypes.data
    if cand is not None:
        f.cand_ptr = _ptr(cand[0]); f.cand_item = _ptr(cand[1])
    return ctypes.byref(f), f


def _call(entry, U, V, index, item, tindex, titem, tval, allow=None, cand=None, null_filter=False, threshold=-math.inf, cutoffs=(3,), dtype=1,
          stats=True):
    """One of the two model entries through ctypes, arrays as given (None = NULL); returns the status code."""
    import ctypes
    import primalcr_amd as pcr
    from primalcr_amd.api import RankStats, TopnStats
    fref, _keep = _filter(allow, cand)
    fp = None if null_filter else fref
    L = pcr.lib()
    if entry == "topn":
        cuts = np.ascontiguousarray(cutoffs, np.int32)
        st = (TopnStats * max(len(cutoffs), 1))()
        return L.pcr_evaluate_topn_filtered_model(_ptr(U), U.shape[0], _ptr(V), V.shape[0], U.shape[1], _ptr(index), _ptr(item), _ptr(tindex),
                                                  _ptr(titem), _ptr(tval), len(cutoffs), cuts.ctypes.data, float(threshold), dtype, fp,
                                                  ctypes.cast(st, ctypes.c_void_p) if stats else None, None, 0)
    st = RankStats()
    return L.pcr_evaluate_ranks_filtered_model(_ptr(U), U.shape[0], _ptr(V), V.shape[0], U.shape[1], _ptr(index), _ptr(item), _ptr(tindex),
                                               _ptr(titem), _ptr(tval), float(threshold), dtype, fp, ctypes.addressof(st) if stats else None,
                                               None, None, 0)


def _solver_call(entry, h, allow=None, cand=None, null_filter=False, threshold=-math.inf, cutoffs=(3,), flags=1, stats=True):
    """One of the two solver entries through ctypes on the solver handle h (None = a NULL solver); returns the status code."""
    import ctypes
    import primalcr_amd as pcr
    from primalcr_amd.api import RankStats, TopnStats
    fref, _keep = _filter(allow, cand)
    fp = None if null_filter else fref
    L = pcr.lib()
    if entry == "topn":
        cuts = np.ascontiguousarray(cutoffs, np.int32)
        st = (TopnStats * max(len(cutoffs), 1))()
        return L.pcr_evaluate_topn_filtered(h, len(cutoffs), cuts.ctypes.data, float(threshold), flags, fp,
                                            ctypes.cast(st, ctypes.c_void_p) if stats else None, None)
    st = RankStats()
    return L.pcr_evaluate_ranks_filtered(h, float(threshold), flags, fp, ctypes.addressof(st) if stats else None, None, None)


# ---------------------------------------------------------------------------------------------------------------- CPU
def _small():
    rng = np.random.default_rng(1)
    U, V = rng.standard_normal((20, 5)), rng.standard_normal((30, 5))
    index = np.array([0] + [2] * 20, np.int64)
    item = np.array([3, 7], np.int32)
    tindex = np.array([0, 3] + [4] * 19, np.int64)
    titem = np.array([9, 1, 9, 4], np.int32)
    tval = np.array([5.0, 3.0, 4.0, 1.0])
    allow = np.ones(30, np.uint8)
    cptr = np.arange(21, dtype=np.int64) * 2
    citem = np.tile(np.array([9, 4], np.int32), 20)
    return (U, V, index, item, tindex, titem, tval), allow, (cptr, citem)


@pytest.mark.parametrize("entry", ["topn", "ranks"])
def test_model_entry_argument_checks(entry):
    import primalcr_amd as pcr
    ok, allow, (cptr, citem) = _small()
    name = f"pcr_evaluate_{entry}_filtered_model".encode()
    err = lambda: pcr.lib().pcr_last_error()

    assert _call(entry, *ok, null_filter=True) == ERR_ARG
    assert name in err() and f"pcr_evaluate_{entry}_model".encode() in err()   # the message points at the unfiltered entry
    assert _call(entry, *ok) == ERR_ARG                                        # a filter with nothing in it
    assert name in err() and f"pcr_evaluate_{entry}_model".encode() in err()
    bad = cptr.copy(); bad[0] = 1
    assert _call(entry, *ok, cand=(bad, citem)) == ERR_ARG and name in err()
    bad = cptr.copy(); bad[4] = 2
    assert _call(entry, *ok, cand=(bad, citem)) == ERR_ARG and name in err()   # not monotone
    assert _call(entry, *ok, cand=(cptr, None)) == ERR_ARG and name in err()   # cand_ptr without cand_item
    bad = citem.copy(); bad[7] = 30
    assert _call(entry, *ok, cand=(cptr, bad)) == ERR_ARG and name in err() and b"outside" in err()
    bad = citem.copy(); bad[7] = -1
    assert _call(entry, *ok, cand=(cptr, bad)) == ERR_ARG and name in err()
    bad = citem.copy(); bad[7] = bad[6]
    assert _call(entry, *ok, cand=(cptr, bad)) == ERR_ARG and name in err() and b"twice" in err()
    assert _call(entry, *ok, allow=allow, threshold=math.nan) == ERR_ARG and name in err()
    assert _call(entry, *ok, allow=allow, stats=False) == ERR_ARG and name in err()
    assert _call(entry, *ok, allow=allow, dtype=5) == ERR_ARG and name in err()
    U, V, index, item, tindex, titem, tval = ok
    assert _call(entry, U, V, index, item, tindex, np.array([9, 1, 30, 4], np.int32), tval, allow=allow) == ERR_ARG and name in err()
    if entry == "topn":
        for cuts in ((), (0,), (5, 5), (3, 2), (1025,), tuple(range(1, 10))):
            assert _call(entry, *ok, allow=allow, cutoffs=cuts) == ERR_ARG and name in err(), cuts
    # the Python wrappers: the library's refusals come back as PcrError, the shape of the candidate rows is checked before
    fn = pcr.evaluate_topn if entry == "topn" else pcr.evaluate_ranks
    with pytest.raises(pcr.PcrError):
        fn(U, V, (tindex, titem, tval), candidates=(cptr, bad))
    with pytest.raises(ValueError):
        fn(U, V, (tindex, titem, tval), candidates=(cptr[:-1], citem))
    with pytest.raises(ValueError):
        fn(U, V, (tindex, titem, tval), allow=np.ones(29, np.uint8))


@pytest.mark.parametrize("entry", ["topn", "ranks"])
def test_solver_entry_refuses_a_null_solver(entry):
    import primalcr_amd as pcr
    _, allow, cand = _small()
    assert _solver_call(entry, None, allow=allow) == ERR_ARG and b"null solver" in pcr.lib().pcr_last_error()
    assert _solver_call(entry, None, cand=cand) == ERR_ARG
    assert _solver_call(entry, None, null_filter=True) == ERR_ARG


def test_header_and_constants():
    import primalcr_amd as pcr
    hdr = open(os.path.join(ROOT, "include", "primalcr.h")).read()
    m = re.search(r"#define PCR_CAND_RANK_STAGE (\d+)\b", hdr)
    assert m and int(m.group(1)) == pcr.PCR_CAND_RANK_STAGE
    topk = open(os.path.join(ROOT, "primalcr_amd", "csrc", "pcr_topk.h")).read()
    assert re.search(rf"constexpr int RANK_STAGE = {pcr.PCR_RANK_STAGE};", topk)
    assert "constexpr int CAND_STAGE = PCR_CAND_RANK_STAGE;" in topk
    for name in ("pcr_evaluate_topn_filtered_model", "pcr_evaluate_topn_filtered", "pcr_evaluate_ranks_filtered_model",
                 "pcr_evaluate_ranks_filtered"):
        assert re.search(rf"\b{name}\([^;]*;\s*/\* \[device\] \*/", hdr), name
    assert re.search(r"\bpcr_sample_negatives\([^;]*;\n", hdr)                  # host-only: no [device] mark


def test_model_entries_without_a_device_are_a_device_error():
    """Valid arguments on a process that sees no GPU: PCR_ERR_DEVICE (never a CPU path)."""
    code = ("import sys; sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')\n"
            "from test_filtered_eval import _call, _small\n"
            "ok, allow, cand = _small()\n"
            "print(*[_call(e, *ok, allow=a, cand=c, dtype=t) for e in ('topn', 'ranks') for a, c, t in ((allow, None, 1), (None, cand, 0), (allow, cand, 1))])\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    assert [int(x) for x in out.stdout.strip().splitlines()[-1].split()] == [ERR_DEVICE] * 6


def _sampler_case(n_neg, big):
    """d2 = 50; users whose pool has 0, 1, n_neg - 1, n_neg, 2 n_neg - 1, 2 n_neg items and a large pool, and a user without test
    ratings; `big` further users (enough of them make pcr_parallel_ranges take several threads)."""
    d2 = 50
    rng = np.random.default_rng(5)
    pools = [0, 1, n_neg - 1, n_neg, 2 * n_neg - 1, 2 * n_neg, d2 - 4, None]
    tr_rows, te_rows = [], []
    for want in pools + [int(x) for x in rng.integers(0, d2 - 1, big)]:
        if want is None:
            tr_rows.append(rng.choice(d2, 5, replace=False)); te_rows.append(np.zeros(0, np.int64)); continue
        out = rng.permutation(d2)[:d2 - want]                        # the items outside the pool: at least one of them a test item
        nt = int(rng.integers(1, min(4, out.shape[0]) + 1))
        te = out[:nt]
        tr = np.sort(np.concatenate([out[nt:], te[:1]]) if want % 2 else out[nt:])      # (a test item may sit in training too)
        te_rows.append(np.concatenate([te, te[:1]]))                 # a duplicated test item
        tr_rows.append(tr)
    csr = lambda rows: (np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64), np.concatenate(rows).astype(np.int32))
    return d2, csr(tr_rows), csr(te_rows), pools


def test_sample_negatives_against_the_rule():
    import primalcr_amd as pcr
    n_neg = 6
    d2, train, test, pools = _sampler_case(n_neg, big=9000)
    tindex, titem = test
    for include_test in (True, False):
        with pcr.tuned(sample_threads=1):
            idx1, it1 = pcr.sample_negatives(d2, test, train, n_neg=n_neg, seed=3, include_test=include_test)
        with pcr.tuned(sample_threads=4):
            idx4, it4 = pcr.sample_negatives(d2, test, train, n_neg=n_neg, seed=3, include_test=include_test)
        assert np.array_equal(idx1, idx4) and np.array_equal(it1, it4)
        assert idx1.dtype == np.int64 and it1.dtype == np.int32
        # the Python restatement, id for id, on the first 400 users (the pool sizes named above are the first of them)
        sub =(tindex[:401].copy(), titem[:tindex[400]]), (train[0][:401].copy(), train[1][:train[0][400]])
        widx, wit = ref.ref_sample_negatives(d2, sub[0][0], sub[0][1], sub[1], n_neg, 3, include_test)
        assert np.array_equal(idx1[:401], widx) and np.array_equal(it1[:widx[-1]], wit)
        for u in range(idx1.shape[0] - 1):
            row = it1[idx1[u]:idx1[u + 1]]
            te = np.unique(titem[tindex[u]:tindex[u + 1]])
            tr = train[1][train[0][u]:train[0][u + 1]]
            assert np.all(np.diff(row) > 0)
            neg = np.setdiff1d(row, te)
            assert np.intersect1d(neg, tr).shape[0] == 0
            if te.shape[0] == 0:
                assert row.shape[0] == 0
                continue
            pool = d2 - np.union1d(te, tr).shape[0]
            assert neg.shape[0] == min(n_neg, pool)
            assert np.array_equal(np.intersect1d(row, te), te if include_test else te[:0])
            if u < len(pools) and pools[u] is not None:
                assert pool == pools[u]
    other = pcr.sample_negatives(d2, test, train, n_neg=n_neg, seed=4)
    base = pcr.sample_negatives(d2, test, train, n_neg=n_neg, seed=3)
    assert np.array_equal(other[0], base[0]) and not np.array_equal(other[1], base[1])       # two seeds: the same sizes, other items
    # sharding: the key holds the global user id
    a, b = 100, 300
    shard_t = (tindex[a:b + 1] - tindex[a], titem[tindex[a]:tindex[b]])
    shard_x = (train[0][a:b + 1] - train[0][a], train[1][train[0][a]:train[0][b]])
    sidx, sit = pcr.sample_negatives(d2, shard_t, shard_x, n_neg=n_neg, seed=3, first_user=a)
    assert np.array_equal(sidx, base[0][a:b + 1] - base[0][a]) and np.array_equal(sit, base[1][base[0][a]:base[0][b]])
    # no training rows at all
    nidx, nit = pcr.sample_negatives(d2, (tindex[:401].copy(), titem[:tindex[400]]), None, n_neg=n_neg, seed=9)
    widx, wit = ref.ref_sample_negatives(d2, tindex[:401], titem[:tindex[400]], None, n_neg, 9, True)
    assert np.array_equal(nidx, widx) and np.array_equal(nit, wit)
    with pytest.raises(pcr.PcrError):
        pcr.sample_negatives(d2, (tindex, titem), train, n_neg=-1)
    with pytest.raises(pcr.PcrError):
        pcr.sample_negatives(40, (tindex, titem), train)              # a test item outside the catalogue


def test_cli_refusals_and_usage(tmp_path):
    import primalcr_amd as pcr
    r = run([RECOMMEND], tmp_path)
    assert r.returncode == 1
    for flag in ("--among", "--eval-candidates", "--negatives", "--seed"):
        assert flag in r.stdout
    assert r.stdout.startswith("Usage: omp-pmf-recommend [-K topk] [-x data_dir] [-u users_file] [--f32] [--scores] model_file output_file\n")
    rng = np.random.default_rng(2)
    pcr.model_save(str(tmp_path / "ok.model"), rng.standard_normal((6, 4)), rng.standard_normal((9, 4)))
    (tmp_path / "items").write_text("1\n2\n")
    (tmp_path / "cand").write_text("1 2\n" * 6)
    for extra in (["--among", "items"], ["--eval-candidates", "cand"], ["--negatives", "5"], ["--seed", "3"]):
        r = run([RECOMMEND] + extra + ["ok.model", "out"], tmp_path)
        assert r.returncode == 1 and "--eval" in r.stderr, extra       # refused without --eval
    for mode in (["--fold-in", "d", "-l", "1"], ["--fold-in-ridge", "d", "-l", "1"], ["--fold-in-nnls", "d", "-l", "1"], ["--diversity"],
                 ["--mmr", "0.5"], ["--tradeoff", "0.5"]):
        r = run([RECOMMEND, "--eval", "d", "--among", "items"] + mode + ["ok.model"], tmp_path)
        assert r.returncode == 1 and "--among" in r.stderr, mode
    r = run([RECOMMEND, "--eval", "d", "--negatives", "5", "--eval-candidates", "cand", "ok.model"], tmp_path)
    assert r.returncode == 1 and "--negatives does not go with --eval-candidates" in r.stderr
    r = run([RECOMMEND, "--eval", "d", "--seed", "5", "ok.model"], tmp_path)
    assert r.returncode == 1 and "--seed goes with --negatives" in r.stderr
    r = run([RECOMMEND, "--eval", "d", "--negatives", "-2", "ok.model"], tmp_path)
    assert r.returncode == 1 and "--negatives" in r.stderr
    assert not (tmp_path / "out").exists()


# ---------------------------------------------------------------------------------------------------------------- GPU helpers
NOT_COUNTED, ALL_RELEVANT, IN_TRAINING = 7, 8, 9                    # the single-user edges
SIZED = range(11, 18)                                                # users whose |R_u^f| is prescribed


def wanted_sizes():
    import primalcr_amd as pcr
    rs, cs = pcr.PCR_RANK_STAGE, pcr.PCR_CAND_RANK_STAGE
    return [1, rs - 1, rs, rs + 1, cs - 1, cs, cs + 1]


def make_case(seed, d2, k):
    """Integer factors, a training CSR (users without ratings, a user who rated almost everything, duplicates), test rows as
    make_test_csr's (items also in training, duplicated items, users without rows) with the edge users written over them, an
    allow set that bans three items, and candidate rows of lengths 0, 1, 63, 64, 65, 129 and all d2 items shuffled."""
    from test_recommend import special_csr
    from test_topn_eval import make_test_csr
    rng = np.random.default_rng(seed)
    U = rng.integers(-3, 4, (D1, k)).astype(np.float64)
    V = rng.integers(-3, 4, (d2, k)).astype(np.float64)
    index, item = special_csr(rng, D1, d2)
    tindex, titem, tval = make_test_csr(rng, D1, d2, index, item)
    rows = [(titem[tindex[u]:tindex[u + 1]].copy(), tval[tindex[u]:tindex[u + 1]].copy()) for u in range(D1)]
    banned = np.array([1, 40, d2 - 1])
    allow = np.ones(d2, np.uint8); allow[banned] = 0
    allowed = np.nonzero(allow)[0].astype(np.int32)
    cand = [None] * D1
    # the relevant items of this user are all filtered out: banned items in its test row, none of them among its candidates
    rows[NOT_COUNTED] = (banned.astype(np.int32), np.full(3, 5.0))
    cand[NOT_COUNTED] = rng.permutation(allowed)[:20]
    # every eligible item of this user is relevant
    rows[ALL_RELEVANT] = (rng.permutation(allowed).astype(np.int32), np.full(allowed.shape[0], 5.0))
    cand[ALL_RELEVANT] = rng.permutation(allowed)
    # a relevant candidate that sits in the user's training row
    tr = item[index[IN_TRAINING]:index[IN_TRAINING + 1]]
    tr_ok = tr[allow[tr] != 0]
    assert tr_ok.shape[0] > 0
    free = np.setdiff1d(allowed, tr)
    rows[IN_TRAINING] = (np.concatenate([tr_ok[:1], free[:2]]).astype(np.int32), np.full(3, 5.0))
    cand[IN_TRAINING] = rng.permutation(np.union1d(rows[IN_TRAINING][0], rng.permutation(d2)[:12]))
    for u, size in zip(SIZED, wanted_sizes()):                       # |R_u^f| = size under every filter (allowed items, rating 5)
        size = min(size, allowed.shape[0] - 1)
        r = rng.permutation(allowed)[:size].astype(np.int32)
        rows[u] = (r, np.full(size, 5.0))
        cand[u] = rng.permutation(np.union1d(r, rng.permutation(d2)[:int(rng.integers(1, 30))]))
    lens = [0, 1, 63, 64, 65, 129, d2]
    for u, n in enumerate(lens):                                     # (the rows of users 0 .. 6 keep make_test_csr's test rows ...)
        cand[u] = rng.permutation(d2)[:min(n, d2)] if n != 1 else rng.permutation(allowed)[:1]
        if n == 0:
            continue
        j = cand[u][allow[cand[u]] != 0][:1]                         # (... and get an allowed item of the row as a relevant one,
        assert j.shape[0] == 1                                       # so that every row of these lengths but the empty one is counted)
        rows[u] = (np.concatenate([rows[u][0], j]).astype(np.int32), np.concatenate([rows[u][1], [5.0]]))
    for u in range(D1):
        if cand[u] is None:
            cand[u] = rng.permutation(np.union1d(np.unique(rows[u][0]), rng.permutation(d2)[:int(rng.integers(0, 25))]))
    tindex = np.zeros(D1 + 1, np.int64); tindex[1:] = np.cumsum([r[0].shape[0] for r in rows])
    titem = np.concatenate([r[0] for r in rows]).astype(np.int32)
    tval = np.concatenate([r[1] for r in rows]).astype(np.float64)
    cptr = np.zeros(D1 + 1, np.int64); cptr[1:] = np.cumsum([c.shape[0] for c in cand])
    citem = np.concatenate(cand).astype(np.int32)
    assert sorted(set(int(c.shape[0]) for c in cand[:7])) == sorted(set(min(n, d2) for n in lens))
    return dict(U=U, V=V, S=U @ V.T, exclude=(index, item), test=(tindex, titem, tval), allow=allow, candidates=(cptr, citem), d2=d2, k=k)


FILTERS = ("allow", "candidates", "both")


def filter_of(case, which):
    return dict(allow=case["allow"] if which != "candidates" else None, candidates=case["candidates"] if which != "allow" else None)


def check_rank_table(got, want):
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    bad = np.nonzero(ok & (got != want))
    assert bad[0].shape[0] == 0, (bad[0][:5], bad[1][:5], got[bad][:5], want[bad][:5])


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("d2", [63, 64, 65, 130])
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
def test_against_the_definitions(dtype, d2):
    import primalcr_amd as pcr
    from test_rank_metrics import check_summary as check_rank_summary
    from test_topn_eval import check_per_user as check_topn_table, check_summary as check_topn_summary, ref_metrics
    cutoffs = (1, 5, 64, 65)
    sizes_seen = {f: set() for f in FILTERS}
    for k in (1, 7, 33):
        case = make_case(1000 * d2 + 10 * k + dtype, d2, k)
        U, V, S, test = case["U"], case["V"], case["S"], case["test"]
        tindex, titem, tval = test
        for which in FILTERS:
            flt = filter_of(case, which)
            F = ref.eligible(D1, d2, **flt)
            ftest, _ = ref.restrict_test(F, *test)
            for exclude in (case["exclude"], None):
                lists = ref.ref_lists(S, F, exclude, cutoffs[-1])
                for thr in (-math.inf, 4.0):
                    tag = (k, which, exclude is None, thr)
                    want_r, want_pu, want, nrel = ref.ref_ranks(S, F, exclude, tindex, titem, tval, thr)
                    got, pu, ranks = pcr.evaluate_ranks(U, V, test, exclude=exclude, threshold=thr, dtype=dtype, per_user=True, ranks=True, **flt)
                    assert ranks.dtype == np.int64 and np.array_equal(ranks, want_r), tag
                    check_rank_table(pu, want_pu)
                    check_rank_summary(got, want)
                    want_tpu, want_t = ref_metrics(lists, *ftest, cutoffs, thr)
                    got_t, tpu = pcr.evaluate_topn(U, V, test, cutoffs=cutoffs, exclude=exclude, threshold=thr, dtype=dtype, per_user=True, **flt)
                    check_topn_table(tpu, want_tpu)
                    check_topn_summary(got_t, want_t)
                    # the comparison is not empty, and every edge class is in it
                    counted = int((nrel > 0).sum())
                    assert got["users"] == counted == got_t[0]["users"] and 10 <= counted < D1, tag
                    assert nrel[NOT_COUNTED] == 0 and np.all(np.isnan(pu[NOT_COUNTED])) and np.all(np.isnan(tpu[NOT_COUNTED])), tag
                    assert np.all(ranks[tindex[NOT_COUNTED]:tindex[NOT_COUNTED + 1]] == 0), tag
                    assert math.isnan(pu[ALL_RELEVANT, 3]) and pu[ALL_RELEVANT, 0] == 1 and got["users_auc"] < got["users"], tag
                    assert ranks[tindex[IN_TRAINING]] >= 1 and titem[tindex[IN_TRAINING]] in exclude_row(case, IN_TRAINING), tag
                    outside = ~F[np.repeat(np.arange(D1), np.diff(tindex)), titem]
                    assert outside.any() and np.all(ranks[outside] == 0), tag
                    sizes_seen[which] |= set(int(x) for x in nrel[list(SIZED)])
                    if which != "allow":                             # candidate rows of 1, 63, 64, 65, 129 and d2 items reach the kernels
                        cptr = case["candidates"][0]
                        assert [int(x) for x in np.diff(cptr)[:7]] == [min(n, d2) for n in (0, 1, 63, 64, 65, 129, d2)], tag
                        assert nrel[0] == 0 and np.all(nrel[1:7] > 0), (tag, nrel[:7])
                        assert np.all(~np.isnan(pu[1:7, 0])) and np.all(~np.isnan(tpu[1:7, 0, 0])), tag
    for which in FILTERS:
        assert sizes_seen[which] >= set(s for s in wanted_sizes() if s <= d2 - 4), (which, sizes_seen[which])


def exclude_row(case, u):
    index, item = case["exclude"]
    return set(int(j) for j in item[index[u]:index[u + 1]])


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
def test_topn_is_the_composition_it_replaces(dtype):
    """evaluate_topn(filter) per user == evaluate_lists(recommend(filter), the test rows restricted to F_u on the host), bit for bit."""
    import primalcr_amd as pcr
    from test_topn_eval import check_summary as check_topn_summary
    cutoffs = (1, 5, 64, 65)
    for d2, k in ((63, 7), (65, 33), (130, 1), (130, 7)):
        case = make_case(77 + d2 + k, d2, k)
        U, V, test = case["U"], case["V"], case["test"]
        for which in FILTERS:
            flt = filter_of(case, which)
            F = ref.eligible(D1, d2, **flt)
            ftest, _ = ref.restrict_test(F, *test)
            for exclude in (case["exclude"], None):
                items, _ = pcr.recommend(U, V, cutoffs[-1], exclude=exclude, dtype=dtype, **flt)
                for thr in (-math.inf, 4.0):
                    want = pcr.evaluate_lists(items, V, d1=D1, test=ftest, cutoffs=cutoffs, threshold=thr, dtype=dtype, per_user=True)
                    got, pu = pcr.evaluate_topn(U, V, test, cutoffs=cutoffs, exclude=exclude, threshold=thr, dtype=dtype, per_user=True, **flt)
                    assert np.array_equal(bits(pu), bits(want["per_user_topn"])), (d2, k, which, exclude is None, thr)
                    # (the summaries are sums over 37 rows there and over the counted rows here: another order of summation)
                    check_topn_summary(got, want["topn"])
                    assert got[0]["users"] >= 10


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
def test_a_filter_that_lets_everything_through_is_the_unfiltered_entry(dtype):
    """allow = all ones, and candidates = every item in shuffled order for every user: summaries, per-user tables and ranks[]
    bitwise those of the unfiltered entries, at one and at several item splits."""
    import primalcr_amd as pcr
    from test_recommend_grid import rec_geometry
    rng = np.random.default_rng(9 + dtype)
    for d2, k, batch in ((130, 7, 0), (2200, 33, 0), (2200, 5, 16)):
        # 2200 items: both sweeps take two item splits of 1152, so the allow words of a split that starts above 0 are read.  The
        # split count is RecGeom's -- a function of the counted users (at most 37: one workgroup) and d2 alone, whatever the
        # scratch per user -- restated by rec_geometry, whose constants tests/test_recommend_grid.py holds to the source
        for users in (10, D1):
            g = rec_geometry(users, d2, 65, dtype)
            assert len(g) == 1 and (g[0].splits, g[0].per) == ((2, 1152) if d2 == 2200 else (1, 192)), g
        case = make_case(5 + d2 + k, min(d2, 130), k)
        U, test, exclude = case["U"], case["test"], case["exclude"]
        V = rng.integers(-3, 4, (d2, k)).astype(np.float64)
        every = dict(allow=np.ones(d2, np.uint8))
        shuffled = dict(candidates=(np.arange(D1 + 1, dtype=np.int64) * d2, np.concatenate([rng.permutation(d2) for _ in range(D1)]).astype(np.int32)))
        with pcr.tuned(**({"ranks_batch_users": batch} if batch else {})):
            for thr in (-math.inf, 4.0):
                for ex in (exclude, None):
                    want = pcr.evaluate_ranks(U, V, test, exclude=ex, threshold=thr, dtype=dtype, per_user=True, ranks=True)
                    want_t = pcr.evaluate_topn(U, V, test, cutoffs=(1, 5, 64, 65), exclude=ex, threshold=thr, dtype=dtype, per_user=True)
                    assert want[0]["users"] >= 10
                    for flt in (every, shuffled):
                        got = pcr.evaluate_ranks(U, V, test, exclude=ex, threshold=thr, dtype=dtype, per_user=True, ranks=True, **flt)
                        assert got[0] == want[0] and np.array_equal(bits(got[1]), bits(want[1])) and np.array_equal(got[2], want[2])
                        got_t = pcr.evaluate_topn(U, V, test, cutoffs=(1, 5, 64, 65), exclude=ex, threshold=thr, dtype=dtype, per_user=True, **flt)
                        assert got_t[0] == want_t[0] and np.array_equal(bits(got_t[1]), bits(want_t[1]))


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
def test_hits_follow_from_the_ranks_when_train_and_test_are_disjoint(dtype):
    import primalcr_amd as pcr
    from test_rank_metrics import disjoint_test_csr
    cutoffs = (1, 5, 64, 65)
    for d2, k in ((64, 7), (130, 33)):
        case = make_case(31 + d2, d2, k)
        U, V, exclude = case["U"], case["V"], case["exclude"]
        tindex, titem, tval = disjoint_test_csr(np.random.default_rng(d2), D1, d2, *exclude)
        cptr, citem = case["candidates"]
        for which in FILTERS:
            flt = filter_of(case, which)
            _, ranks = pcr.evaluate_ranks(U, V, (tindex, titem, tval), exclude=exclude, dtype=dtype, ranks=True, **flt)
            got, pu = pcr.evaluate_topn(U, V, (tindex, titem, tval), cutoffs=cutoffs, exclude=exclude, dtype=dtype, per_user=True, **flt)
            counted = 0
            for u in range(D1):
                r = ranks[tindex[u]:tindex[u + 1]]
                r = r[r > 0]
                if r.shape[0] == 0:
                    assert np.all(np.isnan(pu[u]))
                    continue
                counted += 1
                assert [int((r <= c).sum()) for c in cutoffs] == [int(x) for x in pu[u, :, 0]], (which, u)
            assert counted == got[0]["users"] and counted >= 5
            for c, cut in enumerate(cutoffs):
                hit = sum(1 for u in range(D1) if (ranks[tindex[u]:tindex[u + 1]] > 0).any()
                          and (ranks[tindex[u]:tindex[u + 1]][ranks[tindex[u]:tindex[u + 1]] > 0] <= cut).any())
                assert got[c]["hit_rate"] == hit / counted


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_solver_entry_equals_model_entry_and_leaves_the_solver_alone():
    import primalcr_amd as pcr
    from primalcr_amd import synth
    R = synth.generate("small", seed=21)
    ds = pcr.Dataset.from_ratings(R)
    idx, it, val = ds.csr(0)
    tidx, tit, tval = ds.csr(1)
    rng = np.random.default_rng(4)
    allow = (rng.random(R.d2) < 0.7).astype(np.uint8)
    cand = pcr.sample_negatives(R.d2, ds, ds, n_neg=20, seed=1)
    r, cutoffs = 16, (5, 10)
    for prec in (pcr.PCR_F32, pcr.PCR_F64):
        p = pcr.Parameter(k=r, precision=prec, **{"lambda": 100.0})
        s, t = pcr.Solver(ds, p), pcr.Solver(ds, p)
        U0, V0 = pcr.initial(R.d1, r), pcr.initial(R.d2, r)
        s.set_factors(U0, V0); t.set_factors(U0, V0)
        s.iterate(1); t.iterate(1)
        U, V = s.get_factors()
        before_r = s.evaluate_ranks(per_user=True, ranks=True)
        before_t = s.evaluate_topn(cutoffs, per_user=True)
        for flt in (dict(allow=allow), dict(candidates=cand), dict(allow=allow, candidates=cand)):
            for excl in (True, False):
                a = s.evaluate_ranks(threshold=4.0, exclude_train=excl, per_user=True, ranks=True, **flt)
                b = pcr.evaluate_ranks(U, V, ds, exclude=ds if excl else None, threshold=4.0, dtype=prec, per_user=True, ranks=True, **flt)
                assert a[0] == b[0] and a[0]["users"] > 50 and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2])
                again = s.evaluate_ranks(threshold=4.0, exclude_train=excl, per_user=True, ranks=True, **flt)
                assert again[0] == a[0] and np.array_equal(bits(again[1]), bits(a[1])) and np.array_equal(again[2], a[2])
                a = s.evaluate_topn(cutoffs, exclude_train=excl, per_user=True, **flt)
                b = pcr.evaluate_topn(U, V, ds, cutoffs=cutoffs, exclude=ds if excl else None, dtype=prec, per_user=True, **flt)
                assert a[0] == b[0] and a[0][0]["users"] > 50 and np.array_equal(bits(a[1]), bits(b[1]))
        # the cached unfiltered tables were not touched
        after_r = s.evaluate_ranks(per_user=True, ranks=True)
        after_t = s.evaluate_topn(cutoffs, per_user=True)
        assert after_r[0] == before_r[0] and np.array_equal(bits(after_r[1]), bits(before_r[1])) and np.array_equal(after_r[2], before_r[2])
        assert after_t[0] == before_t[0] and np.array_equal(bits(after_t[1]), bits(before_t[1]))
        # training after the calls: bitwise the factors of training without them
        s.iterate(1); t.iterate(1)
        Us, Vs = s.get_factors(); Ut, Vt = t.get_factors()
        assert np.array_equal(Us, Ut) and np.array_equal(Vs, Vt)
        s.close(); t.close()
        # two local-only shards: their rows are the whole's, their partial sums add up to it
        flt = dict(allow=allow, candidates=cand)
        want = pcr.evaluate_ranks(U0, V0, ds, exclude=ds, dtype=prec, per_user=True, ranks=True, **flt)
        want_t = pcr.evaluate_topn(U0, V0, ds, cutoffs=cutoffs, exclude=ds, dtype=prec, per_user=True, **flt)
        cut = [0, 211, R.d1]
        parts, rows, rks, tparts, trows = [], [], [], [], []
        for rank in range(2):
            a, b = cut[rank], cut[rank + 1]
            dsl = pcr.Dataset.from_csr(b - a, R.d2, idx[a:b + 1] - idx[a], it[idx[a]:idx[b]], val[idx[a]:idx[b]].copy(),
                                       tidx[a:b + 1] - tidx[a], tit[tidx[a]:tidx[b]], tval[tidx[a]:tidx[b]].copy())
            sh = pcr.Solver(dsl, p, rank=rank, nranks=2, shard=(a, R.d1))
            sh.set_local_only(True)
            sh.set_factors_local(U0[a:b], V0)
            cl = (cand[0][a:b + 1] - cand[0][a], cand[1][cand[0][a]:cand[0][b]])
            st, pu, rk = sh.evaluate_ranks(per_user=True, ranks=True, allow=allow, candidates=cl)
            tst, tpu = sh.evaluate_topn(cutoffs, per_user=True, allow=allow, candidates=cl)
            parts.append(st); rows.append(pu); rks.append(rk); tparts.append(tst); trows.append(tpu)
            sh.close()
        assert np.array_equal(bits(np.concatenate(rows)), bits(want[1])) and np.array_equal(np.concatenate(rks), want[2])
        assert np.array_equal(bits(np.concatenate(trows)), bits(want_t[1]))
        for f in ("users", "users_auc", "relevant"):
            assert sum(q[f] for q in parts) == want[0][f]
        for f, wk in (("mrr", "users"), ("mean_rank", "users"), ("mpr", "users"), ("auc", "users_auc")):
            assert sum(q[f] * q[wk] for q in parts) / want[0][wk] == pytest.approx(want[0][f], rel=1e-12, abs=1e-15)
        for c in range(len(cutoffs)):
            for f in ("users", "users_graded", "hits"):
                assert sum(q[c][f] for q in tparts) == want_t[0][c][f]
            for f in ("precision", "recall", "hit_rate", "map", "ndcg"):
                assert sum(q[c][f] * q[c]["users"] for q in tparts) / want_t[0][c]["users"] == pytest.approx(want_t[0][c][f], rel=1e-12, abs=1e-15)


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("entry", ["topn", "ranks"])
def test_solver_entry_argument_checks(entry):
    """The solver entries' own refusals, on a live solver through ctypes: each PCR_ERR_ARG, the entry named in the message, and
    the solver as usable afterwards as before."""
    import primalcr_amd as pcr
    from primalcr_amd import synth
    R = synth.generate("small", seed=21)
    ds = pcr.Dataset.from_ratings(R)
    s = pcr.Solver(ds, pcr.Parameter(k=8, precision=pcr.PCR_F64, **{"lambda": 100.0}))
    s.set_factors(pcr.initial(R.d1, 8), pcr.initial(R.d2, 8))
    n, d2, h = R.d1, R.d2, s._h
    allow = np.ones(d2, np.uint8); allow[::3] = 0
    cptr, citem = pcr.sample_negatives(d2, ds, ds, n_neg=10, seed=2)
    citem = np.ascontiguousarray(citem)
    assert cptr.shape[0] == n + 1 and cptr[3] - cptr[2] >= 2
    name = f"pcr_evaluate_{entry}_filtered".encode()
    unfiltered = f"(pcr_evaluate_{entry} is the entry without one)".encode()

    def refused(**kw):
        rc = _solver_call(entry, h, **kw)
        msg = pcr.lib().pcr_last_error()
        assert rc == ERR_ARG and name in msg and name + b"_model" not in msg, (kw.keys(), rc, msg)
        return msg

    valid = lambda: (s.evaluate_topn((3, 10), per_user=True, allow=allow, candidates=(cptr, citem)) if entry == "topn"
                     else s.evaluate_ranks(per_user=True, ranks=True, allow=allow, candidates=(cptr, citem)))
    before = valid()
    assert (before[0][0] if entry == "topn" else before[0])["users"] > 50
    assert unfiltered in refused(null_filter=True)
    assert unfiltered in refused()                                               # a filter with nothing in it
    bad = cptr.copy(); bad[0] = 1
    assert b"cand_ptr[0]" in refused(cand=(bad, citem))
    bad = cptr.copy(); bad[3] = bad[2] - 1
    assert b"monotone" in refused(cand=(bad, citem))
    assert b"cand_item" in refused(cand=(cptr, None))
    bad = citem.copy(); bad[cptr[2]] = d2
    assert b"outside" in refused(cand=(cptr, bad))
    bad = citem.copy(); bad[cptr[2]] = -1
    assert b"outside" in refused(cand=(cptr, bad), allow=allow)
    bad = citem.copy(); bad[cptr[2] + 1] = bad[cptr[2]]
    assert b"twice" in refused(cand=(cptr, bad))
    assert b"NaN" in refused(allow=allow, threshold=math.nan)
    assert b"stats" in refused(allow=allow, stats=False)
    assert b"flags" in refused(allow=allow, flags=2)
    assert b"flags" in refused(cand=(cptr, citem), flags=5)
    if entry == "topn":
        for cuts in ((), (0,), (5, 5), (3, 2), (1025,), tuple(range(1, 10))):
            refused(allow=allow, cutoffs=cuts)
    assert _solver_call(entry, h, allow=allow, cand=(cptr, citem)) == 0          # and valid arguments pass through the same path
    after = valid()
    assert after[0] == before[0] and all(np.array_equal(bits(a), bits(b)) for a, b in zip(after[1:], before[1:]))
    s.iterate(1)                                                                 # the solver trains on
    s.close()


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_cli_end_to_end(tmp_path):
    """A 12 x 40 model: the CLI prints what sample_negatives() + evaluate_topn() / evaluate_ranks() give through Python."""
    import primalcr_amd as pcr
    from primalcr_amd import synth
    rng = np.random.default_rng(6)
    d1, d2, k = 12, 40, 5
    U, V = rng.standard_normal((d1, k)), rng.standard_normal((d2, k))
    pcr.model_save(str(tmp_path / "m.model"), U, V)
    user = np.repeat(np.arange(d1), 6).astype(np.int32)
    item = np.concatenate([np.sort(rng.choice(d2, 6, replace=False)) for _ in range(d1)]).astype(np.int32)
    val = rng.integers(1, 6, user.shape[0]).astype(np.float64)
    tr = np.arange(user.shape[0]) % 3 < 2                             # four training and two test ratings per user
    tr[user == 3] = True                                              # ... and a user without test ratings
    d = synth.write_dir(synth.Ratings(d1, d2, user[tr], item[tr], val[tr], user[~tr], item[~tr], val[~tr]), str(tmp_path / "data"))
    ds = pcr.Dataset.load(d)

    def parse(stdout):
        res = []
        for line in stdout.splitlines():
            f = line.split()
            if f[0] == "ranks":
                f = f[1:]
            res.append({f[i]: float(f[i + 1]) for i in range(0, len(f), 2)})
        return res

    def same(printed, want):
        assert len(printed) == len(want)
        for p, w in zip(printed, want):
            for key, v in w.items():
                assert float(f"{v:g}") == p[key], (key, p, w)

    allow = np.zeros(d2, np.uint8); allow[::2] = 1; allow[item[~tr][:8]] = 1
    (tmp_path / "items").write_text("".join(f"{j + 1}\n" for j in np.nonzero(allow)[0]))
    cand = pcr.sample_negatives(d2, ds, ds, n_neg=9, seed=11)
    (tmp_path / "cand").write_text("".join(" ".join(str(j + 1) for j in cand[1][cand[0][u]:cand[0][u + 1]]) + "\n" for u in range(d1)))
    for args, flt in ((["--negatives", "5", "--seed", "3"], dict(candidates=pcr.sample_negatives(d2, ds, ds, n_neg=5, seed=3))),
                      (["--among", "items"], dict(allow=allow)),
                      (["--eval-candidates", "cand", "--among", "items"], dict(allow=allow, candidates=cand))):
        r = run([RECOMMEND, "--eval", d, "--ranks", "-x", d, "-c", "1,5"] + args + ["m.model", "per_user.txt"], tmp_path)
        assert r.returncode == 0, r.stderr
        want_t = pcr.evaluate_topn(U, V, ds, cutoffs=(1, 5), exclude=ds, **flt)
        want_r, pu = pcr.evaluate_ranks(U, V, ds, exclude=ds, per_user=True, **flt)
        assert want_r["users"] >= 8
        same(parse(r.stdout), want_t + [want_r])
        lines = (tmp_path / "per_user.txt").read_text().splitlines()
        counted = np.nonzero(~np.isnan(pu[:, 0]))[0]
        assert len(lines) == counted.shape[0]
        for line, u in zip(lines, counted):
            f = line.split()
            assert int(f[0]) == u + 1 and [float(x) for x in f[1:]] == [float(f"{v:g}") for v in pu[u]]
    r = run([RECOMMEND, "--eval", d, "-x", d, "-c", "5", "--negatives", "5", "--seed", "3", "m.model", "topn.txt"], tmp_path)
    assert r.returncode == 0, r.stderr
    want_t, tpu = pcr.evaluate_topn(U, V, ds, cutoffs=(5,), exclude=ds, per_user=True, candidates=pcr.sample_negatives(d2, ds, ds, n_neg=5, seed=3))
    same(parse(r.stdout), want_t)
    assert len((tmp_path / "topn.txt").read_text().splitlines()) == int((~np.isnan(tpu[:, 0, 0])).sum())
    # a candidates file of empty rows only: nobody is counted, and that is a result, not an error
    (tmp_path / "none").write_text("\n" * d1)
    r = run([RECOMMEND, "--eval", d, "--ranks", "-c", "5", "--eval-candidates", "none", "m.model"], tmp_path)
    assert r.returncode == 0, r.stderr
    printed = parse(r.stdout)
    assert len(printed) == 2 and printed[0]["users"] == 0 and printed[1]["users"] == 0 and printed[1]["relevant"] == 0
