"""Filtered top-K recommendation (pcr_recommend_filtered_model / pcr_recommend_filtered, recommend(allow=, candidates=),
omp-pmf-recommend --allow / --candidates).

CPU part: the exported symbols, every argument error of the filter with the entry's name in the message, the device error of a
process without a GPU, the CLI's refusals and its file errors, the first usage line.
GPU part (-m gpu): exact lists on integer factors (every score exact in f32 and fp64, ties everywhere) against ref_topk with
the ineligible items masked out -- allow sets built around the 64-item words and the item splits of the sweep, candidate rows
of every length around the kernel's steps, its buffer and K, in four orders --, bit equality with the unfiltered call on
real-valued factors, invariance, the solver entry, the profile slots, the CLI and the sampled-negatives protocol end to end.
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import BIN_DIR, ROOT
from test_recommend import check_real, excl_mask, lex_equal, ref_topk, special_csr
from test_recommend_grid import boundaries, csr_of, rec_geometry

RECOMMEND = os.path.join(BIN_DIR, "omp-pmf-recommend")
ERR_ARG, ERR_DEVICE = -1, -4
USAGE_LINE_1 = "Usage: omp-pmf-recommend [-K topk] [-x data_dir] [-u users_file] [--f32] [--scores] model_file output_file"


def run(cmd, cwd, timeout=300):
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=timeout)


def _filtered_call(U, V, users, K, allow=None, cand_ptr=None, cand_item=None, no_filter=False, dtype=1):
    """pcr_recommend_filtered_model through ctypes, arrays as given (None = NULL); returns (status, message)."""
    import primalcr_amd as pcr
    n = len(users) if users is not None else U.shape[0]
    items = np.empty(max(n, 1) * max(K, 1), np.int32); scores = np.empty(max(n, 1) * max(K, 1), np.float64)
    ptr = lambda a: None if a is None else a.ctypes.data
    f = pcr.api.ItemFilter(ptr(allow), ptr(cand_ptr), ptr(cand_item))
    rc = pcr.lib().pcr_recommend_filtered_model(ptr(U), U.shape[0], ptr(V), V.shape[0], U.shape[1], None, None, n, ptr(users), K, dtype,
                                                None if no_filter else C.byref(f), items.ctypes.data, scores.ctypes.data, 0)
    return rc, pcr.lib().pcr_last_error().decode()


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_both_symbols_are_exported():
    import primalcr_amd as pcr
    L = pcr.lib()
    assert hasattr(L, "pcr_recommend_filtered_model") and hasattr(L, "pcr_recommend_filtered")


def test_filter_argument_errors():
    import primalcr_amd as pcr
    rng = np.random.default_rng(1)
    d1, d2 = 20, 30
    U, V = rng.standard_normal((d1, 5)), rng.standard_normal((d2, 5))
    users = np.array([4, 9, 17], np.int32)
    who = "pcr_recommend_filtered_model"
    ptr = np.array([0, 2, 2, 5], np.int64)
    item = np.array([3, 7, 0, 29, 11], np.int32)
    rc, msg = _filtered_call(U, V, users, 5, no_filter=True)
    assert rc == ERR_ARG and who in msg and "pcr_recommend " in msg + " ", msg
    rc, msg = _filtered_call(U, V, users, 5)                                     # a filter with nothing in it
    assert rc == ERR_ARG and who in msg and "pcr_recommend " in msg + " ", msg
    rc, msg = _filtered_call(U, V, users, 5, cand_ptr=np.array([1, 2, 2, 5], np.int64), cand_item=item)
    assert rc == ERR_ARG and who in msg and "cand_ptr[0]" in msg, msg
    rc, msg = _filtered_call(U, V, users, 5, cand_ptr=np.array([0, 3, 2, 5], np.int64), cand_item=item)
    assert rc == ERR_ARG and who in msg and "monotone" in msg and "user 9" in msg, msg
    rc, msg = _filtered_call(U, V, users, 5, cand_ptr=ptr)
    assert rc == ERR_ARG and who in msg and "cand_item" in msg, msg
    for bad in (-1, d2):
        it = item.copy(); it[3] = bad
        rc, msg = _filtered_call(U, V, users, 5, cand_ptr=ptr, cand_item=it)
        assert rc == ERR_ARG and who in msg and f"id {bad} " in msg and "user 17" in msg, msg
    it = item.copy(); it[4] = it[2]                                               # an id twice in the last row, not adjacent
    rc, msg = _filtered_call(U, V, users, 5, cand_ptr=ptr, cand_item=it)
    assert rc == ERR_ARG and who in msg and "twice" in msg and "user 17" in msg, msg
    it = item.copy(); it[1] = it[0]
    rc, msg = _filtered_call(U, V, None, 5, cand_ptr=np.array([0, 2] + [5] * (d1 - 1), np.int64), cand_item=it)   # users NULL: the row is the user
    assert rc == ERR_ARG and "twice" in msg and "user 0" in msg, msg
    # the checks of pcr_recommend_model still come first, under this entry's name
    rc, msg = _filtered_call(U, V, users, 1025, allow=np.ones(d2, np.uint8))
    assert rc == ERR_ARG and who in msg and "K = 1025" in msg, msg
    rc, msg = _filtered_call(U, V, np.array([d1], np.int32), 5, allow=np.ones(d2, np.uint8))
    assert rc == ERR_ARG and who in msg, msg
    # Python: shape errors are ValueError
    with pytest.raises(ValueError):
        pcr.recommend(U, V, 5, allow=np.ones(d2 + 1, bool))
    with pytest.raises(ValueError):
        pcr.recommend(U, V, 5, allow=np.ones((d2, 1), bool))
    with pytest.raises(ValueError):                                               # one row per requested user
        pcr.recommend(U, V, 5, users=users, candidates=(np.array([0, 2, 5], np.int64), item))
    with pytest.raises(ValueError):                                               # last index entry != length of item
        pcr.recommend(U, V, 5, users=users, candidates=(ptr, item[:4]))
    with pytest.raises(pcr.PcrError, match="error -1.*twice"):
        pcr.recommend(U, V, 5, users=users, candidates=(ptr, it[[1, 0, 2, 3, 4]]))


def test_filtered_entry_without_a_device_is_a_device_error():
    """Valid arguments on a process that sees no GPU: PCR_ERR_DEVICE (never a CPU path)."""
    code = ("import sys, numpy as np; sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')\n"
            "from test_recommend_filter import _filtered_call\n"
            "U = np.ones((4, 3)); V = np.ones((6, 3)); users = np.arange(4, dtype=np.int32)\n"
            "print(_filtered_call(U, V, users, 3, allow=np.ones(6, np.uint8))[0])\n"
            "print(_filtered_call(U, V, users, 3, cand_ptr=np.array([0, 1, 1, 3, 4], np.int64), cand_item=np.array([2, 0, 5, 1], np.int32))[0])\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    assert [int(x) for x in out.stdout.strip().splitlines()[-2:]] == [ERR_DEVICE, ERR_DEVICE]


def test_cli_refusals_and_file_errors(tmp_path):
    import primalcr_amd as pcr
    r = run([RECOMMEND], tmp_path)
    assert r.returncode == 1 and r.stdout.splitlines()[0] == USAGE_LINE_1
    assert "--allow" in r.stdout and "--candidates" in r.stdout
    for flag in ("--allow", "--candidates"):
        for other in (["--eval", "d"], ["--diversity"], ["--mmr", "0.5"], ["--tradeoff", "0,0.5"], ["--eval", "d", "--ranks"], ["--ranks"],
                      ["--fold-in", "d", "-l", "1"]):
            r = run([RECOMMEND, flag, "f"] + other + ["m", "o"], tmp_path)
            assert r.returncode == 1 and "--allow and --candidates do not go with" in r.stderr, (flag, other, r.stderr)
        r = run([RECOMMEND, "m", "o", flag], tmp_path)
        assert r.returncode == 1 and "needs a value" in r.stderr
    rng = np.random.default_rng(2)
    d1, d2 = 12, 40
    pcr.model_save(str(tmp_path / "ok.model"), rng.standard_normal((d1, 4)), rng.standard_normal((d2, 4)))
    (tmp_path / "users").write_text("3\n1\n7\n")
    for content, what in (("1 2\nx\n3\n", "line 2: not an item id"), ("1 2\n3 4x\n5\n", "line 2: not an item id"), ("1\n0\n2\n", "outside"),
                          (f"1\n2\n{d2 + 1}\n", "outside"), ("1\n2\n", "2 lines for 3 requested users"), ("1\n2\n3\n4\n", "4 lines for 3 requested users")):
        (tmp_path / "cands").write_text(content)
        r = run([RECOMMEND, "-u", "users", "--candidates", "cands", "ok.model", "out"], tmp_path)
        assert r.returncode == 1 and what in r.stderr, (content, r.stderr)
    (tmp_path / "cands").write_text("1 2\n\n3 4 3\n")                             # an id twice in a row: the library's own message
    r = run([RECOMMEND, "-u", "users", "--candidates", "cands", "ok.model", "out"], tmp_path)
    assert r.returncode == 1 and "twice" in r.stderr and "pcr_recommend_filtered_model" in r.stderr, r.stderr
    r = run([RECOMMEND, "--candidates", "cands", "ok.model", "out"], tmp_path)    # every user of the model is requested
    assert r.returncode == 1 and f"3 lines for {d1} requested users" in r.stderr, r.stderr
    r = run([RECOMMEND, "--candidates", "missing", "ok.model", "out"], tmp_path)
    assert r.returncode == 1 and "can't open candidates file" in r.stderr
    for content, what in (("1\nx\n", "not an item id"), ("0\n", "outside"), (f"{d2 + 1}\n", "outside")):
        (tmp_path / "allow").write_text(content)
        r = run([RECOMMEND, "--allow", "allow", "ok.model", "out"], tmp_path)
        assert r.returncode == 1 and what in r.stderr, (content, r.stderr)
    r = run([RECOMMEND, "--allow", "missing", "ok.model", "out"], tmp_path)
    assert r.returncode == 1 and "can't open allow file" in r.stderr


# ---------------------------------------------------------------------------------------------------------------- GPU helpers
def same_bits(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int64), b[1].view(np.int64))


def elig_of(n, d2, allow=None, cands=None):
    """The eligibility of the filter alone, [n, d2]: the candidate rows (or everything) intersected with the allow mask."""
    E = np.ones((n, d2), bool)
    if cands is not None:
        E[:] = False
        for i in range(n):
            E[i, cands[1][cands[0][i]:cands[0][i + 1]]] = True
    if allow is not None:
        E &= np.asarray(allow, bool)[None, :]
    return E


def struck_out(full, E, K):
    """The full ranking full = (items, scores) [n, d2] with the ineligible entries struck out, cut to K and padded."""
    n = full[0].shape[0]
    items = np.full((n, K), -1, np.int32); scores = np.full((n, K), -np.inf)
    for i in range(n):
        keep = (full[0][i] >= 0)
        keep[keep] = E[i, full[0][i][keep]]
        it, sc = full[0][i][keep][:K], full[1][i][keep][:K]
        items[i, :it.shape[0]] = it; scores[i, :it.shape[0]] = sc
    return items, scores


def real_factors(d1, d2, k, dtype):
    import primalcr_amd as pcr
    U, V = pcr.initial(d1, k), pcr.initial(d2, k) * 0.5
    if dtype == 0:
        U, V = U.astype(np.float32).astype(np.float64), V.astype(np.float32).astype(np.float64)
    return U, V


def random_rows(rng, n, d2, lo, hi):
    return csr_of([rng.choice(d2, int(rng.integers(lo, hi)), replace=False).astype(np.int32) for _ in range(n)])


# ---------------------------------------------------------------------------------------------------------------- GPU, exact
ALLOW_D1, ALLOW_KS = 150, (1, 10, 1024)
ALLOW_SHAPES = {130: 1, 2112: 2, 16500: 16}        # d2: the item splits of the sweep for 150 users


@functools.lru_cache(maxsize=None)
def allow_case(d2):
    """Integer factors (the scores are exact in f32 and fp64, with many ties), the exclusion of special_csr, the masks around the
    words and splits of the sweep and, per (mask, exclusion), ref_topk's lists at K = 1024 -- shorter K are their prefixes.
    Computed once and shared by both dtypes; nothing here is written afterwards."""
    rng = np.random.default_rng(100 + d2)
    d1, k = ALLOW_D1, 7
    U = rng.integers(-2, 3, (d1, k)).astype(np.float64)
    V = rng.integers(-2, 3, (d2, k)).astype(np.float64)
    S = U @ V.T                                            # exact: |s| <= 4 k
    index, item = special_csr(rng, d1, d2)
    M = excl_mask(d1, d2, index, item)
    per = rec_geometry(d1, d2, 1024, 1)[0].per
    nsp = -(-d2 // per)
    ones = np.ones(d2, bool)
    masks = {"ones": ones, "zeros": ~ones}
    m = ~ones; m[[0, d2 - 1]] = True
    masks["ends"] = m
    m = ones.copy(); m[64:128] = False
    masks["but_one_word"] = m
    m = ones.copy(); m[(nsp - 1) * per:] = False           # (one split: everything, which equals "zeros" by another road)
    masks["but_one_split"] = m
    m = ~ones
    for b in sorted(set(range(64, d2, 64)) | set(boundaries(d2, per))):
        m[[j for j in (b - 1, b, b + 1) if j < d2]] = True
    masks["boundary_bits"] = m
    masks["half"] = rng.random(d2) < 0.5
    m = ~ones; m[rng.choice(d2, 7, replace=False)] = True
    masks["fewer_than_k"] = m
    for m in masks.values():
        m.setflags(write=False)
    none = np.zeros_like(M)
    refs = {(name, ex): ref_topk(S, (M if ex else none) | ~m[None, :], 1024) for name, m in masks.items() for ex in (False, True)}
    return U, V, (index, item), masks, refs


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("d2", sorted(ALLOW_SHAPES))
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
def test_allow_set_exact_on_integer_factors(dtype, d2):
    import primalcr_amd as pcr
    U, V, excl, masks, refs = allow_case(d2)
    for K in ALLOW_KS:
        g = rec_geometry(ALLOW_D1, d2, K, dtype)
        assert len(g) == 1 and g[0].splits == ALLOW_SHAPES[d2], g
        for name, m in masks.items():
            for ex in (False, True):
                gi, gs = pcr.recommend(U, V, K, exclude=excl if ex else None, dtype=dtype, allow=m)
                ri, rs = refs[(name, ex)]
                assert np.array_equal(gi, ri[:, :K]), (d2, K, name, ex)
                lex_equal(gi, gs, ri[:, :K], rs[:, :K])
                if name == "ones":                         # the unfiltered entry, exactly
                    assert same_bits((gi, gs), pcr.recommend(U, V, K, exclude=excl if ex else None, dtype=dtype)), (d2, K, ex)
                if name == "zeros":
                    assert (gi == -1).all() and np.isneginf(gs).all()
                if name == "fewer_than_k" and K > 7 and not ex:
                    assert ((gi >= 0).sum(axis=1) == 7).all()


CAND_D2, CAND_KS = 3000, (1, 10, 100, 1024)


def ladder(K):
    return [0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, K - 1, K, K + 1, 1023, 1024, 1025, 2049, 3000]


@functools.lru_cache(maxsize=None)
def cand_case(K):
    """Integer factors over 3000 items, special_csr's exclusion (user 5 rated all but three items) and one request per length of
    ladder(K): user i gets a random subset of that size, id-ascending.  One more request has only items of its own training row.
    Returns the expected lists with exclusion on, without and with an allow mask on top; shared by both dtypes, never written."""
    rng = np.random.default_rng(200 + K)
    d2, k = CAND_D2, 9
    lens = ladder(K)
    d1 = len(lens) + 5
    U = rng.integers(-2, 3, (d1, k)).astype(np.float64)
    V = rng.integers(-2, 3, (d2, k)).astype(np.float64)
    index, item = special_csr(rng, d1, d2)
    users = np.array(list(range(len(lens))) + [12], np.int32)
    rows = [np.sort(rng.choice(d2, n, replace=False)).astype(np.int32) for n in lens]
    rows.append(np.unique(item[index[12]:index[13]]).astype(np.int32))      # every candidate is a training item: all padding
    assert rows[-1].shape[0] > 0
    S = U[users] @ V.T
    M = excl_mask(d1, d2, index, item)[users]
    allow = rng.random(d2) < 0.5
    allow.setflags(write=False)
    E = elig_of(users.shape[0], d2, cands=csr_of(rows))
    want = ref_topk(S, M | ~E, K)
    want_allow = ref_topk(S, M | ~(E & allow[None, :]), K)
    assert (want[0][-1] == -1).all()
    return U, V, (index, item), users, rows, S, allow, want, want_allow


def ordered(rows, S, order, rng):
    out = []
    for i, r in enumerate(rows):
        if order == "ascending_id":
            o = np.arange(r.shape[0])
        elif order == "random":
            o = rng.permutation(r.shape[0])
        else:
            o = np.lexsort((r, -S[i, r]))                  # the order of a list: best first
            if order == "score_ascending":                 # every candidate beats the threshold: the worst case for the merges
                o = o[::-1]
        out.append(r[o])
    return csr_of(out)


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("K", CAND_KS)
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
def test_candidate_lists_exact_in_every_order(dtype, K):
    import primalcr_amd as pcr
    U, V, excl, users, rows, S, allow, want, want_allow = cand_case(K)
    rng = np.random.default_rng(K)
    first = None
    for order in ("ascending_id", "random", "score_ascending", "score_descending"):
        cands = ordered(rows, S, order, rng)
        got = pcr.recommend(U, V, K, exclude=excl, users=users, dtype=dtype, candidates=cands)
        lex_equal(*got, *want)
        got_allow = pcr.recommend(U, V, K, exclude=excl, users=users, dtype=dtype, candidates=cands, allow=allow)
        lex_equal(*got_allow, *want_allow)
        if first is None:
            first = (got, got_allow)
        assert same_bits(got, first[0]) and same_bits(got_allow, first[1]), order
    assert (got[0][-1] == -1).all() and (got[0][0] == -1).all()                   # the row without eligible candidates, the empty row


# ---------------------------------------------------------------------------------------------------------------- GPU, bit equality
@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("k", [13, 100, 200])
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
def test_filtered_scores_have_the_bits_of_recommend(dtype, k):
    import primalcr_amd as pcr
    rng = np.random.default_rng(300 + k)
    d1, d2, K = 70, 1000, 50
    U, V = real_factors(d1, d2, k, dtype)
    excl = special_csr(rng, d1, d2)
    plain = pcr.recommend(U, V, K, exclude=excl, dtype=dtype)
    assert same_bits(pcr.recommend(U, V, K, exclude=excl, dtype=dtype, allow=np.ones(d2, bool)), plain)
    whole = csr_of([rng.permutation(d2).astype(np.int32) for _ in range(d1)])
    assert same_bits(pcr.recommend(U, V, K, exclude=excl, dtype=dtype, candidates=whole), plain)
    A = rng.random(d2) < 0.3
    ids = np.nonzero(A)[0].astype(np.int32)
    by_mask = pcr.recommend(U, V, K, exclude=excl, dtype=dtype, allow=A)
    by_rows = pcr.recommend(U, V, K, exclude=excl, dtype=dtype, candidates=csr_of([rng.permutation(ids) for _ in range(d1)]))
    assert same_bits(by_mask, by_rows)
    # the unfiltered full ranking with the ineligible entries struck out
    full = pcr.recommend(U, V, d2, exclude=excl, dtype=dtype)
    cands = random_rows(rng, d1, d2, 0, 400)
    for allow, cd in ((A, None), (None, cands), (A, cands)):
        got = pcr.recommend(U, V, K, exclude=excl, dtype=dtype, allow=allow, candidates=cd)
        assert same_bits(got, struck_out(full, elig_of(d1, d2, allow, cd), K)), (allow is None, cd is None)
    assert same_bits(by_mask, struck_out(full, elig_of(d1, d2, A), K))


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
def test_real_valued_factors_with_a_random_filter(dtype):
    import primalcr_amd as pcr
    rng = np.random.default_rng(7)
    d1, d2, k, K = 60, 3706, 100, 100
    U, V = real_factors(d1, d2, k, dtype)
    index, item = special_csr(rng, d1, d2)
    M = excl_mask(d1, d2, index, item)
    allow = rng.random(d2) < 0.5
    cands = random_rows(rng, d1, d2, 50, 2000)
    for a, c in ((allow, None), (None, cands), (allow, cands)):
        gi, gs = pcr.recommend(U, V, K, exclude=(index, item), dtype=dtype, allow=a, candidates=c)
        check_real(U, V, M | ~elig_of(d1, d2, a, c), gi, gs, K, dtype == 0)


# ---------------------------------------------------------------------------------------------------------------- GPU, invariance and plumbing
@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f64"])
def test_a_list_depends_on_its_user_alone(dtype):
    import primalcr_amd as pcr
    rng = np.random.default_rng(17)
    d1, d2, k, K = 100, 2500, 24, 20
    U, V = real_factors(d1, d2, k, dtype)
    excl = special_csr(rng, d1, d2)
    allow = rng.random(d2) < 0.6
    rows = [rng.choice(d2, int(rng.integers(0, 300)), replace=False).astype(np.int32) for _ in range(d1)]
    for kw in (dict(allow=allow), dict(candidates=csr_of(rows)), dict(allow=allow, candidates=csr_of(rows))):
        sub = lambda users: {**kw, **({"candidates": csr_of([rows[u] for u in users])} if "candidates" in kw else {})}
        full = pcr.recommend(U, V, K, exclude=excl, dtype=dtype, **kw)
        assert same_bits(full, pcr.recommend(U, V, K, exclude=excl, dtype=dtype, **kw))          # two identical calls
        perm = rng.permutation(d1).astype(np.int32)[:37]
        a = pcr.recommend(U, V, K, exclude=excl, dtype=dtype, users=perm, **sub(perm))
        assert same_bits(a, (full[0][perm], full[1][perm]))
        for u in (0, 5, 63, 64, 99):
            one = np.array([u], np.int32)
            a = pcr.recommend(U, V, K, exclude=excl, dtype=dtype, users=one, **sub(one))
            assert same_bits(a, (full[0][one], full[1][one])), u


def _solver_data(seed):
    import primalcr_amd as pcr
    from primalcr_amd import synth
    R = synth.generate("small", seed=seed)
    return R, pcr.Dataset.from_ratings(R)


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_solver_entry_equals_model_entry_and_leaves_training_alone():
    import primalcr_amd as pcr
    R, ds = _solver_data(21)
    rng = np.random.default_rng(3)
    r, K = 12, 30
    allow = rng.random(R.d2) < 0.5
    users = rng.permutation(R.d1).astype(np.int32)[:90]
    cands = random_rows(rng, users.shape[0], R.d2, 0, 200)
    all_rows = random_rows(rng, R.d1, R.d2, 0, 40)
    for solver_type, prec in ((pcr.PCR_SOLVER_PCRPP, pcr.PCR_F32), (pcr.PCR_SOLVER_PCRPP, pcr.PCR_F64), (pcr.PCR_SOLVER_CCDR1, pcr.PCR_F64)):
        p = pcr.Parameter(k=r, precision=prec, solver_type=solver_type, **{"lambda": 100.0})
        s, t = pcr.Solver(ds, p), pcr.Solver(ds, p)
        if solver_type == pcr.PCR_SOLVER_CCDR1:
            U0, V0 = pcr.initial_col(R.d1, r), np.zeros((R.d2, r))
        else:
            U0, V0 = pcr.initial(R.d1, r), pcr.initial(R.d2, r)
        s.set_factors(U0, V0); t.set_factors(U0, V0)
        s.iterate(1); t.iterate(1)
        U, V = s.get_factors()
        for ex in (True, False):
            for kw in (dict(allow=allow), dict(users=users, candidates=cands), dict(users=users, allow=allow, candidates=cands),
                       dict(candidates=all_rows)):
                a = s.recommend(K, exclude_train=ex, **kw)
                b = pcr.recommend(U, V, K, exclude=ds if ex else None, dtype=prec, **kw)
                assert same_bits(a, b), (solver_type, prec, ex, sorted(kw))
        s.iterate(1); t.iterate(1)                         # training after the filtered calls: bitwise that of the twin without them
        Us, Vs = s.get_factors(); Ut, Vt = t.get_factors()
        assert np.array_equal(Us, Ut) and np.array_equal(Vs, Vt), (solver_type, prec)
        s.close(); t.close()


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_shard_users_and_profile_slots():
    import primalcr_amd as pcr
    R, ds = _solver_data(8)
    idx, it, val = ds.csr(0)
    rng = np.random.default_rng(5)
    r, K = 8, 10
    U, V = pcr.initial(R.d1, r), pcr.initial(R.d2, r)
    p = pcr.Parameter(k=r, **{"lambda": 100.0})
    allow = rng.random(R.d2) < 0.5
    a, b = 211, R.d1                                       # the second of two shards
    dsl = pcr.Dataset.from_csr(b - a, R.d2, (idx[a:b + 1] - idx[a]).astype(np.int64), it[idx[a]:idx[b]].astype(np.int32), val[idx[a]:idx[b]].copy())
    s = pcr.Solver(dsl, p, rank=1, nranks=2, shard=(a, R.d1))
    s.set_factors_local(U[a:b], V)
    users = np.array([b - 1, a, a + 7], np.int32)          # global ids
    cands = random_rows(rng, 3, R.d2, 5, 100)
    got = s.recommend(K, users=users, allow=allow, candidates=cands)
    assert same_bits(got, pcr.recommend(U, V, K, exclude=(idx, it.astype(np.int32)), users=users, dtype=p.precision, allow=allow, candidates=cands))
    for outside in (0, a - 1):
        with pytest.raises(pcr.PcrError, match="error -1"):
            s.recommend(K, users=np.array([a, outside], np.int32), allow=allow)
        with pytest.raises(pcr.PcrError, match="error -1"):
            s.recommend(K, users=np.array([a, outside], np.int32), candidates=csr_of([np.arange(3, dtype=np.int32)] * 2))
    # the slots count the launches: an allow set alone is one sweep and one merge, candidate lists one launch of their own kernel
    launches = lambda: {n: v[1] for n, v in s.profile_all().items() if n.startswith("recommend/")}
    s.profile(True)
    s.recommend(K, allow=allow)
    assert launches() == {"recommend/score": 1, "recommend/merge": 1}
    s.recommend(K, users=users, candidates=cands)
    s.recommend(K, users=users, candidates=cands, allow=allow)
    assert launches() == {"recommend/score": 1, "recommend/merge": 1, "recommend/candidates": 2}
    s.close()


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_cli_equals_the_python_call(tmp_path):
    import primalcr_amd as pcr
    from primalcr_amd import synth
    R = synth.generate("tiny", seed=3)                     # 60 x 40
    d = synth.write_dir(R, str(tmp_path / "data"))
    ds = pcr.Dataset.load(d)
    rng = np.random.default_rng(4)
    U, V = rng.standard_normal((R.d1, 6)), rng.standard_normal((R.d2, 6))
    pcr.model_save(str(tmp_path / "m.model"), U, V)
    U, V = pcr.model_load(str(tmp_path / "m.model"))

    def fmt(users, it, sc, with_scores):
        res = []
        for u, row, srow in zip(users, it, sc):
            res.append(" ".join([str(u + 1)] + [f"{j + 1}:{s:f}" if with_scores else str(j + 1) for j, s in zip(row, srow) if j >= 0]))
        return res

    lines = lambda name: open(tmp_path / name).read().splitlines()
    allow = np.zeros(R.d2, bool); allow[rng.choice(R.d2, 25, replace=False)] = True
    (tmp_path / "allow").write_text("".join(f"{j + 1}\n" for j in rng.permutation(np.nonzero(allow)[0])))
    users = np.array([7, 0, R.d1 - 1, 7, 42], np.int32)
    (tmp_path / "users").write_text("".join(f"{u + 1}\n" for u in users))
    rows = [rng.choice(R.d2, n, replace=False).astype(np.int32) for n in (12, 0, 40, 1, 20)]
    (tmp_path / "cands").write_text("".join(" ".join(str(j + 1) for j in r) + "\n" for r in rows))

    r = run([RECOMMEND, "--allow", "allow", "-x", d, "m.model", "a.txt"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert lines("a.txt") == fmt(range(R.d1), *pcr.recommend(U, V, 10, exclude=ds, allow=allow), False)
    r = run([RECOMMEND, "-K", "5", "-u", "users", "--candidates", "cands", "--scores", "--f32", "-x", d, "m.model", "c.txt"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert lines("c.txt") == fmt(users, *pcr.recommend(U, V, 5, exclude=ds, users=users, dtype=pcr.PCR_F32, candidates=csr_of(rows)), True)
    r = run([RECOMMEND, "-K", "5", "-u", "users", "--candidates", "cands", "--allow", "allow", "m.model", "b.txt"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert lines("b.txt") == fmt(users, *pcr.recommend(U, V, 5, users=users, allow=allow, candidates=csr_of(rows)), False)
    assert lines("b.txt")[1] == "1"                        # the empty row: the user id alone


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_sampled_negatives_end_to_end():
    """One held-out item against 99 sampled unrated items per user: recommend(candidates=) and the existing evaluate_lists()
    give the hit rate and NDCG@10 numpy computes from the same (exact, integer) scores."""
    import primalcr_amd as pcr
    rng = np.random.default_rng(31)
    d1, d2, k = 200, 1500, 8
    U = rng.integers(-2, 3, (d1, k)).astype(np.float64)
    V = rng.integers(-2, 3, (d2, k)).astype(np.float64)
    index, item = special_csr(rng, d1, d2)
    M = excl_mask(d1, d2, index, item)
    users = np.array([u for u in range(d1) if (~M[u]).sum() >= 100], np.int32)     # (special_csr's user 5 has three unrated items)
    assert users.shape[0] == d1 - 1
    rows, held = [], []
    for u in users:
        pick = rng.choice(np.nonzero(~M[u])[0], 100, replace=False).astype(np.int32)
        held.append(pick[0])
        rows.append(rng.permutation(pick))
    held = np.array(held, np.int32)
    items, scores = pcr.recommend(U, V, 10, exclude=(index, item), users=users, candidates=csr_of(rows))
    tindex = np.zeros(d1 + 1, np.int64); tindex[users + 1] = 1; tindex = np.cumsum(tindex)
    res = pcr.evaluate_lists(items, V, d1=d1, users=users, test=(tindex, held, np.ones(held.shape[0])), cutoffs=(10,))
    S = U[users] @ V.T
    rank = np.array([int(((S[i, r] > S[i, h]) | ((S[i, r] == S[i, h]) & (r < h))).sum()) for i, (r, h) in enumerate(zip(rows, held))])
    hit = rank < 10
    assert 0 < hit.sum() < users.shape[0]
    top = res["topn"][0]
    assert top["users"] == users.shape[0] and top["hits"] == int(hit.sum())
    assert top["hit_rate"] == pytest.approx(hit.mean(), rel=1e-12)
    assert top["ndcg"] == pytest.approx(np.where(hit, 1.0 / np.log2(rank + 2.0), 0.0).mean(), rel=1e-12)
    for i in np.nonzero(hit)[0][:20]:
        assert items[i, rank[i]] == held[i]
