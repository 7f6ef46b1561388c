"""Non-negative fold-in for CCDR1 -N 1 models (pcr_fold_in_nnls_model, pcr_fold_in_nnls; include/primalcr.h, "non-negative
fold-in"): header / API agreement, argument errors, the CLI's refusals and the fixtures' preconditions on
the CPU; on the GPU every fixture user against tests/nnls_ref.py (the header's pivoting rule around np.linalg.solve), an exact
case on dyadic inputs, the ridge entry, the two forms against each other, determinism, singular systems, the solver entry, a
training user of a -N 1 model, recommend_new_users_nnls and the CLI.

The reference certifies itself: test_fixture_preconditions holds every reference row to a KKT residual of 1e-12 |b| with
min u >= 0, every system to a condition number of 1e4 (so the reference's own error is about 1e4 x 2^-53 = 1e-12 relative, far
inside the row bounds), and every user to a complementarity margin of 1e-8 -- min over P of u_j / max |u| and over Z of y_j / |b|
-- which makes the zero pattern of a row well defined at the accuracy of either form.  Bounds: FP64_ROW / FP32_ROW per row and
1e-9 / 1e-5 relative on loss and obj, the project's own (tests/test_foldin_ridge.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import nnls_ref as nr
import primalcr_amd as pcr
import ridge_ref as rr
from conftest import BIN_DIR, ROOT
from primalcr_amd import synth

RECOMMEND = os.path.join(BIN_DIR, "omp-pmf-recommend")
ERR_ARG, ERR_DEVICE = -1, -4
D2 = 3000
RANKS = [1, 3, 4, 16, 17, 100, 112, 116, 200]      # one tile, the 64 / 256-thread edge, the last direct rank, the first CG ranks
FIXED = [0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 300, 2049]      # tests/test_foldin_ridge.py's FIXED
LAM = 0.05
KINDS = ["gauss", "abs"]                           # F ~ N(0, 1) / sqrt(k), and |F|
PREC = {"F64": pcr.PCR_F64, "F32": pcr.PCR_F32}
FP64_ROW, FP32_ROW = 1e-7, 5e-3
OBJ_TOL = {"F64": 1e-9, "F32": 1e-5}
COND_MAX, KKT_MAX, MARGIN_MIN, PIVOTS_MAX = 1e4, 1e-12, 1e-8, 16


def lengths(k):
    extra = {k - 1, k, k + 1, 111, 112, 113}
    return FIXED + sorted(x for x in extra - set(FIXED) if x >= 0)


_F, _X, _REF = {}, {}, {}


def factors(kind, k):
    if (kind, k) not in _F:
        G = np.random.default_rng(5).normal(size=(D2, k)) / np.sqrt(k)
        _F[(kind, k)] = np.abs(G) if kind == "abs" else G
    return _F[(kind, k)]


def users_of(k):
    if k not in _X:
        _X[k] = rr.make_users(D2, lengths(k), 11)
    return _X[k]


def reference(kind, k, pname, weighted):
    key = (kind, k, pname, weighted)
    if key not in _REF:
        idx, it, val = users_of(k)
        _REF[key] = nr.fold_in(factors(kind, k), idx, it, val, LAM, weighted=weighted, f32=pname == "F32")
    return _REF[key]


def row_err(U, Uref):
    return np.abs(U - Uref).max(axis=1) / np.maximum(1.0, np.abs(Uref).max(axis=1))


def rel(a, b):
    return np.abs(a - b) / np.where(b == 0.0, 1.0, np.abs(b))


def run(cmd, cwd):
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True)


def sub_csr(X, users):
    idx, it, val = X
    rows = [(it[idx[u]:idx[u + 1]], val[idx[u]:idx[u + 1]]) for u in users]
    nidx = np.concatenate([[0], np.cumsum([len(a) for a, _ in rows])]).astype(np.int64)
    return nidx, np.concatenate([a for a, _ in rows]).astype(np.int32), np.concatenate([b for _, b in rows])


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


# ------------------------------------------------------------------------------------------------------------------------------
# CPU part
# ------------------------------------------------------------------------------------------------------------------------------

def test_header_and_api_agree():
    L = pcr.lib()
    assert hasattr(L, "pcr_fold_in_nnls_model") and hasattr(L, "pcr_fold_in_nnls")
    hdr = open(os.path.join(ROOT, "include", "primalcr.h")).read()
    for name, val in (("PCR_NNLS_FIELDS", len(pcr.PCR_NNLS_FIELDS)), ("PCR_NNLS_DIRECT", pcr.PCR_NNLS_DIRECT), ("PCR_NNLS_CG", pcr.PCR_NNLS_CG),
                      ("PCR_NNLS_OK", pcr.PCR_NNLS_OK), ("PCR_NNLS_SINGULAR", pcr.PCR_NNLS_SINGULAR), ("PCR_NNLS_CAP", pcr.PCR_NNLS_CAP),
                      ("PCR_NNLS_PIVOT_CAP", pcr.PCR_NNLS_PIVOT_CAP)):
        assert f"#define {name} " in hdr and int(hdr.split(f"#define {name} ")[1].split()[0]) == val, name
    assert (pcr.PCR_NNLS_DIRECT, pcr.PCR_NNLS_CG) == (0, 1) == (nr.DIRECT, nr.CG)
    assert (pcr.PCR_NNLS_OK, pcr.PCR_NNLS_SINGULAR, pcr.PCR_NNLS_CAP) == (0, 1, 2) == (nr.OK, nr.SINGULAR, nr.CAP)
    assert pcr.PCR_NNLS_PIVOT_CAP == 64 == nr.PIVOT_CAP
    assert pcr.PCR_NNLS_FIELDS == ("n", "form", "pivots", "zeros", "loss", "obj", "status")
    struct = hdr.split("typedef struct pcr_nnls_stats {")[1].split("}")[0]
    names = [w.strip() for part in struct.replace("int64_t", "").replace("double", "").split(";") for w in part.split(",") if w.strip()]
    assert names == [f for f, _ in pcr.NnlsStats._fields_] == ["users", "direct", "cg", "singular", "cap", "pivots", "zeros", "loss", "obj"]
    assert C.sizeof(pcr.NnlsStats) == 72
    # the rule: a function of k alone -- direct while the padded rank fits PCR_RIDGE_DIRECT_MAX
    for k, f in ((1, 0), (16, 0), (17, 0), (100, 0), (112, 0), (113, 1), (116, 1), (200, 1)):
        assert pcr.nnls_form(k) == f == nr.form(k), k


def test_argument_errors_come_before_any_device_and_name_the_entry():
    F = factors("gauss", 3)
    idx, it, val = np.array([0, 2, 3], np.int64), np.array([5, 1, 7], np.int32), np.array([1.0, 2.0, 3.0])

    def refused(match, **kw):
        a = dict(F=F, ratings=(idx, it, val), lam=1.0)
        a.update(kw)
        with pytest.raises(pcr.PcrError, match=match) as e:
            pcr.fold_in_nnls(**a)
        assert f"error {ERR_ARG}:" in str(e.value) and "pcr_fold_in_nnls_model" in str(e.value), str(e.value)

    refused("outside", ratings=(idx, np.array([5, 1, D2], np.int32), val))
    refused("outside", ratings=(idx, np.array([5, -1, 7], np.int32), val))
    refused("not finite", ratings=(idx, it, np.array([1.0, np.nan, 3.0])))
    refused("not finite", ratings=(idx, it, np.array([1.0, np.inf, 3.0])))
    refused("monotone", ratings=(np.array([0, 3, 2, 3], np.int64), it, val))
    refused(r"index\[0\]", ratings=(np.array([1, 2, 3], np.int64), it, val))
    refused("lambda", lam=-1.0)
    refused("lambda", lam=float("nan"))
    refused("lambda", lam=float("inf"))
    refused("precision", dtype=7)
    L = pcr.lib()
    out = np.zeros((2, 3))
    args = lambda Fp, rows, k, outp: (Fp, rows, k, 1.0, 1, pcr.PCR_F64, 0, 2, idx.ctypes.data, it.ctypes.data, val.ctypes.data, outp, None, None)
    for bad in (args(None, D2, 3, out.ctypes.data), args(F.ctypes.data, D2, 3, None), args(F.ctypes.data, D2, 0, out.ctypes.data),
                args(F.ctypes.data, 0, 3, out.ctypes.data)):
        assert L.pcr_fold_in_nnls_model(*bad) == ERR_ARG
        assert b"pcr_fold_in_nnls_model" in L.pcr_last_error()
    assert L.pcr_fold_in_nnls(None, 1, 2, idx.ctypes.data, it.ctypes.data, val.ctypes.data, out.ctypes.data, None, None) == ERR_ARG
    with pcr.tuned(nnls_form="cg"):                                # the knob exists; an unknown one is refused
        pass
    with pytest.raises(pcr.PcrError):
        pcr.tune("nnls_shape", "cg")


def test_without_a_device_the_call_fails_with_err_device():
    """Valid arguments on a process that sees no GPU: PCR_ERR_DEVICE (never a CPU path)."""
    code = ("import sys, numpy as np; sys.path.insert(0, sys.argv[1])\n"
            "import primalcr_amd as pcr\n"
            "try:\n"
            "    pcr.fold_in_nnls(np.ones((6, 3)), (np.array([0, 2, 2]), np.array([1, 4]), np.array([1.0, 2.0])), 1.0)\n"
            "    print('no error')\n"
            "except pcr.PcrError as e:\n"
            "    print(str(e))\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    assert f"error {ERR_DEVICE}:" in out.stdout, out.stdout


def test_cli_usage_and_refusals(tmp_path):
    r = run([RECOMMEND], tmp_path)
    assert r.returncode == 1 and r.stdout.startswith("Usage: omp-pmf-recommend [-K topk] [-x data_dir] [-u users_file] [--f32] [--scores]")
    assert "omp-pmf-recommend --fold-in-nnls data_dir -l lambda [--plain-reg] [-K topk] [--f32] [--scores] model_file output_file\n" in r.stdout
    assert "omp-pmf-recommend --fold-in-nnls data_dir -l lambda [--plain-reg] --eval data_dir [-c ...] [--threshold v] [--f32] model_file [output_file]\n" in r.stdout
    assert "foldin_nnls users n direct n cg n singular n cap n pivots n zeros n loss x obj x" in r.stdout
    # the existing lines, unchanged
    assert "omp-pmf-recommend --fold-in-ridge data_dir -l lambda [--plain-reg] [-K topk] [--f32] [--scores] model_file output_file\n" in r.stdout
    assert "    -l lambda      the regulariser of the model (required with --fold-in)\n" in r.stdout
    (tmp_path / "users").write_text("1\n")
    for extra in (["-x", "d"], ["-u", "users"], ["--diversity"], ["--mmr", "0.5"], ["--tradeoff", "0,1"], ["--eval", "d", "--ranks"]):
        r = run([RECOMMEND, "--fold-in-nnls", "d", "-l", "1"] + extra + ["m", "o"], tmp_path)
        assert r.returncode == 1 and "--fold-in-nnls does not go with" in r.stderr, (extra, r.stderr)
    for extra in (["--allow", "users"], ["--candidates", "users"], ["--fold-in", "d"], ["--fold-in-ridge", "d"], ["-s", "2"], ["--steps", "3"]):
        r = run([RECOMMEND, "--fold-in-nnls", "d", "-l", "1"] + extra + ["m", "o"], tmp_path)
        assert r.returncode == 1 and "--fold-in-nnls" in r.stderr, (extra, r.stderr)
    r = run([RECOMMEND, "--fold-in-ridge", "d", "--fold-in-nnls", "d", "-l", "1", "m", "o"], tmp_path)       # either order
    assert r.returncode == 1 and "--fold-in-nnls does not go with --fold-in-ridge" in r.stderr
    r = run([RECOMMEND, "--fold-in-nnls", "d", "m", "o"], tmp_path)
    assert r.returncode == 1 and "--fold-in-nnls needs -l" in r.stderr
    r = run([RECOMMEND, "--fold-in-nnls", "d", "-l", "-1", "m", "o"], tmp_path)
    assert r.returncode == 1 and "-l" in r.stderr
    r = run([RECOMMEND, "--plain-reg", "m", "o"], tmp_path)                                    # neither option: the existing message
    assert r.returncode == 1 and "--plain-reg goes with --fold-in-ridge" in r.stderr
    R = synth.generate("tiny", seed=3)                              # 60 x 40
    d = synth.write_dir(R, str(tmp_path / "data"))
    rng = np.random.default_rng(2)
    pcr.model_save(str(tmp_path / "wrong.model"), rng.standard_normal((5, 4)), rng.standard_normal((R.d2 + 1, 4)))
    r = run([RECOMMEND, "--fold-in-nnls", d, "-l", "1", "wrong.model", "out"], tmp_path)
    assert r.returncode == 1 and "items, the model" in r.stderr, r.stderr


@pytest.mark.parametrize("k", RANKS)
@pytest.mark.parametrize("kind", KINDS)
def test_fixture_preconditions(kind, k):
    """From the reference alone, for both regularisers and both storage types: the lengths the issue lists, a KKT residual
    <= 1e-12 |b| with min u >= 0 for every reference row, condition numbers <= 1e4, at most 16 pivots (a quarter of the cap) and a
    complementarity margin >= 1e-8."""
    idx, it, val = users_of(k)
    lens = np.diff(idx)
    assert list(lens) == lengths(k) and set(FIXED) | {k - 1, k, k + 1, 111, 112, 113} == set(lens)
    assert val.min() >= 1.0 and val.max() <= 5.0
    for weighted in (True, False):
        for pname in PREC:
            ref = reference(kind, k, pname, weighted)
            live = lens > 0
            print(f"{kind} k={k} {pname} weighted={weighted}: kkt {ref['kkt'].max():.3g} cond {ref['cond'].max():.3g} "
                  f"pivots {ref['pivots'].max()} margin {ref['margin'][live].min():.3g}")
            assert np.all(ref["status"] == nr.OK)
            assert ref["kkt"].max() <= KKT_MAX, (weighted, pname, int(ref["kkt"].argmax()), ref["kkt"].max())
            assert ref["rows"].min() >= 0.0
            assert ref["cond"].max() <= COND_MAX, (weighted, pname, int(ref["cond"].argmax()), ref["cond"].max())
            assert ref["pivots"].max() <= PIVOTS_MAX and PIVOTS_MAX * 4 == pcr.PCR_NNLS_PIVOT_CAP
            assert ref["margin"][live].min() >= MARGIN_MIN, (weighted, pname, int(ref["margin"].argmin()), ref["margin"].min())
            assert np.array_equal(ref["rows"][live] > 0.0, ref["passive"][live])               # (the margin, seen in the rounded rows)


# ------------------------------------------------------------------------------------------------------------------------------
# GPU part
# ------------------------------------------------------------------------------------------------------------------------------

def check_against_reference(kind, k, pname, weighted, U, pu, pivots=False):
    ref = reference(kind, k, pname, weighted)
    lens = np.diff(users_of(k)[0])
    assert U.min() >= 0.0                                                                       # exactly
    assert np.array_equal(U > 0.0, ref["rows"] > 0.0), np.flatnonzero(((U > 0.0) != (ref["rows"] > 0.0)).any(axis=1))
    assert np.array_equal((U[lens > 0] > 0.0), ref["passive"][lens > 0])
    e = row_err(U, ref["rows"])
    el, eo = rel(pu[:, 4], ref["loss"]), rel(pu[:, 5], ref["obj"])
    print(f"{kind} k={k} {pname} weighted={weighted}: row {e.max():.3g} loss {el.max():.3g} obj {eo.max():.3g} pivots {int(pu[:, 2].max())}")
    assert e.max() <= (FP64_ROW if pname == "F64" else FP32_ROW), (int(e.argmax()), e.max())
    assert el.max() <= OBJ_TOL[pname], (int(el.argmax()), el.max())
    assert eo.max() <= OBJ_TOL[pname], (int(eo.argmax()), eo.max())
    assert np.array_equal(pu[:, 0], lens.astype(np.float64))
    assert np.array_equal(pu[:, 3], (U == 0.0).sum(axis=1).astype(np.float64))
    assert np.all(pu[:, 6] == pcr.PCR_NNLS_OK), pu[:, 6]
    if pivots:
        assert np.array_equal(pu[:, 2], ref["pivots"].astype(np.float64)), (pu[:, 2], ref["pivots"])


@pytest.mark.gpu
@pytest.mark.parametrize("weighted", [True, False], ids=["weighted", "plain"])
@pytest.mark.parametrize("pname", ["F64", "F32"])
@pytest.mark.parametrize("k", RANKS)
@pytest.mark.parametrize("kind", KINDS)
def test_rows_and_sets_against_the_reference(kind, k, pname, weighted):
    U, st, pu = pcr.fold_in_nnls(factors(kind, k), users_of(k), LAM, weighted=weighted, dtype=PREC[pname], per_user=True)
    form = pcr.nnls_form(k)
    check_against_reference(kind, k, pname, weighted, U, pu, pivots=form == pcr.PCR_NNLS_DIRECT and pname == "F64")
    n = len(lengths(k))
    assert np.all(pu[:, 1] == form)
    assert st["users"] == n and st["direct"] == (n if form == pcr.PCR_NNLS_DIRECT else 0) and st["cg"] == n - st["direct"]
    assert st["singular"] == 0 and st["cap"] == 0 and st["pivots"] == int(pu[:, 2].sum()) and st["zeros"] == int(pu[:, 3].sum())
    assert st["loss"] == float(np.cumsum(pu[:, 4])[-1]) and st["obj"] == float(np.cumsum(pu[:, 5])[-1])
    assert np.all(U[0] == 0.0) and list(pu[0]) == [0.0, form, 0.0, k, 0.0, 0.0, pcr.PCR_NNLS_OK]       # the user without ratings
    assert np.all(pu[1:, 2] >= 1)


def dyadic_case(k, seed):
    """Row i of F is e_(i mod k).  A user rates each of its columns c times (c = 3 or 15, ONE value per user) with non-zero
    integers of both signs, so with plain lambda = 1: G is diagonal, G_jj = 4 or 16 on its columns and 1 elsewhere, b_j a small
    integer.  Every quantity of either form is then a small dyadic rational: the direct form factors a diagonal of squares of
    powers of two; the CG form sees G = (c + 1) I on the support of b and stops after one exact step with step size 1 / (c + 1)."""
    rng = np.random.default_rng(seed)
    rows = 15 * k
    F = np.zeros((rows, k))
    F[np.arange(rows), np.arange(rows) % k] = 1.0
    index, items, vals = [0], [], []
    for u in range(24):
        c = 3 if u % 2 == 0 else 15
        cols = np.flatnonzero(rng.random(k) < 0.6) if u % 3 else np.arange(k)
        if cols.size == 0:
            cols = np.array([0])
        it = np.sort(np.concatenate([cols + k * j for j in range(c)])).astype(np.int32)
        v = rng.integers(1, 6, size=it.size).astype(np.float64)
        if u % 4:                                                   # (every fourth user: no negative rating, so no b_j < 0)
            v *= rng.choice([-1.0, 1.0], size=it.size)
        items.append(it); vals.append(v)
        index.append(index[-1] + it.size)
    return F, (np.array(index, np.int64), np.concatenate(items), np.concatenate(vals))


@pytest.mark.gpu
@pytest.mark.parametrize("pname", ["F64", "F32"])
@pytest.mark.parametrize("k", [16, 100, 116])
def test_exact_on_dyadic_input(k, pname):
    F, X = dyadic_case(k, 7 + k)
    idx, it, val = X
    U, st, pu = pcr.fold_in_nnls(F, X, 1.0, weighted=False, dtype=PREC[pname], per_user=True)
    assert np.all(pu[:, 1] == pcr.nnls_form(k)) and st["singular"] == 0 and st["cap"] == 0
    seen = set()
    for u in range(len(idx) - 1):
        A, r = F[it[idx[u]:idx[u + 1]]], val[idx[u]:idx[u + 1]]
        b, g = A.T @ r, (A * A).sum(axis=0) + 1.0
        assert set(g) <= {1.0, 4.0, 16.0}
        want = np.maximum(0.0, b / g)
        assert same_bits(U[u], want), (u, U[u], want)
        assert pu[u, 2] == (2 if (b < 0).any() else 1), (u, pu[u, 2])
        seen.add(int(pu[u, 2]))
    assert seen == {1, 2}


@pytest.mark.gpu
def test_a_positive_ridge_row_is_returned_bit_for_bit():
    """A user with n > k (the ridge entry's primal form) whose ridge row is entrywise positive: pivot 1 is that solve, on the same
    Gram build, factorisation and solves -- the same bits, 1 pivot.  The |F|, k = 16, weighted fixture has twelve users with
    n > k; the ridge row of eight of them is entrywise positive (tests/ridge_ref.py agrees: the other four have an entry below
    -0.05), and every one of the eight is compared."""
    k = 16
    F, X = factors("abs", k), users_of(k)
    lens = np.diff(X[0])
    Ur, _, pr = pcr.fold_in_ridge(F, X, LAM, weighted=True, per_user=True)
    Un, _, pn = pcr.fold_in_nnls(F, X, LAM, weighted=True, per_user=True)
    pick = np.flatnonzero((lens > k) & (pr[:, 1] == pcr.PCR_RIDGE_PRIMAL) & (Ur > 0.0).all(axis=1))
    want = np.flatnonzero((lens > k) & (rr.fold_in(F, *X, LAM, weighted=True)[0] > 0.0).all(axis=1))
    assert list(pick) == list(want) and len(pick) == 8, (pick, want)
    for u in pick:
        assert same_bits(Un[u], Ur[u]) and pn[u, 2] == 1 and pn[u, 3] == 0, u
        # loss and obj: the same row, but the ridge entry adds a long user's n <= 2049 non-negative terms on 256 threads and this
        # one on 64 -- another order, at most n x 2^-53 = 2.3e-13 relative apart
        assert rel(pn[u, 4:6], pr[u, 3:5]).max() <= 1e-12, (u, pn[u, 4:6], pr[u, 3:5])


@pytest.mark.gpu
@pytest.mark.parametrize("weighted", [True, False], ids=["weighted", "plain"])
@pytest.mark.parametrize("k", RANKS)
@pytest.mark.parametrize("kind", KINDS)
def test_objective_between_the_ridge_entry_and_the_zero_row(kind, k, weighted):
    """The unconstrained minimum is a lower bound, the feasible row u = 0 (obj = |r|^2) an upper one, for every user."""
    F, X = factors(kind, k), users_of(k)
    _, _, pr = pcr.fold_in_ridge(F, X, LAM, weighted=weighted, per_user=True)
    _, _, pn = pcr.fold_in_nnls(F, X, LAM, weighted=weighted, per_user=True)
    r2 = np.array([float(X[2][X[0][u]:X[0][u + 1]] @ X[2][X[0][u]:X[0][u + 1]]) for u in range(len(X[0]) - 1)])
    assert np.all(pn[:, 5] >= pr[:, 4] - 1e-9 * pn[:, 5]), np.flatnonzero(pn[:, 5] < pr[:, 4] - 1e-9 * pn[:, 5])
    assert np.all(pn[:, 5] <= r2), np.flatnonzero(pn[:, 5] > r2)


@pytest.mark.gpu
@pytest.mark.parametrize("weighted", [True, False], ids=["weighted", "plain"])
@pytest.mark.parametrize("k", [x for x in RANKS if x <= 112])
@pytest.mark.parametrize("kind", KINDS)
def test_forms_agree(kind, k, weighted):
    """pcr_tune nnls_form=cg at a direct rank: every user takes the CG form, lands on the same zero pattern and within FP64_ROW."""
    F, X = factors(kind, k), users_of(k)
    with pcr.tuned(nnls_form="cg"):
        U, st, pu = pcr.fold_in_nnls(F, X, LAM, weighted=weighted, per_user=True)
    assert np.all(pu[:, 1] == pcr.PCR_NNLS_CG) and st["cg"] == st["users"] and st["direct"] == 0
    check_against_reference(kind, k, "F64", weighted, U, pu)
    with pcr.tuned(nnls_form="auto"):
        U2, st2, pu2 = pcr.fold_in_nnls(F, X, LAM, weighted=weighted, per_user=True)
    assert np.all(pu2[:, 1] == pcr.PCR_NNLS_DIRECT) and st2["direct"] == st2["users"]
    assert np.array_equal(U > 0.0, U2 > 0.0)
    e = row_err(U, U2)
    assert e.max() <= FP64_ROW, (int(e.argmax()), e.max())


@pytest.mark.gpu
@pytest.mark.parametrize("pname", ["F64", "F32"])
@pytest.mark.parametrize("k", [17, 100, 116])
def test_determinism_and_independence(k, pname):
    """A user's row and table line are the same bits across two identical calls, in a permuted batch, with the batch split in two
    and alone in a call (the launch's grid and every other user change)."""
    F = factors("abs", k)
    rng = np.random.default_rng(3)
    pool = np.array([n for n in lengths(k) if n <= 400])
    N = 300
    X = rr.make_users(D2, list(rng.choice(pool, size=N)), 23)
    call = lambda Y: pcr.fold_in_nnls(F, Y, LAM, weighted=False, dtype=PREC[pname], per_user=True)
    Ua, sa, pa = call(X)
    Ub, sb, pb = call(X)
    assert same_bits(Ua, Ub) and same_bits(pa, pb) and sa == sb
    assert pa[:, 2].max() >= 2                                         # (the batch does pivot)
    perm = rng.permutation(N)
    Up, _, pp = call(sub_csr(X, perm))
    assert same_bits(Up, Ua[perm]) and same_bits(pp, pa[perm])
    for part in (np.arange(0, N // 2), np.arange(N // 2, N)):
        Uh, _, ph = call(sub_csr(X, part))
        assert same_bits(Uh, Ua[part]) and same_bits(ph, pa[part])
    lens = np.diff(X[0])
    for u in {int(perm[0]), int(perm[-1]), int(lens.argmax()), int(pa[:, 2].argmax())}:
        U1, _, p1 = call(sub_csr(X, [u]))
        assert same_bits(U1[0], Ua[u]) and same_bits(p1[0], pa[u]), u


@pytest.mark.gpu
@pytest.mark.parametrize("pname", ["F64", "F32"])
def test_singular_systems_are_reported(pname):
    """lambda = 0 and a column nobody rated (rows (2, 0, ...)): the direct form meets a zero pivot -- SINGULAR, a zero row and
    loss = obj = |r|^2."""
    for k in (2, 5):
        F = np.zeros((10, k)); F[:, 0] = 2.0
        idx = np.array([0, 2, 5], np.int64)
        it = np.array([4, 4, 1, 2, 3], np.int32)
        val = np.array([1.0, 3.0, 1.0, 2.0, 4.0])
        U, st, pu = pcr.fold_in_nnls(F, (idx, it, val), 0.0, dtype=PREC[pname], per_user=True)
        assert np.all(pu[:, 1] == pcr.PCR_NNLS_DIRECT) and np.all(pu[:, 6] == pcr.PCR_NNLS_SINGULAR) and np.all(U == 0.0)
        assert list(pu[:, 4]) == [10.0, 21.0] == list(pu[:, 5]) and list(pu[:, 3]) == [k, k]
        assert st["singular"] == 2 and st["cap"] == 0 and st["zeros"] == 2 * k


def _small():
    R = synth.generate("small", seed=31, d1=300, d2=400, nnz=300 * 40)
    return R, pcr.Dataset.from_ratings(R)


def _nmf_solver(ds, R, k, lam, prec):
    s = pcr.Solver(ds, pcr.Parameter(k=k, precision=prec, solver_type=pcr.PCR_SOLVER_CCDR1, **{"lambda": lam}))
    s.set_ccd_params(do_nmf=1)
    s.set_factors(np.abs(pcr.initial_col(R.d1, k)), None)
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("pname", ["F64", "F32"])
def test_solver_entry_on_a_nmf_ccdr1_and_on_a_primalcr_solver(pname):
    """Solver.fold_in_nnls on a CCDR1 -N 1 solver and on a PrimalCR++ solver holding the same V equal fold_in_nnls(V, ...) bit for
    bit; the profile slot foldin/nnls is filled; the solver is left as a twin that never folded anything in."""
    R, ds = _small()
    k, lam = 8, 0.05
    idx, it, val = users_of(17)
    sub = (idx, it % R.d2, val)                                        # (duplicated items: two ratings each)
    a, b = _nmf_solver(ds, R, k, lam, PREC[pname]), _nmf_solver(ds, R, k, lam, PREC[pname])
    for s in (a, b):
        s.iterate(2)
    U, V = a.get_factors()
    assert U.min() >= 0.0 and V.min() >= 0.0
    mis = a.counter("ccd_residual_mismatch")
    a.profile(True)
    for weighted in (True, False):
        a.profile_reset()
        Us, ss, ps = a.fold_in_nnls(sub, weighted=weighted, per_user=True)
        assert a.profile_get("foldin/nnls")[1] >= 1 and "foldin/nnls" in a.profile_all()
        Um, sm, pm = pcr.fold_in_nnls(V, sub, lam, weighted=weighted, dtype=PREC[pname], per_user=True)
        assert same_bits(Us, Um) and same_bits(ps, pm) and ss == sm
        assert Us.min() >= 0.0 and ss["singular"] == 0 and ss["cap"] == 0
    a.profile(False)
    c = pcr.Solver(ds, pcr.Parameter(k=k, precision=PREC[pname], solver_type=pcr.PCR_SOLVER_PCRPP, **{"lambda": lam}))
    c.set_factors(U, V)
    Uc, sc, pc = c.fold_in_nnls(sub, per_user=True)
    Um, sm, pm = pcr.fold_in_nnls(V, sub, lam, dtype=PREC[pname], per_user=True)
    assert same_bits(Uc, Um) and same_bits(pc, pm) and sc == sm
    Uc2, Vc2 = c.get_factors()
    assert np.array_equal(Uc2, U) and np.array_equal(Vc2, V)
    c.close()
    assert a.counter("ccd_residual_mismatch") == mis == b.counter("ccd_residual_mismatch")
    assert all(np.array_equal(x, y) for x, y in zip(a.get_factors(), b.get_factors()))
    ra, rb = a.iterate(1), b.iterate(1)
    key = ("obj", "cg_v", "cg_u")
    assert [[x[f] for f in key] for x in ra] == [[x[f] for f in key] for x in rb]
    assert all(np.array_equal(x, y) for x, y in zip(a.get_factors(), b.get_factors()))
    a.close(); b.close()


@pytest.mark.gpu
def test_a_training_user_of_a_nmf_model():
    """Train -N 1 for a few outer iterations in fp64 and fold the training users back in with the training lambda, weighted: the
    trained row U[u] is feasible and the fold-in is the minimiser over the feasible set, so obj_nnls <= obj(U[u]) (relative 1e-9)."""
    R, ds = _small()
    k, lam = 8, 0.05
    s = _nmf_solver(ds, R, k, lam, pcr.PCR_F64)
    s.iterate(3)
    U, V = s.get_factors()
    s.close()
    assert U.min() >= 0.0 and V.min() >= 0.0
    idx, it, val = ds.csr(0)
    it = it.astype(np.int32)
    New, st, pu = pcr.fold_in_nnls(V, (idx, it, val), lam, weighted=True, per_user=True)
    assert st["singular"] == 0 and st["cap"] == 0 and New.min() >= 0.0
    for i in range(len(idx) - 1):
        A, r = V[it[idx[i]:idx[i + 1]]], val[idx[i]:idx[i + 1]]
        mu = lam * len(r)
        o_tr = rr.loss_obj(A, r, mu, U[i])[1]
        o_new = rr.loss_obj(A, r, mu, New[i])[1]
        assert o_new <= o_tr * (1 + 1e-9), (i, o_new, o_tr)
        assert abs(pu[i, 5] - o_new) <= 1e-9 * max(1.0, o_new)


@pytest.mark.gpu
def test_end_to_end(tmp_path):
    """recommend_new_users_nnls is fold_in_nnls + recommend(exclude=...) bit for bit; the CLI's --fold-in-nnls output file and
    summary line agree with the Python calls; --eval prints the top-N block."""
    R, ds = _small()
    d = synth.write_dir(R, str(tmp_path / "data"))
    k, lam = 8, 0.05
    rng = np.random.default_rng(4)
    U, V = np.abs(rng.normal(size=(R.d1, k))) / np.sqrt(k), np.abs(rng.normal(size=(R.d2, k))) / np.sqrt(k)
    pcr.model_save(str(tmp_path / "m.model"), U, V)
    for plain in (False, True):
        Un, stats = pcr.fold_in_nnls(V, ds, lam, weighted=not plain)
        items, scores, U2, st2 = pcr.recommend_new_users_nnls(V, ds, lam, 10, weighted=not plain)
        ri, rs = pcr.recommend(Un, V, 10, exclude=ds)
        assert np.array_equal(U2, Un) and st2 == stats and np.array_equal(items, ri) and np.array_equal(scores, rs)
        assert Un.min() >= 0.0
        flag = ["--plain-reg"] if plain else []
        r = run([RECOMMEND, "--fold-in-nnls", d, "-l", str(lam)] + flag + ["m.model", "lists.txt"], tmp_path)
        assert r.returncode == 0, r.stderr
        want = ("foldin_nnls users %d direct %d cg %d singular %d cap %d pivots %d zeros %d loss %s obj %s" %
                (stats["users"], stats["direct"], stats["cg"], stats["singular"], stats["cap"], stats["pivots"], stats["zeros"],
                 "%g" % stats["loss"], "%g" % stats["obj"]))
        assert r.stdout.splitlines() == [want]
        lines = open(tmp_path / "lists.txt").read().splitlines()
        assert lines == [" ".join([str(u + 1)] + [str(j + 1) for j in row if j >= 0]) for u, row in enumerate(ri)]
    r = run([RECOMMEND, "--fold-in-nnls", d, "-l", str(lam), "--plain-reg", "--eval", d, "-c", "5,10", "m.model"], tmp_path)
    assert r.returncode == 0, r.stderr
    ev = pcr.evaluate_topn(Un, V, ds, cutoffs=(5, 10), exclude=ds)
    out = r.stdout.splitlines()
    assert out[0] == want and len(out) == 3
    for line, e in zip(out[1:], ev):
        f = line.split()
        assert f[0] == "cutoff" and int(f[1]) == e["cutoff"] and int(f[3]) == e["users"] and int(f[7]) == e["hits"]
        assert f[9] == "%g" % e["precision"] and f[11] == "%g" % e["recall"] and f[17] == "%g" % e["ndcg"], (line, e)
