"""Squared-loss (ridge) fold-in for CCDR1 models (pcr_fold_in_ridge_model, pcr_fold_in_ridge; include/primalcr.h, "ridge
fold-in"): header / API agreement, argument errors and the CLI's refusals on the CPU; on the GPU the
length edges of every form against tests/ridge_ref.py (np.linalg.solve per user), the forms against each other, determinism,
the solver entry on a CCDR1 and on a PrimalCR++ solver, singular systems on dyadic inputs, CCDR1's own objective, and the CLI.

Inputs are well conditioned by construction (entries of F about N(0, 1) / sqrt(k), ratings in 1..5, mu >= 1e-2 mean |row|^2):
test_fixture_is_well_conditioned holds every system of the fixtures below a condition number of 1e4, so the reference's own
error (about 1e4 x 2^-53 = 1e-12 relative) sits far inside the bounds: FP64_ROW / FP32_ROW per row (the project's per-row bounds,
tests/test_foldin.py), 1e-9 / 1e-5 relative on loss and obj."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import primalcr_amd as pcr
import ridge_ref as rr
from conftest import BIN_DIR, ROOT
from primalcr_amd import synth

RECOMMEND = os.path.join(BIN_DIR, "omp-pmf-recommend")
ERR_ARG, ERR_DEVICE = -1, -4
D2 = 3000
RANKS = [1, 3, 4, 16, 17, 100, 112, 116]
FIXED = [0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 300, 2049]
LAM = 0.05                                 # mu = LAM n >= 0.05 (weighted) or 0.05 (plain); mean |row|^2 = 1
PREC = {"F64": pcr.PCR_F64, "F32": pcr.PCR_F32}
FP64_ROW, FP32_ROW = 1e-7, 5e-3            # the project's per-row bounds (tests/test_foldin.py)
OBJ_TOL = {"F64": 1e-9, "F32": 1e-5}
COND_MAX = 1e4
DUP_USER, DESC_USER = 6, 7                 # lengths()[6] = 15 ratings with one item twice, lengths()[7] = 16 given item-descending


def lengths(k):
    """The issue's fixed lengths, then each boundary of the form rule and +-1 of it, and k - 1, k, k + 1."""
    extra = set()
    for b in pcr.ridge_boundaries(k):
        extra |= {b - 1, b, b + 1}
    extra |= {k - 1, k, k + 1}
    return FIXED + sorted(x for x in extra - set(FIXED) if x >= 0)


_F, _X, _REF = {}, {}, {}


def factors(k):
    if k not in _F:
        _F[k] = np.random.default_rng(5).normal(size=(D2, k)) / np.sqrt(k)
    return _F[k]


def users_of(k):
    if k not in _X:
        _X[k] = rr.make_users(D2, lengths(k), 11, dup_user=DUP_USER, desc_user=DESC_USER)
    return _X[k]


def reference(k, pname, weighted):
    key = (k, pname, weighted)
    if key not in _REF:
        idx, it, val = users_of(k)
        _REF[key] = rr.fold_in(factors(k), idx, it, val, LAM, weighted=weighted, f32=pname == "F32")
    return _REF[key]


def row_err(U, Uref):
    return np.abs(U - Uref).max(axis=1) / np.maximum(1.0, np.abs(Uref).max(axis=1))


def rel(a, b):
    return np.abs(a - b) / np.where(b == 0.0, 1.0, np.abs(b))


def run(cmd, cwd):
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True)


# ------------------------------------------------------------------------------------------------------------------------------
# CPU part
# ------------------------------------------------------------------------------------------------------------------------------

def test_header_and_api_agree():
    L = pcr.lib()
    assert hasattr(L, "pcr_fold_in_ridge_model") and hasattr(L, "pcr_fold_in_ridge")
    hdr = open(os.path.join(ROOT, "include", "primalcr.h")).read()
    for name, val in (("PCR_RIDGE_FIELDS", len(pcr.PCR_RIDGE_FIELDS)), ("PCR_RIDGE_DUAL", pcr.PCR_RIDGE_DUAL),
                      ("PCR_RIDGE_PRIMAL", pcr.PCR_RIDGE_PRIMAL), ("PCR_RIDGE_CG", pcr.PCR_RIDGE_CG), ("PCR_RIDGE_OK", pcr.PCR_RIDGE_OK),
                      ("PCR_RIDGE_SINGULAR", pcr.PCR_RIDGE_SINGULAR), ("PCR_RIDGE_CG_CAP", pcr.PCR_RIDGE_CG_CAP),
                      ("PCR_RIDGE_WAVE_MAX", pcr.PCR_RIDGE_WAVE_MAX), ("PCR_RIDGE_DIRECT_MAX", pcr.PCR_RIDGE_DIRECT_MAX)):
        assert f"#define {name} " in hdr and int(hdr.split(f"#define {name} ")[1].split()[0]) == val, name
    assert (pcr.PCR_RIDGE_DUAL, pcr.PCR_RIDGE_PRIMAL, pcr.PCR_RIDGE_CG) == (0, 1, 2) == (rr.DUAL, rr.PRIMAL, rr.CG)
    assert (pcr.PCR_RIDGE_OK, pcr.PCR_RIDGE_SINGULAR, pcr.PCR_RIDGE_CG_CAP) == (0, 1, 2)
    assert (pcr.PCR_RIDGE_WAVE_MAX, pcr.PCR_RIDGE_DIRECT_MAX) == (64, 112) == (rr.WAVE_MAX, rr.DIRECT_MAX)
    assert pcr.PCR_RIDGE_FIELDS == ("n", "form", "iters", "loss", "obj", "status")
    struct = hdr.split("typedef struct pcr_ridge_stats {")[1].split("}")[0]
    names = [w.strip() for part in struct.replace("int64_t", "").replace("double", "").split(";") for w in part.split(",") if w.strip()]
    assert names == [f for f, _ in pcr.RidgeStats._fields_] == ["users", "dual", "primal", "cg", "singular", "cg_cap", "iters", "loss", "obj"]
    assert C.sizeof(pcr.RidgeStats) == 72
    # the rule: dual up to min(k, DIRECT_MAX); above it primal while the padded rank fits, else CG
    assert pcr.ridge_boundaries(8) == [8] and pcr.ridge_boundaries(100) == [100] and pcr.ridge_boundaries(112) == [112]
    assert pcr.ridge_boundaries(116) == [112] and pcr.ridge_boundaries(200) == [112]
    for k, n, f in ((8, 8, 0), (8, 9, 1), (100, 100, 0), (100, 101, 1), (112, 113, 1), (116, 112, 0), (116, 113, 2), (116, 5000, 2),
                    (200, 20, 0), (200, 112, 0), (200, 113, 2), (100, 100000, 1), (1, 0, 0), (1, 2, 1)):
        assert pcr.ridge_form(n, k) == f == rr.form(n, k), (k, n)


def test_argument_errors_come_before_any_device_and_name_the_entry():
    F = factors(3)
    idx, it, val = np.array([0, 2, 3], np.int64), np.array([5, 1, 7], np.int32), np.array([1.0, 2.0, 3.0])

    def refused(match, **kw):
        a = dict(F=F, ratings=(idx, it, val), lam=1.0)
        a.update(kw)
        with pytest.raises(pcr.PcrError, match=match) as e:
            pcr.fold_in_ridge(**a)
        assert f"error {ERR_ARG}:" in str(e.value) and "pcr_fold_in_ridge_model" in str(e.value), str(e.value)

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
        assert L.pcr_fold_in_ridge_model(*bad) == ERR_ARG
        assert b"pcr_fold_in_ridge_model" in L.pcr_last_error()
    assert L.pcr_fold_in_ridge(None, 1, 2, idx.ctypes.data, it.ctypes.data, val.ctypes.data, out.ctypes.data, None, None) == ERR_ARG
    with pcr.tuned(ridge_form="cg"):                               # the knob exists; an unknown one is refused
        pass
    with pytest.raises(pcr.PcrError):
        pcr.tune("ridge_shape", "cg")


def test_without_a_device_the_call_fails_with_err_device():
    """Valid arguments on a process that sees no GPU: PCR_ERR_DEVICE (never a CPU path)."""
    code = ("import sys, numpy as np; sys.path.insert(0, sys.argv[1])\n"
            "import primalcr_amd as pcr\n"
            "try:\n"
            "    pcr.fold_in_ridge(np.ones((6, 3)), (np.array([0, 2, 2]), np.array([1, 4]), np.array([1.0, 2.0])), 1.0)\n"
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
    assert "omp-pmf-recommend --fold-in-ridge data_dir -l lambda [--plain-reg] [-K topk] [--f32] [--scores] model_file output_file\n" in r.stdout
    assert "omp-pmf-recommend --fold-in-ridge data_dir -l lambda [--plain-reg] --eval data_dir [-c ...] [--threshold v] [--f32] model_file [output_file]\n" in r.stdout
    # the existing lines, unchanged
    assert "omp-pmf-recommend --fold-in data_dir -l lambda [-s 1|2] [--steps S] [-K topk] [--f32] [--scores] model_file output_file\n" in r.stdout
    assert "    -l lambda      the regulariser of the model (required with --fold-in)\n" in r.stdout
    (tmp_path / "users").write_text("1\n")
    for extra in (["-x", "d"], ["-u", "users"], ["--diversity"], ["--mmr", "0.5"], ["--tradeoff", "0,1"], ["--eval", "d", "--ranks"]):
        r = run([RECOMMEND, "--fold-in-ridge", "d", "-l", "1"] + extra + ["m", "o"], tmp_path)
        assert r.returncode == 1 and "--fold-in-ridge does not go with" in r.stderr, (extra, r.stderr)
    for extra in (["--allow", "users"], ["--candidates", "users"], ["--fold-in", "d"], ["-s", "2"], ["--steps", "3"]):
        r = run([RECOMMEND, "--fold-in-ridge", "d", "-l", "1"] + extra + ["m", "o"], tmp_path)
        assert r.returncode == 1 and "--fold-in-ridge" in r.stderr, (extra, r.stderr)
    r = run([RECOMMEND, "--fold-in-ridge", "d", "m", "o"], tmp_path)
    assert r.returncode == 1 and "--fold-in-ridge needs -l" in r.stderr
    r = run([RECOMMEND, "--fold-in-ridge", "d", "-l", "-1", "m", "o"], tmp_path)
    assert r.returncode == 1 and "-l" in r.stderr
    r = run([RECOMMEND, "--plain-reg", "m", "o"], tmp_path)
    assert r.returncode == 1 and "--plain-reg goes with --fold-in-ridge" in r.stderr
    r = run([RECOMMEND, "--fold-in", "d", "-l", "1", "-s", "0", "m", "o"], tmp_path)          # --fold-in keeps refusing -s 0
    assert r.returncode == 1 and "-s" in r.stderr
    R = synth.generate("tiny", seed=3)                              # 60 x 40
    d = synth.write_dir(R, str(tmp_path / "data"))
    rng = np.random.default_rng(2)
    pcr.model_save(str(tmp_path / "wrong.model"), rng.standard_normal((5, 4)), rng.standard_normal((R.d2 + 1, 4)))
    r = run([RECOMMEND, "--fold-in-ridge", d, "-l", "1", "wrong.model", "out"], tmp_path)
    assert r.returncode == 1 and "items, the model" in r.stderr, r.stderr


@pytest.mark.parametrize("k", RANKS)
def test_fixture_is_well_conditioned(k):
    """Every system of the fixture -- the one its form factors and the primal one the forced-CG run iterates on -- stays below a
    condition number of 1e4, weighted and plain; the fixture holds the lengths the issue lists."""
    idx, it, val = users_of(k)
    lens = np.diff(idx)
    assert list(lens) == lengths(k) and set(FIXED) <= set(lens)
    for b in pcr.ridge_boundaries(k):
        assert {b - 1, b, b + 1} <= set(lens)
    assert {k - 1, k, k + 1} <= set(lens)
    a, b = int(idx[DUP_USER]), int(idx[DUP_USER + 1])
    assert it[a] == it[b - 1] and len(set(it[a:b])) == b - a - 1                       # one item twice
    a, b = int(idx[DESC_USER]), int(idx[DESC_USER + 1])
    assert np.all(np.diff(it[a:b]) < 0)                                                # given item-descending
    assert val.min() >= 1.0 and val.max() <= 5.0
    F = factors(k)
    assert LAM >= 1e-2 * float((F * F).sum(axis=1).mean()) * 0.99
    for weighted in (True, False):
        c = rr.conditions(F, idx, it, LAM, weighted)
        solved = np.where(lens <= k, np.maximum(c[:, 0], c[:, 1]), c[:, 1])     # (no form solves the n x n system of a user with n > k)
        assert solved.max() < COND_MAX, (weighted, solved.max())


# ------------------------------------------------------------------------------------------------------------------------------
# GPU part
# ------------------------------------------------------------------------------------------------------------------------------

def check_against_reference(k, pname, weighted, U, pu, forms=None):
    Uref, lref, oref = reference(k, pname, weighted)
    lens = np.diff(users_of(k)[0])
    e = row_err(U, Uref)
    el, eo = rel(pu[:, 3], lref), rel(pu[:, 4], oref)
    print(f"k={k} {pname} weighted={weighted}: row {e.max():.3g} loss {el.max():.3g} obj {eo.max():.3g}")
    assert e.max() <= (FP64_ROW if pname == "F64" else FP32_ROW), (int(e.argmax()), e.max())
    assert el.max() <= OBJ_TOL[pname], (int(el.argmax()), el.max())
    assert eo.max() <= OBJ_TOL[pname], (int(eo.argmax()), eo.max())
    assert np.array_equal(pu[:, 0], lens.astype(np.float64))
    if forms is not None:
        assert list(pu[:, 1]) == forms
        assert np.all(pu[:, 5] == pcr.PCR_RIDGE_OK), pu[:, 5]
        assert np.all(pu[pu[:, 1] != pcr.PCR_RIDGE_CG, 2] == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("weighted", [True, False], ids=["weighted", "plain"])
@pytest.mark.parametrize("pname", ["F64", "F32"])
@pytest.mark.parametrize("k", RANKS)
def test_length_edges_against_the_reference(k, pname, weighted):
    """Largest deviations observed on the MI355X are recorded in NOTES.md ("Ridge fold-in")."""
    X = users_of(k)
    U, st, pu = pcr.fold_in_ridge(factors(k), X, LAM, weighted=weighted, dtype=PREC[pname], per_user=True)
    forms = [rr.form(n, k) for n in lengths(k)]
    check_against_reference(k, pname, weighted, U, pu, forms)
    assert st["users"] == len(forms) and st["dual"] == forms.count(0) and st["primal"] == forms.count(1) and st["cg"] == forms.count(2)
    assert st["singular"] == 0 and st["cg_cap"] == 0 and st["iters"] == int(pu[:, 2].sum())
    assert st["loss"] == float(np.cumsum(pu[:, 3])[-1]) and st["obj"] == float(np.cumsum(pu[:, 4])[-1])
    if 2 in forms:
        assert np.all(pu[pu[:, 1] == 2, 2] >= 1)
    assert np.all(U[0] == 0.0) and pu[0, 3] == 0.0 and pu[0, 4] == 0.0               # the user without ratings


@pytest.mark.gpu
@pytest.mark.parametrize("weighted", [True, False], ids=["weighted", "plain"])
@pytest.mark.parametrize("pname", ["F64", "F32"])
@pytest.mark.parametrize("k", RANKS)
def test_forms_agree(k, pname, weighted):
    """The same users under pcr_tune ridge_form=cg: every user takes the CG form and lands within the same bounds."""
    with pcr.tuned(ridge_form="cg"):
        U, st, pu = pcr.fold_in_ridge(factors(k), users_of(k), LAM, weighted=weighted, dtype=PREC[pname], per_user=True)
    assert np.all(pu[:, 1] == pcr.PCR_RIDGE_CG) and st["cg"] == st["users"] and st["dual"] == st["primal"] == 0
    assert np.all(pu[:, 5] != pcr.PCR_RIDGE_SINGULAR)
    check_against_reference(k, pname, weighted, U, pu)
    with pcr.tuned(ridge_form="auto"):
        U2, _, pu2 = pcr.fold_in_ridge(factors(k), users_of(k), LAM, weighted=weighted, dtype=PREC[pname], per_user=True)
    assert list(pu2[:, 1]) == [rr.form(n, k) for n in lengths(k)]
    e = row_err(U, U2)
    assert e.max() <= (FP64_ROW if pname == "F64" else FP32_ROW)


def sub_csr(X, users, reverse=False):
    idx, it, val = X
    rows = [(it[idx[u]:idx[u + 1]], val[idx[u]:idx[u + 1]]) for u in users]
    if reverse:
        rows = [(a[::-1], b[::-1]) for a, b in rows]
    nidx = np.concatenate([[0], np.cumsum([len(a) for a, _ in rows])]).astype(np.int64)
    return nidx, np.concatenate([a for a, _ in rows]).astype(np.int32), np.concatenate([b for _, b in rows])


@pytest.mark.gpu
@pytest.mark.parametrize("pname", ["F64", "F32"])
@pytest.mark.parametrize("k", [17, 116])
def test_determinism_and_independence(k, pname):
    """A user's row and table line are the same bits alone in a call, first or last in a shuffled batch of 500, with the batch
    split in two and across two identical calls."""
    F = factors(k)
    rng = np.random.default_rng(3)
    pool = np.array([n for n in lengths(k) if n <= 400])
    X = rr.make_users(D2, list(rng.choice(pool, size=500)), 23)
    call = lambda Y: pcr.fold_in_ridge(F, Y, LAM, dtype=PREC[pname], per_user=True)
    Ua, sa, pa = call(X)
    Ub, sb, pb = call(X)
    assert np.array_equal(Ua.view(np.uint64), Ub.view(np.uint64)) and np.array_equal(pa.view(np.uint64), pb.view(np.uint64)) and sa == sb
    perm = rng.permutation(500)
    Up, _, pp = call(sub_csr(X, perm))
    assert np.array_equal(Up, Ua[perm]) and np.array_equal(pp, pa[perm])
    for part in (np.arange(0, 250), np.arange(250, 500)):
        Uh, _, ph = call(sub_csr(X, part))
        assert np.array_equal(Uh, Ua[part]) and np.array_equal(ph, pa[part])
    lens = np.diff(X[0])
    for u in {int(perm[0]), int(perm[-1]), int(lens.argmax()), int(np.flatnonzero(lens > 0)[lens[lens > 0].argmin()])}:
        U1, _, p1 = call(sub_csr(X, [u]))
        assert np.array_equal(U1[0], Ua[u]) and np.array_equal(p1[0], pa[u]), u
    Ud, _, pd = call(sub_csr(X, np.arange(500), reverse=True))         # rows given item-descending
    assert np.array_equal(Ud, Ua) and np.array_equal(pd, pa)


def _small():
    R = synth.generate("small", seed=31, d1=300, d2=400, nnz=300 * 40)
    return R, pcr.Dataset.from_ratings(R)


@pytest.mark.gpu
@pytest.mark.parametrize("pname", ["F64", "F32"])
def test_solver_entry_on_a_ccdr1_and_on_a_primalcr_solver(pname):
    """Solver.fold_in_ridge on a CCDR1 solver and on a PrimalCR++ solver holding the same V equal fold_in_ridge(V, ...) bit for
    bit; the solver is left as a twin that never folded anything in."""
    R, ds = _small()
    k, lam = 8, 0.05
    idx, it, val = users_of(17)
    sub = (idx, it % R.d2, val)                                        # (duplicated items: two ratings each)
    prm = dict(k=k, precision=PREC[pname], solver_type=pcr.PCR_SOLVER_CCDR1, **{"lambda": lam})
    a, b = pcr.Solver(ds, pcr.Parameter(**prm)), pcr.Solver(ds, pcr.Parameter(**prm))
    for s in (a, b):
        s.set_factors(pcr.initial_col(R.d1, k), None)
        s.iterate(2)
    U, V = a.get_factors()
    mis = a.counter("ccd_residual_mismatch")
    for weighted in (True, False):
        Us, ss, ps = a.fold_in_ridge(sub, weighted=weighted, per_user=True)
        Um, sm, pm = pcr.fold_in_ridge(V, sub, lam, weighted=weighted, dtype=PREC[pname], per_user=True)
        assert np.array_equal(Us.view(np.uint64), Um.view(np.uint64)) and np.array_equal(ps.view(np.uint64), pm.view(np.uint64)) and ss == sm
    c = pcr.Solver(ds, pcr.Parameter(k=k, precision=PREC[pname], solver_type=pcr.PCR_SOLVER_PCRPP, **{"lambda": lam}))
    c.set_factors(U, V)
    Uc, sc, pc = c.fold_in_ridge(sub, per_user=True)
    Um, sm, pm = pcr.fold_in_ridge(V, sub, lam, dtype=PREC[pname], per_user=True)
    assert np.array_equal(Uc.view(np.uint64), Um.view(np.uint64)) and np.array_equal(pc.view(np.uint64), pm.view(np.uint64)) and sc == sm
    Uc2, Vc2 = c.get_factors()
    assert np.array_equal(Uc2, U) and np.array_equal(Vc2, V)
    c.close()
    assert a.counter("ccd_residual_mismatch") == mis == b.counter("ccd_residual_mismatch")
    assert all(np.array_equal(x, y) for x, y in zip(a.get_factors(), b.get_factors()))
    ra, rb = a.iterate(1), b.iterate(1)
    key = ("obj", "cg_v", "cg_u")
    assert [[x[f] for f in key] for x in ra] == [[x[f] for f in key] for x in rb]
    assert all(np.array_equal(x, y) for x, y in zip(a.get_factors(), b.get_factors()))
    assert a.counter("ccd_residual_mismatch") == b.counter("ccd_residual_mismatch")
    a.close(); b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pname", ["F64", "F32"])
def test_singular_systems_are_reported_exactly_on_dyadic_inputs(pname):
    """lambda = 0 on rows (2, 0, ...): two ratings of one item (dual) and three ratings at rank 2 (primal) are SINGULAR with a
    zero row and loss = |r|^2; one rating r is solved exactly, u = (r / 2, 0, ...)."""
    for k in (5, 2):
        F = np.zeros((10, k)); F[:, 0] = 2.0
        idx = np.array([0, 2, 3, 6 if k == 2 else 3, (6 if k == 2 else 3) + 1], np.int64)
        it = np.array([4, 4, 7] + ([1, 2, 3] if k == 2 else []) + [9], np.int32)
        val = np.array([1.0, 3.0, 5.0] + ([1.0, 2.0, 4.0] if k == 2 else []) + [3.0])
        U, st, pu = pcr.fold_in_ridge(F, (idx, it, val), 0.0, dtype=PREC[pname], per_user=True)
        assert pu[0, 1] == pcr.PCR_RIDGE_DUAL and pu[0, 5] == pcr.PCR_RIDGE_SINGULAR and np.all(U[0] == 0.0) and pu[0, 3] == 10.0 == pu[0, 4]
        assert pu[1, 5] == pcr.PCR_RIDGE_OK and list(U[1]) == [2.5] + [0.0] * (k - 1) and pu[1, 3] == 0.0 and pu[1, 4] == 0.0
        if k == 2:
            assert pu[2, 1] == pcr.PCR_RIDGE_PRIMAL and pu[2, 5] == pcr.PCR_RIDGE_SINGULAR and np.all(U[2] == 0.0) and pu[2, 3] == 21.0
        assert pu[3, 5] == pcr.PCR_RIDGE_OK and list(U[3]) == [1.5] + [0.0] * (k - 1)
        assert st["singular"] == (2 if k == 2 else 1) and st["cg_cap"] == 0


@pytest.mark.gpu
def test_against_ccdr1_itself():
    """Train -s 0 for a few outer iterations in fp64 and fold the training users back in with the training lambda, weighted: the
    fold-in is the exact minimiser of what CCDR1 descends on, per user -- and per item with F = U and the item-major CSR."""
    R, ds = _small()
    k, lam = 8, 0.05
    s = pcr.Solver(ds, pcr.Parameter(k=k, precision=pcr.PCR_F64, solver_type=pcr.PCR_SOLVER_CCDR1, **{"lambda": lam}))
    s.set_factors(pcr.initial_col(R.d1, k), None)
    s.iterate(3)
    U, V = s.get_factors()
    s.close()
    idx, it, val = ds.csr(0)
    it = it.astype(np.int32)
    order = np.argsort(it, kind="stable")                              # item-major CSR: row j = the users who rated item j
    users_of_rating = np.repeat(np.arange(R.d1), np.diff(idx)).astype(np.int32)
    cidx = np.concatenate([[0], np.cumsum(np.bincount(it, minlength=R.d2))]).astype(np.int64)
    sides = (("user", V, U, (idx, it, val)), ("item", U, V, (cidx, users_of_rating[order], val[order])))
    for side, F, trained, (xi, xt, xv) in sides:
        New, st, pu = pcr.fold_in_ridge(F, (xi, xt, xv), lam, weighted=True, per_user=True)
        assert st["singular"] == 0 and st["cg_cap"] == 0
        for i in range(len(xi) - 1):
            A, r = F[xt[xi[i]:xi[i + 1]]], xv[xi[i]:xi[i + 1]]
            mu = lam * len(r)
            o_tr = rr.loss_obj(A, r, mu, trained[i])[1]
            o_new = rr.loss_obj(A, r, mu, New[i])[1]
            assert o_new <= o_tr * (1 + 1e-9), (side, i, o_new, o_tr)
            assert abs(pu[i, 4] - o_new) <= 1e-9 * max(1.0, o_new)
            g = A.T @ (A @ New[i] - r) + mu * New[i]
            assert np.abs(g).max() <= 1e-7 * max(1.0, np.abs(A.T @ r).max() if len(r) else 0.0), (side, i, np.abs(g).max())


@pytest.mark.gpu
def test_end_to_end(tmp_path):
    """recommend_new_users_ridge is fold_in_ridge + recommend(exclude=...) bit for bit; the CLI's --fold-in-ridge output file and
    summary line agree with the Python calls; --eval prints the top-N block."""
    R, ds = _small()
    d = synth.write_dir(R, str(tmp_path / "data"))
    k, lam = 8, 0.05
    rng = np.random.default_rng(4)
    U, V = rng.normal(size=(R.d1, k)) / np.sqrt(k), rng.normal(size=(R.d2, k)) / np.sqrt(k)
    pcr.model_save(str(tmp_path / "m.model"), U, V)
    for plain in (False, True):
        Un, stats = pcr.fold_in_ridge(V, ds, lam, weighted=not plain)
        items, scores, U2, st2 = pcr.recommend_new_users_ridge(V, ds, lam, 10, weighted=not plain)
        ri, rs = pcr.recommend(Un, V, 10, exclude=ds)
        assert np.array_equal(U2, Un) and st2 == stats and np.array_equal(items, ri) and np.array_equal(scores, rs)
        flag = ["--plain-reg"] if plain else []
        r = run([RECOMMEND, "--fold-in-ridge", d, "-l", str(lam)] + flag + ["m.model", "lists.txt"], tmp_path)
        assert r.returncode == 0, r.stderr
        want = ("foldin_ridge users %d dual %d primal %d cg %d singular %d cg_cap %d iters %d loss %s obj %s" %
                (stats["users"], stats["dual"], stats["primal"], stats["cg"], stats["singular"], stats["cg_cap"], stats["iters"],
                 "%g" % stats["loss"], "%g" % stats["obj"]))
        assert r.stdout.splitlines() == [want]
        lines = open(tmp_path / "lists.txt").read().splitlines()
        assert lines == [" ".join([str(u + 1)] + [str(j + 1) for j in row if j >= 0]) for u, row in enumerate(ri)]
    r = run([RECOMMEND, "--fold-in-ridge", d, "-l", str(lam), "--plain-reg", "--eval", d, "-c", "5,10", "m.model"], tmp_path)
    assert r.returncode == 0, r.stderr
    ev = pcr.evaluate_topn(Un, V, ds, cutoffs=(5, 10), exclude=ds)
    out = r.stdout.splitlines()
    assert out[0] == want and len(out) == 3
    for line, e in zip(out[1:], ev):
        f = line.split()
        assert f[0] == "cutoff" and int(f[1]) == e["cutoff"] and int(f[3]) == e["users"] and int(f[7]) == e["hits"]
        assert f[9] == "%g" % e["precision"] and f[11] == "%g" % e["recall"] and f[17] == "%g" % e["ndcg"], (line, e)
