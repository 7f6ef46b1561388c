"""Confidence-weighted / implicit fold-in (pcr_fold_in_conf_model, pcr_fold_in_conf; include/primalcr.h, "confidence-weighted and
implicit fold-in"): header / API agreement, argument errors, the form rule, the CLI's refusals, the
fixture's conditioning and the reference against itself on the CPU; on the GPU bitwise parity with the ridge entry, every length
edge against tests/conf_ref.py (np.linalg.solve per user), the forms against each other, the completed-row identity, weight 2 as
a rating given twice, determinism, singular systems on dyadic inputs, implicit CCDR1's own objective, the solver entry and the CLI.

The fixture is tests/test_foldin_ridge.py's (3000 rows of about N(0, 1) / sqrt(k), ratings in 1..5, LAM = 0.05) with weights drawn
from {0.25, 0.5, 1, 2, 4} and alpha in {0, 0.25, 1}, so that c_p < alpha occurs: test_fixture_is_well_conditioned holds every
system below the project's cap of 1e4 (the largest is about 214), so the reference's own error (about 1e4 x 2^-53 = 1e-12
relative) sits far inside the bounds: FP64_ROW / FP32_ROW per row, 1e-9 / 1e-5 relative on loss and obj."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import conf_ref as cr
import primalcr_amd as pcr
import ridge_ref as rr
from conftest import BIN_DIR, ROOT
from primalcr_amd import synth

RECOMMEND = os.path.join(BIN_DIR, "omp-pmf-recommend")
ERR_ARG, ERR_DEVICE = -1, -4
D2 = 3000
RANKS = [1, 3, 4, 16, 17, 100, 112, 116]
FIXED = [0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 300, 2049]
LAM = 0.05
PREC = {"F64": pcr.PCR_F64, "F32": pcr.PCR_F32}
FP64_ROW, FP32_ROW = 1e-7, 5e-3
OBJ_TOL = {"F64": 1e-9, "F32": 1e-5}
COND_MAX = 1e4
DUP_USER, DESC_USER = 6, 7
WEIGHTS = np.array([0.25, 0.5, 1.0, 2.0, 4.0])
CONFIGS = {"w-a0": (True, 0.0), "w-a.25": (True, 0.25), "w-a1": (True, 1.0)}       # (weights given, alpha)


def lengths(k):
    """test_foldin_ridge.py's fixed lengths, then each boundary of the form rule (with and without alpha) and +-1 of it, and
    k - 1, k, k + 1."""
    extra = set()
    for b in pcr.conf_boundaries(k, False) + pcr.conf_boundaries(k, True):
        extra |= {b - 1, b, b + 1}
    extra |= {k - 1, k, k + 1}
    return FIXED + sorted(x for x in extra - set(FIXED) if x >= 0)


_F, _X, _REF = {}, {}, {}


def factors(k):
    if k not in _F:
        _F[k] = np.random.default_rng(5).normal(size=(D2, k)) / np.sqrt(k)
    return _F[k]


def users_of(k):
    """(index, item, val, weights): ridge_ref.make_users' rows with one weight of WEIGHTS per rating."""
    if k not in _X:
        idx, it, val = rr.make_users(D2, lengths(k), 11, dup_user=DUP_USER, desc_user=DESC_USER)
        _X[k] = idx, it, val, np.random.default_rng(17).choice(WEIGHTS, size=len(it))
    return _X[k]


def reference(k, pname, weighted, cfg):
    key = (k, pname, weighted, cfg)
    if key not in _REF:
        idx, it, val, w = users_of(k)
        given, alpha = CONFIGS[cfg]
        _REF[key] = cr.fold_in(factors(k), idx, it, val, LAM, weights=w if given else None, alpha=alpha, weighted=weighted, f32=pname == "F32")
    return _REF[key]


def row_err(U, Uref):
    return np.abs(U - Uref).max(axis=1) / np.maximum(1.0, np.abs(Uref).max(axis=1))


def rel(a, b):
    return np.abs(a - b) / np.where(b == 0.0, 1.0, np.abs(b))


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def run(cmd, cwd):
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True)


def call(k, pname, weighted, cfg, X=None, **kw):
    idx, it, val, w = users_of(k) if X is None else X
    given, alpha = CONFIGS[cfg]
    return pcr.fold_in_conf(factors(k), (idx, it, val), LAM, weights=w if given else None, alpha=alpha, weighted=weighted, dtype=PREC[pname],
                            per_user=True, **kw)


# ------------------------------------------------------------------------------------------------------------------------------
# CPU part
# ------------------------------------------------------------------------------------------------------------------------------

def test_header_and_api_agree():
    L = pcr.lib()
    assert hasattr(L, "pcr_fold_in_conf_model") and hasattr(L, "pcr_fold_in_conf")
    hdr = open(os.path.join(ROOT, "include", "primalcr.h")).read()
    flat = " ".join(hdr.split())
    assert ("int pcr_fold_in_conf_model(const double *F, int64_t rows, int64_t k, double lambda, int weighted, double alpha, int precision, "
            "int device, int64_t n, const int64_t *index, const int32_t *item, const double *val, const double *weight") in flat
    assert ("int pcr_fold_in_conf(pcr_solver *s, int weighted, double alpha, int64_t n, const int64_t *index, const int32_t *item, "
            "const double *val, const double *weight, double *U_out, pcr_ridge_stats *stats, double *per_user);") in flat
    assert hdr.index("/* ridge fold-in:") < hdr.index("/* confidence-weighted and implicit fold-in:") < hdr.index("/* non-negative fold-in:")
    assert len(L.pcr_fold_in_conf_model.argtypes) == 16 and len(L.pcr_fold_in_conf.argtypes) == 11
    assert L.pcr_fold_in_conf_model.argtypes[5] is C.c_double and L.pcr_fold_in_conf.argtypes[2] is C.c_double
    for name in ("fold_in_conf", "recommend_new_users_conf", "conf_form", "conf_boundaries"):
        assert hasattr(pcr, name) and name in pcr.__all__, name
    assert hasattr(pcr.Solver, "fold_in_conf")


@pytest.mark.parametrize("k", RANKS + [8, 64, 65, 200])
def test_form_rule_and_boundaries(k):
    """A function of (len, k, alpha > 0) alone: the ridge rule at alpha == 0; for alpha > 0 primal at every length while the padded
    rank fits the direct forms, CG beyond; one wave never carries more than 4 x 4 tiles."""
    kp = (k + 15) // 16 * 16
    for n in list(range(0, 130)) + [300, 2049, 100000]:
        assert pcr.conf_form(n, k, False) == pcr.ridge_form(n, k) == cr.form(n, k, False)
        f = pcr.conf_form(n, k, True)
        assert f == cr.form(n, k, True) == (pcr.PCR_RIDGE_PRIMAL if kp <= pcr.PCR_RIDGE_DIRECT_MAX else pcr.PCR_RIDGE_CG)
        for imp in (False, True):
            b = pcr.conf_block(n, k, imp)
            assert b == cr.block(n, k, imp)
            form = pcr.conf_form(n, k, imp)
            side = kp if form == pcr.PCR_RIDGE_PRIMAL else (n + 15) // 16 * 16
            if form != pcr.PCR_RIDGE_CG and b == 64:
                assert side <= 64 and n <= pcr.PCR_RIDGE_WAVE_MAX, (n, k, imp)
            if form == pcr.PCR_RIDGE_CG:
                assert b == 256
    assert set(pcr.ridge_boundaries(k)) <= set(pcr.conf_boundaries(k, False)) <= set(pcr.ridge_boundaries(k)) | {pcr.PCR_RIDGE_WAVE_MAX}
    assert pcr.conf_boundaries(k, True) == ([pcr.PCR_RIDGE_WAVE_MAX] if kp <= 64 else [])
    for b in pcr.conf_boundaries(k, False):
        assert (pcr.conf_form(b, k), pcr.conf_block(b, k)) != (pcr.conf_form(b + 1, k), pcr.conf_block(b + 1, k))


def test_argument_errors_come_before_any_device_and_name_the_entry():
    F = factors(3)
    idx, it, val = np.array([0, 2, 3], np.int64), np.array([5, 1, 7], np.int32), np.array([1.0, 2.0, 3.0])
    w = np.array([1.0, 2.0, 0.5])

    def refused(match, **kw):
        a = dict(F=F, ratings=(idx, it, val), lam=1.0, weights=w, alpha=0.5)
        a.update(kw)
        with pytest.raises(pcr.PcrError, match=match) as e:
            pcr.fold_in_conf(**a)
        assert f"error {ERR_ARG}:" in str(e.value) and "pcr_fold_in_conf_model" in str(e.value), str(e.value)

    for bad in (0.0, -1.0, np.nan, np.inf):
        refused("weight", weights=np.array([1.0, bad, 0.5]))
    for bad in (-0.5, np.nan, np.inf, -np.inf):
        refused("alpha", alpha=bad)
    refused("outside", ratings=(idx, np.array([5, 1, D2], np.int32), val))
    refused("outside", ratings=(idx, np.array([5, -1, 7], np.int32), val))
    refused("not finite", ratings=(idx, it, np.array([1.0, np.nan, 3.0])))
    refused("monotone", ratings=(np.array([0, 3, 2, 3], np.int64), it, val))
    refused(r"index\[0\]", ratings=(np.array([1, 2, 3], np.int64), it, val))
    refused("lambda", lam=-1.0)
    refused("lambda", lam=float("nan"))
    refused("precision", dtype=7)
    with pytest.raises(ValueError, match="one weight per rating"):
        pcr.fold_in_conf(F, (idx, it, val), 1.0, weights=np.ones(2))
    L = pcr.lib()
    out = np.zeros((2, 3))
    args = lambda Fp, rows, k, outp: (Fp, rows, k, 1.0, 1, 0.5, pcr.PCR_F64, 0, 2, idx.ctypes.data, it.ctypes.data, val.ctypes.data, w.ctypes.data, outp,
                                      None, None)
    for bad in (args(None, D2, 3, out.ctypes.data), args(F.ctypes.data, D2, 3, None), args(F.ctypes.data, D2, 0, out.ctypes.data),
                args(F.ctypes.data, 0, 3, out.ctypes.data)):
        assert L.pcr_fold_in_conf_model(*bad) == ERR_ARG
        assert b"pcr_fold_in_conf_model" in L.pcr_last_error()
    assert L.pcr_fold_in_conf(None, 1, 0.5, 2, idx.ctypes.data, it.ctypes.data, val.ctypes.data, w.ctypes.data, out.ctypes.data, None, None) == ERR_ARG


def test_without_a_device_the_call_fails_with_err_device():
    """Valid arguments on a process that sees no GPU: PCR_ERR_DEVICE (never a CPU path), with and without weights / alpha."""
    code = ("import sys, numpy as np; sys.path.insert(0, sys.argv[1])\n"
            "import primalcr_amd as pcr\n"
            "X = (np.array([0, 2, 2]), np.array([1, 4]), np.array([1.0, 2.0]))\n"
            "for kw in (dict(), dict(weights=np.array([2.0, 0.5]), alpha=0.5)):\n"
            "    try:\n"
            "        pcr.fold_in_conf(np.ones((6, 3)), X, 1.0, **kw)\n"
            "        print('no error')\n"
            "    except pcr.PcrError as e:\n"
            "        print(str(e))\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    assert out.stdout.count(f"error {ERR_DEVICE}:") == 2, out.stdout


def test_cli_usage_and_refusals(tmp_path):
    r = run([RECOMMEND], tmp_path)
    assert r.returncode == 1
    assert "omp-pmf-recommend --fold-in-ridge data_dir -l lambda [--rating-weights file] [--implicit alpha] ...\n" in r.stdout
    (tmp_path / "w").write_text("1 1 2.0\n")
    for mine in (["--rating-weights", "w"], ["--implicit", "0.5"]):
        for other in (["--fold-in", "d"], ["--fold-in-nnls", "d"], ["--fold-in-items", "w"]):
            r = run([RECOMMEND] + other + ["-l", "1"] + mine + ["m", "o"], tmp_path)
            assert r.returncode == 1 and mine[0] + " does not go with --fold-in, --fold-in-nnls or --fold-in-items" in r.stderr, (mine, other, r.stderr)
        r = run([RECOMMEND] + mine + ["m", "o"], tmp_path)
        assert r.returncode == 1 and mine[0] + " goes with --fold-in-ridge" in r.stderr, r.stderr
    for bad in ("-1", "nan", "inf", "x", "0.5x", ""):
        r = run([RECOMMEND, "--fold-in-ridge", "d", "-l", "1", "--implicit", bad, "m", "o"], tmp_path)
        assert r.returncode == 1 and "--implicit" in r.stderr and "finite number >= 0" in r.stderr, (bad, r.stderr)
    # a malformed weights file and one that does not match the ratings are refused on the host (this process sees no device)
    R = synth.generate("tiny", seed=3)
    d = synth.write_dir(R, str(tmp_path / "data"))
    rng = np.random.default_rng(2)
    pcr.model_save(str(tmp_path / "m.model"), rng.standard_normal((5, 4)), rng.standard_normal((R.d2, 4)))
    (tmp_path / "bad").write_text("1 1 2.0\n1 x 1.0\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    for wfile in ("bad", "w"):
        r = subprocess.run([RECOMMEND, "--fold-in-ridge", d, "-l", "1", "--rating-weights", wfile, "m.model", "o"], cwd=tmp_path, capture_output=True,
                           text=True, env=env)
        assert r.returncode == 1 and "--rating-weights" in r.stderr and "device" not in r.stderr.lower(), r.stderr


@pytest.mark.parametrize("k", RANKS)
def test_fixture_is_well_conditioned(k):
    """Every system of the fixture -- primal and dual, weighted and plain, at each alpha -- has a positive smallest eigenvalue and
    a condition number below the project's cap; the fixture holds the lengths the issue lists, and c_p < alpha occurs."""
    idx, it, val, w = users_of(k)
    lens = np.diff(idx)
    assert list(lens) == lengths(k) and set(FIXED) <= set(lens) and {k - 1, k, k + 1} <= set(lens)
    for b in pcr.conf_boundaries(k, False) + pcr.conf_boundaries(k, True):
        assert {b - 1, b, b + 1} <= set(lens)
    a, b = int(idx[DUP_USER]), int(idx[DUP_USER + 1])
    assert it[a] == it[b - 1] and len(set(it[a:b])) == b - a - 1
    a, b = int(idx[DESC_USER]), int(idx[DESC_USER + 1])
    assert np.all(np.diff(it[a:b]) < 0)
    assert set(np.unique(w)) == set(WEIGHTS) and w.min() < 1.0 < w.max()
    F = factors(k)
    worst = 0.0
    for weighted in (True, False):
        for given, alpha in list(CONFIGS.values()) + [(False, 0.0), (False, 1.0)]:
            c = cr.conditions(F, idx, it, LAM, weights=w if given else None, alpha=alpha, weighted=weighted)
            assert c[:, 0].min() > 0.0 and c[:, 1].max() < COND_MAX, (weighted, given, alpha, c[:, 0].min(), c[:, 1].max())
            worst = max(worst, c[:, 1].max())
    print(f"k={k}: largest condition number {worst:.4g}")


@pytest.mark.parametrize("k", [3, 17, 100])
def test_reference_implicit_equals_the_completed_row(k):
    """Reference against reference at d = 300: the implicit problem on a sparse row is the alpha = 0 weighted problem on the
    completed row -- all d items, the unrated ones as rating 0 of weight alpha -- to 1e-10."""
    d = 300
    F = np.random.default_rng(6).normal(size=(d, k)) / np.sqrt(k)
    idx, it, val = rr.make_users(d, [0, 1, 5, 64, 65, 299, 300], 13)
    w = np.random.default_rng(7).choice(WEIGHTS, size=len(it))
    for alpha in (0.25, 1.0):
        for weighted in (True, False):
            U, loss, obj = cr.fold_in(F, idx, it, val, LAM, weights=w, alpha=alpha, weighted=weighted)
            cidx, cit, cval, cw = cr.completed(F, idx, it, val, w, alpha)
            Uc, lc, oc = cr.fold_in(F, cidx, cit, cval, LAM, weights=cw, alpha=0.0, weighted=weighted)
            assert row_err(U, Uc).max() <= 1e-10 and rel(loss, lc).max() <= 1e-10 and rel(obj, oc).max() <= 1e-10


# ------------------------------------------------------------------------------------------------------------------------------
# GPU part
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("weighted", [True, False], ids=["weighted", "plain"])
@pytest.mark.parametrize("pname", ["F64", "F32"])
@pytest.mark.parametrize("k", RANKS)
def test_parity_with_the_ridge_entry(k, pname, weighted):
    """weight = NULL, alpha = 0 (the ridge kernels themselves) and weight = ones, alpha = 0 (the weighted instantiations) return
    the ridge entry's rows and per-user table bit for bit."""
    idx, it, val, _ = users_of(k)
    U, st, pu = pcr.fold_in_ridge(factors(k), (idx, it, val), LAM, weighted=weighted, dtype=PREC[pname], per_user=True)
    for w in (None, np.ones(len(it))):
        U2, st2, pu2 = pcr.fold_in_conf(factors(k), (idx, it, val), LAM, weights=w, alpha=0.0, weighted=weighted, dtype=PREC[pname], per_user=True)
        assert np.array_equal(bits(U), bits(U2)) and np.array_equal(bits(pu), bits(pu2)) and st == st2, w is None


def check_against_reference(k, pname, weighted, cfg, U, pu, forms=None):
    Uref, lref, oref = reference(k, pname, weighted, cfg)
    lens = np.diff(users_of(k)[0])
    e = row_err(U, Uref)
    el, eo = rel(pu[:, 3], lref), rel(pu[:, 4], oref)
    print(f"k={k} {pname} weighted={weighted} {cfg}: row {e.max():.3g} loss {el.max():.3g} obj {eo.max():.3g}")
    assert e.max() <= (FP64_ROW if pname == "F64" else FP32_ROW), (int(e.argmax()), e.max())
    assert el.max() <= OBJ_TOL[pname], (int(el.argmax()), el.max())
    assert eo.max() <= OBJ_TOL[pname], (int(eo.argmax()), eo.max())
    assert np.array_equal(pu[:, 0], lens.astype(np.float64))
    if forms is not None:
        assert list(pu[:, 1]) == forms
        assert np.all(pu[:, 5] == pcr.PCR_RIDGE_OK), pu[:, 5]
        assert np.all(pu[pu[:, 1] != pcr.PCR_RIDGE_CG, 2] == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("weighted", [True, False], ids=["weighted", "plain"])
@pytest.mark.parametrize("pname", ["F64", "F32"])
@pytest.mark.parametrize("k", RANKS)
def test_length_edges_against_the_reference(k, pname, weighted, cfg):
    """Largest deviations observed on the MI355X are recorded in NOTES.md ("Confidence-weighted / implicit fold-in")."""
    U, st, pu = call(k, pname, weighted, cfg)
    forms = [cr.form(n, k, CONFIGS[cfg][1] > 0.0) for n in lengths(k)]
    check_against_reference(k, pname, weighted, cfg, U, pu, forms)
    assert st["users"] == len(forms) and st["dual"] == forms.count(0) and st["primal"] == forms.count(1) and st["cg"] == forms.count(2)
    assert st["singular"] == 0 and st["cg_cap"] == 0 and st["iters"] == int(pu[:, 2].sum())
    assert st["loss"] == float(np.cumsum(pu[:, 3])[-1]) and st["obj"] == float(np.cumsum(pu[:, 4])[-1])
    assert np.all(U[0] == 0.0) and pu[0, 3] == 0.0 and pu[0, 4] == 0.0 and pu[0, 5] == pcr.PCR_RIDGE_OK       # the user without ratings


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("pname", ["F64", "F32"])
@pytest.mark.parametrize("k", RANKS)
def test_forms_agree(k, pname, cfg):
    """The same users under pcr_tune ridge_form=cg: every user takes the CG form, stays below its iteration cap and lands within
    the same bounds of the reference and of the default forms."""
    alpha = CONFIGS[cfg][1]
    for weighted in (True, False):
        with pcr.tuned(ridge_form="cg"):
            U, st, pu = call(k, pname, weighted, cfg)
        assert np.all(pu[:, 1] == pcr.PCR_RIDGE_CG) and st["cg"] == st["users"] and st["dual"] == st["primal"] == 0
        assert np.all(pu[:, 5] == pcr.PCR_RIDGE_OK) and st["cg_cap"] == 0
        cap = np.array([2 * k + 10 if alpha > 0.0 else 2 * min(n, k) + 10 for n in lengths(k)])
        assert np.all(pu[:, 2] < cap), (pu[:, 2], cap)
        check_against_reference(k, pname, weighted, cfg, U, pu)
        U2, _, pu2 = call(k, pname, weighted, cfg)
        assert list(pu2[:, 1]) == [cr.form(n, k, alpha > 0.0) for n in lengths(k)]
        assert row_err(U, U2).max() <= (FP64_ROW if pname == "F64" else FP32_ROW)


@pytest.mark.gpu
@pytest.mark.parametrize("pname", ["F64", "F32"])
@pytest.mark.parametrize("k", [3, 17, 100])
def test_completion_device_against_device(k, pname):
    """d = 300: the implicit call on the sparse rows against the alpha = 0 call on the completed rows, within the row bounds."""
    d = 300
    F = np.random.default_rng(6).normal(size=(d, k)) / np.sqrt(k)
    idx, it, val = rr.make_users(d, [0, 1, 5, 64, 65, 299, 300], 13)
    w = np.random.default_rng(7).choice(WEIGHTS, size=len(it))
    for alpha in (0.25, 1.0):
        cidx, cit, cval, cw = cr.completed(F, idx, it, val, w, alpha)
        for weighted in (True, False):
            U, st, pu = pcr.fold_in_conf(F, (idx, it, val), LAM, weights=w, alpha=alpha, weighted=weighted, dtype=PREC[pname], per_user=True)
            Uc, sc, pc = pcr.fold_in_conf(F, (cidx, cit, cval), LAM, weights=cw, alpha=0.0, weighted=weighted, dtype=PREC[pname], per_user=True)
            assert st["singular"] == st["cg_cap"] == sc["singular"] == sc["cg_cap"] == 0
            e = row_err(U[1:], Uc[1:])
            print(f"k={k} {pname} alpha={alpha} weighted={weighted}: row {e.max():.3g}")
            assert e.max() <= (FP64_ROW if pname == "F64" else FP32_ROW), (int(e.argmax()), e.max())
            assert np.all(U[0] == 0.0) and np.abs(Uc[0]).max() <= (FP64_ROW if pname == "F64" else FP32_ROW)


@pytest.mark.gpu
@pytest.mark.parametrize("pname", ["F64", "F32"])
@pytest.mark.parametrize("k", [3, 17, 100])
def test_weight_two_is_the_rating_twice(k, pname):
    """alpha = 0, device against device: ratings of weight 2 against the same ratings given twice with weight 1 (W and so mu are
    equal).  At k = 100 the pairs stand on both sides of len = k: 60 / 90 (dual, dual) and 90 / 120 (dual, primal), 120 / 150."""
    F = factors(k)
    idx, it, val = rr.make_users(D2, [1, 2, 5, 60, 90, 120, 300], 29)
    rng = np.random.default_rng(31)
    w = rng.choice(WEIGHTS, size=len(it))
    idx2, it2, val2, w2 = [0], [], [], []
    for u in range(len(idx) - 1):
        a, b = int(idx[u]), int(idx[u + 1])
        twice = np.arange(a, b)[: max(1, (b - a) // 2)]                # the first half of the row is given twice
        w[twice] = 2.0
        it2 += list(it[a:b]) + list(it[twice]); val2 += list(val[a:b]) + list(val[twice])
        w2 += [1.0 if z in set(twice) else w[z] for z in range(a, b)] + [1.0] * len(twice)
        idx2.append(len(it2))
    X2 = np.array(idx2, np.int64), np.array(it2, np.int32), np.array(val2)
    for weighted in (True, False):
        U, st, pu = pcr.fold_in_conf(F, (idx, it, val), LAM, weights=w, weighted=weighted, dtype=PREC[pname], per_user=True)
        U2, st2, pu2 = pcr.fold_in_conf(F, X2, LAM, weights=np.array(w2), weighted=weighted, dtype=PREC[pname], per_user=True)
        if k == 100:
            assert list(pu[:, 1]) == [0, 0, 0, 0, 0, 1, 1] and list(pu2[:, 1]) == [0, 0, 0, 0, 1, 1, 1]
        e = row_err(U, U2)
        print(f"k={k} {pname} weighted={weighted}: row {e.max():.3g}")
        assert e.max() <= (FP64_ROW if pname == "F64" else FP32_ROW), (int(e.argmax()), e.max())


def sub_csr(X, users, reverse=False):
    idx, it, val, w = X
    rows = [(it[idx[u]:idx[u + 1]], val[idx[u]:idx[u + 1]], w[idx[u]:idx[u + 1]]) for u in users]
    if reverse:
        rows = [(a[::-1], b[::-1], c[::-1]) for a, b, c in rows]
    nidx = np.concatenate([[0], np.cumsum([len(a) for a, _, _ in rows])]).astype(np.int64)
    return (nidx, np.concatenate([a for a, _, _ in rows]).astype(np.int32), np.concatenate([b for _, b, _ in rows]),
            np.concatenate([c for _, _, c in rows]))


@pytest.mark.gpu
@pytest.mark.parametrize("alpha", [0.0, 0.25])
@pytest.mark.parametrize("pname", ["F64", "F32"])
@pytest.mark.parametrize("k", [17, 116])
def test_determinism_and_independence(k, pname, alpha):
    """A user's row and table line are the same bits across two identical calls, with the users reversed or shuffled, in two
    sub-batches, alone, and with every row given item-descending (the weights travel with the ratings)."""
    F = factors(k)
    rng = np.random.default_rng(3)
    pool = np.array([n for n in lengths(k) if n <= 400])
    idx, it, val = rr.make_users(D2, list(rng.choice(pool, size=200)), 23)
    X = idx, it, val, rng.choice(WEIGHTS, size=len(it))
    go = lambda Y: pcr.fold_in_conf(F, Y[:3], LAM, weights=Y[3], alpha=alpha, dtype=PREC[pname], per_user=True)
    Ua, sa, pa = go(X)
    Ub, sb, pb = go(X)
    assert np.array_equal(bits(Ua), bits(Ub)) and np.array_equal(bits(pa), bits(pb)) and sa == sb
    for perm in (np.arange(200)[::-1], rng.permutation(200)):
        Up, _, pp = go(sub_csr(X, perm))
        assert np.array_equal(bits(Up), bits(Ua[perm])) and np.array_equal(bits(pp), bits(pa[perm]))
    for part in (np.arange(0, 100), np.arange(100, 200)):
        Uh, _, ph = go(sub_csr(X, part))
        assert np.array_equal(bits(Uh), bits(Ua[part])) and np.array_equal(bits(ph), bits(pa[part]))
    lens = np.diff(idx)
    for u in {0, 199, int(lens.argmax())}:
        U1, _, p1 = go(sub_csr(X, [u]))
        assert np.array_equal(bits(U1[0]), bits(Ua[u])) and np.array_equal(bits(p1[0]), bits(pa[u])), u
    Ud, _, pd = go(sub_csr(X, np.arange(200), reverse=True))
    assert np.array_equal(bits(Ud), bits(Ua)) and np.array_equal(bits(pd), bits(pa))


@pytest.mark.gpu
@pytest.mark.parametrize("alpha", [0.0, 0.5])
@pytest.mark.parametrize("pname", ["F64", "F32"])
def test_singular_systems_are_reported_exactly_on_dyadic_inputs(pname, alpha):
    """lambda = 0 on rows (2, 0): a zero column of F makes every primal system singular, and two ratings of one item the dual one;
    the row is zeros and loss = obj = sum c r^2 exactly (dyadic weights and alpha).  One rating at rank 5 and alpha = 0 is solved
    exactly through the dual form."""
    k = 2
    F = np.zeros((10, k)); F[:, 0] = 2.0
    idx = np.array([0, 2, 5, 5], np.int64)
    it = np.array([4, 4, 1, 2, 3], np.int32)
    val = np.array([1.0, 3.0, 1.0, 2.0, 4.0])
    w = np.array([0.5, 2.0, 4.0, 0.25, 2.0])
    U, st, pu = pcr.fold_in_conf(F, (idx, it, val), 0.0, weights=w, alpha=alpha, dtype=PREC[pname], per_user=True)
    want_form = pcr.PCR_RIDGE_PRIMAL if alpha > 0 else pcr.PCR_RIDGE_DUAL
    assert pu[0, 1] == want_form and pu[0, 5] == pcr.PCR_RIDGE_SINGULAR and np.all(U[0] == 0.0) and pu[0, 3] == 0.5 + 18.0 == pu[0, 4]
    assert pu[1, 1] == pcr.PCR_RIDGE_PRIMAL and pu[1, 5] == pcr.PCR_RIDGE_SINGULAR and np.all(U[1] == 0.0) and pu[1, 3] == 4.0 + 1.0 + 32.0 == pu[1, 4]
    assert pu[2, 5] == pcr.PCR_RIDGE_OK and np.all(U[2] == 0.0) and pu[2, 3] == 0.0 == pu[2, 4]
    assert st["singular"] == 2 and st["cg_cap"] == 0
    if alpha == 0.0:
        F5 = np.zeros((10, 5)); F5[:, 0] = 2.0
        U, st, pu = pcr.fold_in_conf(F5, (np.array([0, 1], np.int64), np.array([9], np.int32), np.array([3.0])), 0.0, weights=np.array([4.0]),
                                     dtype=PREC[pname], per_user=True)
        assert pu[0, 1] == pcr.PCR_RIDGE_DUAL and pu[0, 5] == pcr.PCR_RIDGE_OK and list(U[0]) == [1.5, 0.0, 0.0, 0.0, 0.0] and pu[0, 3] == 0.0


def _implicit_ccdr1(prec=pcr.PCR_F64):
    """About 60 x 40 at rank 4: CCDR1 with rating weights and set_implicit(0.5), a few iterations."""
    R = synth.generate("tiny", seed=3)
    ds = pcr.Dataset.from_ratings(R)
    idx, it, val = ds.csr(0)
    w = np.random.default_rng(41).choice(WEIGHTS, size=len(it))
    s = pcr.Solver(ds, pcr.Parameter(k=4, precision=prec, solver_type=pcr.PCR_SOLVER_CCDR1, **{"lambda": LAM}))
    s.set_factors(pcr.initial_col(R.d1, 4), None)
    s.set_rating_weights(w)
    s.set_implicit(0.5)
    s.iterate(3)
    return R, ds, s, (idx, it.astype(np.int32), val, w)


@pytest.mark.gpu
def test_against_implicit_ccdr1_itself():
    """Fold every training user -- and, with F = U and the item-major ratings, every item -- back into an implicit CCDR1 model with
    its own weights and the stored alpha: the folded row's objective is at most the trained row's, and the table's obj is the
    reference's at the returned row."""
    R, ds, s, (idx, it, val, w) = _implicit_ccdr1()
    U, V = s.get_factors()
    alpha = s.counter("ccd_implicit")
    s.close()
    assert alpha == 0.5
    order = np.argsort(it, kind="stable")
    users_of_rating = np.repeat(np.arange(R.d1), np.diff(idx)).astype(np.int32)
    cidx = np.concatenate([[0], np.cumsum(np.bincount(it, minlength=R.d2))]).astype(np.int64)
    sides = (("user", V, U, (idx, it, val, w)), ("item", U, V, (cidx, users_of_rating[order], val[order], w[order])))
    for side, F, trained, (xi, xt, xv, xw) in sides:
        New, st, pu = pcr.fold_in_conf(F, (xi, xt, xv), LAM, weights=xw, alpha=alpha, weighted=True, per_user=True)
        assert st["singular"] == 0 and st["cg_cap"] == 0 and st["primal"] == st["users"]
        G, d = F.T @ F, F.shape[0]
        for i in range(len(xi) - 1):
            a, b = xi[i], xi[i + 1]
            if a == b:
                assert np.all(New[i] == 0.0)
                continue
            A, r, c = F[xt[a:b]], xv[a:b], xw[a:b]
            mu = cr.mu_of(LAM, c, alpha, d, True)
            o_tr = cr.loss_obj(A, r, c, alpha, G, mu, trained[i])[1]
            o_new = cr.loss_obj(A, r, c, alpha, G, mu, New[i])[1]
            assert o_new <= o_tr * (1 + 1e-9), (side, i, o_new, o_tr)
            assert abs(pu[i, 4] - o_new) <= 1e-9 * max(1.0, o_new), (side, i, pu[i, 4], o_new)


@pytest.mark.gpu
@pytest.mark.parametrize("pname", ["F64", "F32"])
def test_solver_entry(pname):
    """Solver.fold_in_conf on the implicit CCDR1 solver (alpha=None: its stored alpha) and on a PrimalCR++ solver holding the same
    factors equals fold_in_conf(V, ...) bit for bit; nothing of the solver is written."""
    R, ds, s, (idx, it, val, w) = _implicit_ccdr1(PREC[pname])
    U, V = s.get_factors()
    X = (idx, it, val)
    for weighted in (True, False):
        Us, ss, ps = s.fold_in_conf(X, weights=w, weighted=weighted, per_user=True)
        Um, sm, pm = pcr.fold_in_conf(V, X, LAM, weights=w, alpha=0.5, weighted=weighted, dtype=PREC[pname], per_user=True)
        assert np.array_equal(bits(Us), bits(Um)) and np.array_equal(bits(ps), bits(pm)) and ss == sm
        assert ss["primal"] == ss["users"]
    Us, ss, ps = s.fold_in_conf(X, weights=w, alpha=0.0, per_user=True)
    Um, sm, pm = pcr.fold_in_conf(V, X, LAM, weights=w, alpha=0.0, dtype=PREC[pname], per_user=True)
    assert np.array_equal(bits(Us), bits(Um)) and np.array_equal(bits(ps), bits(pm)) and ss == sm
    assert all(np.array_equal(x, y) for x, y in zip(s.get_factors(), (U, V))) and s.counter("ccd_implicit") == 0.5
    s.close()
    c = pcr.Solver(ds, pcr.Parameter(k=4, precision=PREC[pname], solver_type=pcr.PCR_SOLVER_PCRPP, **{"lambda": LAM}))
    c.set_factors(U, V)
    Uc, sc, pc = c.fold_in_conf(X, weights=w, alpha=0.25, per_user=True)
    Um, sm, pm = pcr.fold_in_conf(V, X, LAM, weights=w, alpha=0.25, dtype=PREC[pname], per_user=True)
    assert np.array_equal(bits(Uc), bits(Um)) and np.array_equal(bits(pc), bits(pm)) and sc == sm
    U0, s0, p0 = c.fold_in_conf(X, per_user=True)                       # (no implicit setting on this solver type: alpha = 0, no weights: the ridge entry)
    Ur, sr, pr = c.fold_in_ridge(X, per_user=True)
    assert np.array_equal(bits(U0), bits(Ur)) and np.array_equal(bits(p0), bits(pr)) and s0 == sr
    assert all(np.array_equal(x, y) for x, y in zip(c.get_factors(), (U, V)))
    c.close()


@pytest.mark.gpu
def test_end_to_end(tmp_path):
    """recommend_new_users_conf is fold_in_conf + recommend(exclude=...) bit for bit; the CLI's --rating-weights / --implicit
    output file and summary line agree with the Python calls."""
    R = synth.generate("tiny", seed=3)
    ds = pcr.Dataset.from_ratings(R)
    d = synth.write_dir(R, str(tmp_path / "data"))
    k = 4
    rng = np.random.default_rng(4)
    U, V = rng.normal(size=(R.d1, k)) / np.sqrt(k), rng.normal(size=(R.d2, k)) / np.sqrt(k)
    pcr.model_save(str(tmp_path / "m.model"), U, V)
    idx, it, val = ds.csr(0)
    w = rng.choice(WEIGHTS, size=len(it))
    users = np.repeat(np.arange(R.d1), np.diff(idx))
    order = rng.permutation(len(it))                                   # (any order: the file is matched to the ratings)
    (tmp_path / "w.txt").write_text("".join(f"{users[z] + 1} {it[z] + 1} {w[z]}\n" for z in order))
    for flags, kw in ((["--rating-weights", "w.txt"], dict(weights=w)), (["--implicit", "0.5"], dict(alpha=0.5)),
                      (["--rating-weights", "w.txt", "--implicit", "0.25", "--plain-reg"], dict(weights=w, alpha=0.25, weighted=False))):
        Un, stats = pcr.fold_in_conf(V, ds, LAM, **kw)
        items, scores, U2, st2 = pcr.recommend_new_users_conf(V, ds, LAM, 10, **kw)
        ri, rs = pcr.recommend(Un, V, 10, exclude=ds)
        assert np.array_equal(U2, Un) and st2 == stats and np.array_equal(items, ri) and np.array_equal(scores, rs)
        r = run([RECOMMEND, "--fold-in-ridge", d, "-l", str(LAM)] + flags + ["m.model", "lists.txt"], tmp_path)
        assert r.returncode == 0, r.stderr
        want = ("foldin_conf users %d dual %d primal %d cg %d singular %d cg_cap %d iters %d loss %s obj %s" %
                (stats["users"], stats["dual"], stats["primal"], stats["cg"], stats["singular"], stats["cg_cap"], stats["iters"],
                 "%g" % stats["loss"], "%g" % stats["obj"]))
        assert r.stdout.splitlines() == [want]
        lines = open(tmp_path / "lists.txt").read().splitlines()
        assert lines == [" ".join([str(u + 1)] + [str(j + 1) for j in row if j >= 0]) for u, row in enumerate(ri)]
