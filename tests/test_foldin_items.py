"""Item fold-in (include/primalcr.h, "item fold-in": pcr_fold_in_items_model, pcr_fold_in_items, omp-pmf-recommend --fold-in-items):
rows of V for items a PrimalCR / PrimalCR++ model was not trained on.  The checker is tests/itemfold_ref.py: F_j, its gradient and
Hessian-vector product by all pairs in numpy fp64 and the loop of rules 1-6 restated from the header -- anchored, without any
restated loop, to the in-tree oracle (F_j is the change of objective_new when the item is appended; its gradient and H a are the
last rows of obtain_g_new / compute_Ha_new) and to strong convexity (|v - v*| <= |grad F_j(v)| / lambda)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import itemfold_ref as ir
import primalcr_amd as pcr
from conftest import BIN_DIR, ROOT
from exact_data import density, dyadic_matrix
from oracle.oracle_py import CSR
from primalcr_amd import synth

RECOMMEND = os.path.join(BIN_DIR, "omp-pmf-recommend")
TRAIN = os.path.join(BIN_DIR, "omp-pmf-train")
ERR_ARG, ERR_DEVICE, ERR_STATE, ERR_UNSUPPORTED = -1, -4, -6, -7
GRID = [(7, 32.0), (100, 32.0), (12, 1.0), (1, 32.0), (132, 32.0)]
SOLVERS = (2, 1)
STARTS = ("zero", "dyadic")
CELLS = [(k, lam, s, st) for (k, lam) in GRID for s in SOLVERS for st in STARTS]
CELL_IDS = [f"k{k}-l{lam:g}-s{s}-{st}" for k, lam, s, st in CELLS]
PREC = {"F64": pcr.PCR_F64, "F32": pcr.PCR_F32}
FP64_ROW, FP32_ROW = 1e-7, 5e-3          # the project's per-row bounds (tests/test_foldin.py)
FP32_OBJ = 2e-5                           # the project's fp32 objective tolerance
FIELDS = ("raters", "steps", "cg", "ls", "obj0", "obj", "gnorm2", "status")
F = {f: i for i, f in enumerate(FIELDS)}
D1 = pcr.PCR_ITEMFOLD_LDS_MAX + 2 + 10   # just above the largest rater count of the fixture
LOOP_CELL = (12, 1.0, "dyadic")           # (k, lambda, start) of the tests of the whole loop
LOOP_STEPS = 30
CAP_STEPS = 2                             # ... and the step cap at which the loop's fixture holds items of every end


def rater_counts():
    """One new item per rater count 0 .. 3, around 32, 64 and 128, 500, and -1 / +0 / +1 around every count at which k_itemfold changes form."""
    base = [0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 500]
    extra = set()
    for b in pcr.itemfold_boundaries():
        extra |= {b - 1, b, b + 1}
    return base + sorted(extra - set(base))


_FIX, _UV, _REF = {}, {}, {}


def fixture(solver):
    if solver not in _FIX:
        _FIX[solver] = ir.make_fixture(solver, D1, rater_counts())
    return _FIX[solver]


def factors(k):
    if k not in _UV:
        rng = np.random.default_rng(5)
        _UV[k] = (rng.normal(size=(D1, k)) / np.sqrt(k), rng.normal(size=(ir.D2, k)) / np.sqrt(k))
    return _UV[k]


def model(k, lam, solver):
    U, V = factors(k)
    return ir.Model(U, V, fixture(solver)[0], solver, lam)


def start(kind, n, k):
    if kind == "zero":
        return np.zeros((n, k))
    return np.rint(np.random.default_rng(17).normal(0.0, 0.1, size=(n, k)) * 1024.0) / 1024.0      # multiples of 2^-10: exact in fp32


def cg_knobs():
    p = pcr.Parameter()
    return dict(cg_max=p.cg_max_iter, cg_tol=p.cg_tol)


def ref_steps(cell, nsteps):
    """The numpy loop's first steps of a cell, each one step from its own previous point (computed once, shared)."""
    have = _REF.setdefault(cell, [])
    k, lam, solver, st = cell
    M, items = model(k, lam, solver), fixture(solver)[1]
    while len(have) < nsteps:
        V0 = have[-1][0] if have else start(st, len(items), k)
        have.append(ir.fold_in_items(M, items, V0, 1, **cg_knobs()))
    return have[:nsteps]


def train_args(X):
    return X.idx, X.item.astype(np.int32), X.val


def foldin(cell, V0, steps, dtype, items=None, **kw):
    k, lam, solver, _ = cell
    U, V = factors(k)
    X, its, _ = fixture(solver)
    return pcr.fold_in_items(U, V, train_args(X), ir.item_csr(its if items is None else items), lam, solver_type=solver, V0=V0, steps=steps,
                             dtype=dtype, per_item=True, **kw)


def run(cmd, cwd):
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True)


def row_ratio(A, B, fac):
    return np.abs(A - B).max(1) / (fac * np.maximum(np.abs(B).max(1), 1e-3 * np.abs(B).max()))


# ------------------------------------------------------------------------------------------------------------------------------
# CPU part
# ------------------------------------------------------------------------------------------------------------------------------

def test_symbols_constants_and_fields():
    L = pcr.lib()
    assert hasattr(L, "pcr_fold_in_items_model") and hasattr(L, "pcr_fold_in_items")
    hdr = open(os.path.join(ROOT, "include", "primalcr.h")).read()
    for name, val in (("PCR_ITEMFOLD_WAVE_MAX", pcr.PCR_ITEMFOLD_WAVE_MAX), ("PCR_ITEMFOLD_LDS_MAX", pcr.PCR_ITEMFOLD_LDS_MAX),
                      ("PCR_ITEMFOLD_SCORES_WAVE_MAX", pcr.PCR_ITEMFOLD_SCORES_WAVE_MAX), ("PCR_ITEMFOLD_FIELDS", len(pcr.PCR_ITEMFOLD_FIELDS))):
        assert f"#define {name}" in hdr and int(hdr.split(f"#define {name}")[1].split()[0]) == val, name
    assert pcr.PCR_ITEMFOLD_FIELDS == FIELDS
    assert C.sizeof(pcr.ItemfoldStats) == 80
    assert [f for f, _ in pcr.ItemfoldStats._fields_] == ["items", "converged", "step_cap", "stalled", "steps", "cg", "ls", "raters", "unique_raters", "obj"]
    b = pcr.itemfold_boundaries()
    assert b == [pcr.PCR_ITEMFOLD_WAVE_MAX, pcr.PCR_ITEMFOLD_LDS_MAX] and set(b) | {x - 1 for x in b} | {x + 1 for x in b} <= set(rater_counts())
    lens = set(np.diff(fixture(2)[0].idx).tolist())
    for x in pcr.rater_scores_boundaries():
        assert {x - 1, x, x + 1} <= lens
    assert "not modelled" in hdr.split("item fold-in")[1] and "itemfold_table_bytes" in hdr
    assert pcr.tune("itemfold_table_bytes", "4096") is None and pcr.tune("itemfold_table_bytes", None) is None


def test_argument_errors_come_before_any_device_and_name_the_entry():
    rng = np.random.default_rng(1)
    U, V = rng.normal(size=(4, 3)), rng.normal(size=(6, 3))
    tr = (np.array([0, 2, 2, 3, 5], np.int64), np.array([0, 5, 1, 2, 3], np.int32), np.array([1.0, 2.0, 3.0, 4.0, 5.0]))
    new = (np.array([0, 2, 3], np.int64), np.array([0, 3, 2], np.int32), np.array([1.0, 2.0, 3.0]))

    def refused(match, code=ERR_ARG, **kw):
        a = dict(U=U, V=V, train=tr, new_items=new, lam=32.0)
        a.update(kw)
        with pytest.raises(pcr.PcrError, match=match) as e:
            pcr.fold_in_items(**a)
        assert f"error {code}:" in str(e.value) and "pcr_fold_in_items_model" in str(e.value), str(e.value)

    refused("outside", new_items=(new[0], np.array([0, 4, 2], np.int32), new[2]))
    refused("outside", new_items=(new[0], np.array([0, -1, 2], np.int32), new[2]))
    refused("not finite", new_items=(new[0], new[1], np.array([1.0, np.nan, 3.0])))
    refused("not finite", new_items=(new[0], new[1], np.array([1.0, np.inf, 3.0])))
    refused("monotone", new_items=(np.array([0, 3, 2, 3], np.int64), new[1], new[2]))
    refused(r"index\[0\]", new_items=(np.array([1, 2, 3], np.int64), new[1], new[2]))
    refused("training index not monotone", train=(np.array([0, 2, 1, 3, 5], np.int64), tr[1], tr[2]))
    refused(r"training index\[0\]", train=(np.array([1, 2, 2, 3, 5], np.int64), tr[1], tr[2]))
    refused("training item", train=(tr[0], np.array([0, 6, 1, 2, 3], np.int32), tr[2]))
    refused("training rating", train=(tr[0], tr[1], np.array([1.0, np.nan, 3.0, 4.0, 5.0])))
    refused("steps", steps=0)
    refused("steps", steps=-3)
    refused("precision", dtype=7)
    refused("solver type", solver_type=3)
    refused("CCDR1", code=ERR_UNSUPPORTED, solver_type=pcr.PCR_SOLVER_CCDR1)
    many = np.arange(70000, dtype=np.float64)                       # more levels than the level builder's 16 bits (PrimalCR: raw doubles)
    with pytest.raises(pcr.PcrError, match="pcr_fold_in_items_model.*65535") as e:
        pcr.fold_in_items(np.zeros((1, 2)), np.zeros((70000, 2)), (np.array([0, 70000], np.int64), np.arange(70000, dtype=np.int32), many),
                          (np.array([0, 1], np.int64), np.array([0], np.int32), np.array([1.0])), 1.0, solver_type=pcr.PCR_SOLVER_PCR)
    assert f"error {ERR_UNSUPPORTED}:" in str(e.value)
    with pytest.raises(ValueError):
        pcr.fold_in_items(U, V, tr, new, 32.0, V0=np.zeros((3, 3)))
    with pytest.raises(ValueError):
        pcr.fold_in_items(U[:3], V, tr, new, 32.0)
    p = pcr.Parameter(k=3)
    out = np.zeros((2, 3))
    L = pcr.lib()
    a = [tr[0].ctypes.data, tr[1].ctypes.data, tr[2].ctypes.data, 2, new[0].ctypes.data, new[1].ctypes.data, new[2].ctypes.data, None, 1]
    for Up, Vp, op, t0 in ((None, V.ctypes.data, out.ctypes.data, a[0]), (U.ctypes.data, None, out.ctypes.data, a[0]),
                           (U.ctypes.data, V.ctypes.data, None, a[0]), (U.ctypes.data, V.ctypes.data, out.ctypes.data, None)):
        assert L.pcr_fold_in_items_model(C.byref(p), Up, 4, Vp, 6, t0, *a[1:], op, None, None) == ERR_ARG
        assert b"pcr_fold_in_items_model" in L.pcr_last_error() and b"null" in L.pcr_last_error()
    assert L.pcr_fold_in_items_model(C.byref(p), U.ctypes.data, 4, V.ctypes.data, 6, a[0], None, a[2], *a[3:], out.ctypes.data, None, None) == ERR_ARG
    assert L.pcr_fold_in_items(None, None, 2, new[0].ctypes.data, new[1].ctypes.data, new[2].ctypes.data, None, 1, out.ctypes.data, None, None) == ERR_ARG


def test_without_a_device_the_calls_fail_with_err_device():
    """Valid arguments on a process that sees no GPU: PCR_ERR_DEVICE (never a CPU path)."""
    code = ("import sys, numpy as np; sys.path.insert(0, sys.argv[1])\n"
            "import primalcr_amd as pcr\n"
            "try:\n"
            "    pcr.fold_in_items(np.ones((2, 3)), np.ones((6, 3)), (np.array([0, 2, 2]), np.array([1, 4]), np.array([1.0, 2.0])),\n"
            "                      (np.array([0, 1]), np.array([0]), np.array([2.0])), 1.0)\n"
            "    print('no error')\n"
            "except pcr.PcrError as e:\n"
            "    print(str(e))\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    assert f"error {ERR_DEVICE}:" in out.stdout, out.stdout


def test_cli_usage_and_refusals(tmp_path):
    r = run([RECOMMEND], tmp_path)
    assert r.returncode == 1
    assert "omp-pmf-recommend --fold-in-items ratings_file -x data_dir -l lambda [-s 1|2] [--steps S] [--f32] model_file output_model\n" in r.stdout
    src = open(os.path.join(ROOT, "primalcr_amd", "csrc", "cli", "omp_pmf_recommend.cpp")).read()
    assert "//   omp-pmf-recommend --fold-in-items ratings_file -x data_dir -l lambda [-s 1|2] [--steps S] [--f32] model_file output_model\n" in src
    base = [RECOMMEND, "--fold-in-items", "r.txt", "-x", "d", "-l", "1"]
    for extra in (["--fold-in", "d"], ["--fold-in-ridge", "d"], ["--fold-in-nnls", "d"], ["--eval", "d"], ["--diversity"], ["--mmr", "0.5"],
                  ["--tradeoff", "0,1"], ["--ranks"], ["--allow", "a"], ["--candidates", "c"], ["-K", "5"], ["-u", "users"], ["--scores"],
                  ["--plain-reg"], ["-c", "5"], ["--threshold", "3"], ["--pool", "20"]):
        r = run(base + extra + ["m", "o"], tmp_path)
        assert r.returncode == 1 and "--fold-in-items does not go with" in r.stderr, (extra, r.stderr)
    r = run([RECOMMEND, "--fold-in-items", "r.txt", "-l", "1", "m", "o"], tmp_path)
    assert r.returncode == 1 and "--fold-in-items needs -x" in r.stderr
    r = run([RECOMMEND, "--fold-in-items", "r.txt", "-x", "d", "m", "o"], tmp_path)
    assert r.returncode == 1 and "--fold-in-items needs -l" in r.stderr
    r = run(base + ["m"], tmp_path)
    assert r.returncode == 1 and r.stdout.startswith("Usage:")
    for bad in (["-s", "0"], ["-s", "3"], ["--steps", "0"]):
        r = run(base + bad + ["m", "o"], tmp_path)
        assert r.returncode == 1 and bad[0] in r.stderr, (bad, r.stderr)
    R = synth.generate("tiny", seed=3)                              # 60 x 40
    d = synth.write_dir(R, str(tmp_path / "data"))
    rng = np.random.default_rng(2)
    pcr.model_save(str(tmp_path / "ok.model"), rng.standard_normal((R.d1, 4)), rng.standard_normal((R.d2, 4)))
    pcr.model_save(str(tmp_path / "wrong.model"), rng.standard_normal((5, 4)), rng.standard_normal((R.d2, 4)))
    for text, what in (("1 1\n", "expected"), (f"{R.d1 + 1} 1 3\n", "outside"), ("1 0 3\n", "at least 1"), ("1 1 nan\n", "not finite"),
                       ("1 1 3\n1 2000000000 3\n", "exceeds the 2 ratings")):
        (tmp_path / "r.txt").write_text(text)
        r = run([RECOMMEND, "--fold-in-items", "r.txt", "-x", d, "-l", "1", "ok.model", "out.model"], tmp_path)
        assert r.returncode == 1 and what in r.stderr and not os.path.exists(tmp_path / "out.model"), (text, r.stderr)
    (tmp_path / "r.txt").write_text("1 1 3\n")
    r = run([RECOMMEND, "--fold-in-items", "r.txt", "-x", d, "-l", "1", "wrong.model", "out.model"], tmp_path)
    assert r.returncode == 1 and "the model" in r.stderr, r.stderr


def oracle_anchor(oracle, M, users, vals, v, a):
    """(F_j(v), grad F_j(v), H a) from the in-tree oracle on the appended data, with no loop of this file's: the training rows of
    the item's raters alone (every other user's terms cancel in the difference and are not in row j)."""
    ru = np.unique(users)
    X = M.X
    idx = np.concatenate([[0], np.cumsum(np.diff(X.idx)[ru])])
    sel = np.concatenate([np.arange(X.idx[u], X.idx[u + 1]) for u in ru]) if len(ru) else np.zeros(0, np.int64)
    Xs = CSR(len(ru), X.d2, idx, X.item[sel], X.val[sel])
    Us = M.U[ru]
    Xp = ir.appended(Xs, np.searchsorted(ru, users), vals)
    Vp = np.vstack([M.V, v[None, :]])
    m, mp = oracle.comp_m(Us, M.V, Xs), oracle.comp_m(Us, Vp, Xp)
    Fj = oracle.objective_new(mp, Us, Vp, Xp, M.lam, solver=M.solver) - oracle.objective_new(m, Us, M.V, Xs, M.lam, solver=M.solver)
    g = oracle.obtain_g_new(Us, Vp, Xp, mp, M.lam, solver=M.solver)[-1]
    A = np.zeros_like(Vp); A[-1] = a
    return Fj, g, oracle.compute_Ha_new(A, mp, Us, Xp, M.lam, solver=M.solver)[-1]


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("k,lam", [(7, 32.0), (12, 1.0)])
def test_reference_anchors_on_the_oracle(oracle, solver, k, lam):
    """F_j, its gradient and H a of tests/itemfold_ref.py against the oracle on the appended data, for every item of the fixture
    that lists no user twice (two new ratings of one user would be compared with each other there, which the fold-in does not
    model), at a dyadic start and at a random point."""
    M = model(k, lam, solver)
    X, items, names = fixture(solver)
    rng = np.random.default_rng(3)
    V0 = start("dyadic", len(items), k)
    for j, (users, vals) in enumerate(items):
        if names[j] == "dup":
            continue
        it = ir.Item(M, users, vals)
        for v in (V0[j], rng.normal(size=k) / np.sqrt(k)):
            a = rng.normal(size=k)
            Fj, g, Ha = oracle_anchor(oracle, M, users, vals, v, a)
            scale = max(abs(Fj), 1.0)
            assert abs(it.F(v) - Fj) <= 1e-10 * scale, (names[j], it.F(v), Fj)
            assert np.abs(it.grad(v) - g).max() <= 1e-10 * max(np.abs(g).max(), 1.0), names[j]
            assert np.abs(it.Hv(v, a) - Ha).max() <= 1e-10 * max(np.abs(Ha).max(), 1.0), names[j]


def test_fixture_preconditions_on_the_reference():
    """What the fixture is to hold, shown on the reference alone."""
    for solver in SOLVERS:
        X, items, names = fixture(solver)
        lens = np.diff(X.idx)
        assert X.d1 == D1 and X.d2 == ir.D2 and D1 > pcr.PCR_ITEMFOLD_LDS_MAX + 2
        assert all(lens[u] == n for u, n in ir.LONG_USERS.items()) and lens[ir.EMPTY_USER] == 0 and lens[ir.ONE_RATING_USER] == 1
        a, b = X.idx[ir.ONE_LEVEL_USER], X.idx[ir.ONE_LEVEL_USER + 1]
        assert b - a > 1 and len(np.unique(ir.levels_of(X.val[a:b], solver))) == 1
        assert np.median(lens) <= 8
        assert [len(u) for u, _ in items[:len(rater_counts())]] == rater_counts()
        M = model(7, 32.0, solver)
        by = {nm: ir.Item(M, *items[names.index(nm)]) for nm in ("ties", "dup", "empty_rater", "gap")}
        assert by["ties"].n == 2 and len(by["ties"].sg) > 0 and not by["ties"].anypair                # every new rating ties: no pair
        assert len(by["dup"].users) - len(np.unique(by["dup"].users)) == 1
        assert by["empty_rater"].n == 1 and len(by["empty_rater"].sg) == 0
        g = by["gap"]
        assert (g.sg != 0).all() and (g.sg > 0).any() and (g.sg < 0).any()                           # the level is absent, between two
        levs = ir.levels_of(X.val[X.idx[ir.GAP_USERS[0]]:X.idx[ir.GAP_USERS[0] + 1]], solver)
        assert levs.min() < ir.levels_of(g.vals, solver)[0] < levs.max() and ir.levels_of(g.vals, solver)[0] not in levs


def loop_start(solver):
    """The start rows of the tests of the whole loop: dyadic, but item "restart" starts where the reference's loop (PrimalCR++, the
    fp32 call's roundings, LOOP_STEPS) leaves the item of the most raters -- at that item's fp32 noise floor."""
    key = ("start", solver)
    if key not in _REF:
        k, lam, st = LOOP_CELL
        X, items, names = fixture(solver)
        V0 = start(st, len(items), k)
        if "row" not in _REF:
            j = fixture(2)[2].index("restart")
            _REF["row"] = ir.fold_in_item(ir.Item(model(k, lam, 2), *fixture(2)[1][j]), V0[j], LOOP_STEPS, dtype=np.float32, **cg_knobs())
        V0[names.index("restart")] = _REF["row"][0]
        _REF[key] = V0
    return _REF[key]


def test_fixture_has_every_end_on_the_reference():
    """The reference's loop of LOOP_CELL with the fp32 call's roundings, capped at CAP_STEPS steps: at least one item ends
    CONVERGED, one at the STEP_CAP and one STALLED ("restart": the loop had left its row STALLED, and from there no try is
    accepted)."""
    k, lam, st = LOOP_CELL
    items, names = fixture(2)[1:]
    rows, tab = ir.fold_in_items(model(k, lam, 2), items, loop_start(2), CAP_STEPS, dtype=np.float32, **cg_knobs())
    assert _REF["row"][1]["status"] == ir.STALLED
    status = tab[:, F["status"]].astype(int)
    assert set(status.tolist()) == {ir.CONVERGED, ir.STEP_CAP, ir.STALLED}, status
    j = names.index("restart")
    assert status[j] == ir.STALLED and tab[j, F["steps"]] == 0 and np.array_equal(rows[j], loop_start(2)[j])


# ------------------------------------------------------------------------------------------------------------------------------
# GPU part
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("r", [12, 100])
@pytest.mark.parametrize("pname", ["F32", "F64"])
def test_start_point_values_are_exact_on_dyadic_inputs(pname, r, solver):
    """U, V and V0 with entries of {-1, -1/2, 0, 1/2, 1} (tests/exact_data.py) and lambda = 32: every score is a multiple of 1/4,
    every hinge term too, c of 1/2, g of 1/4 and the objective of 1/16 -- small integers in those units, so every sum is exact in
    fp32 and fp64 in any order.  obj0 and gnorm2 of a steps = 1 call equal the numpy values bit for bit."""
    rng = np.random.default_rng(100 * r + solver)
    X, items, names = fixture(solver)
    U, V, V0 = dyadic_matrix(rng, D1, r, density(r)), dyadic_matrix(rng, ir.D2, r, density(r)), dyadic_matrix(rng, len(items), r, density(r))
    M = ir.Model(U, V, X, solver, 32.0)
    want = np.zeros((len(items), 2))
    for j, (users, vals) in enumerate(items):
        it = ir.Item(M, users, vals)
        g = it.grad(V0[j]) if it.n else np.zeros(r)
        want[j] = it.F(V0[j]), float(g @ g)
        assert np.abs(it.state(it.UR @ V0[j])[1]).max(initial=0.0) * 2 < 2 ** 22 and np.abs(g).max() * 4 < 2 ** 22    # units with bits to spare
    rows, stats, per = pcr.fold_in_items(U, V, train_args(X), ir.item_csr(items), 32.0, solver_type=solver, V0=V0, steps=1, dtype=PREC[pname],
                                         per_item=True)
    bad = np.nonzero((per[:, F["obj0"]] != want[:, 0]) | (per[:, F["gnorm2"]] != want[:, 1]))[0]
    assert len(bad) == 0, [(names[j], per[j, F["obj0"]], want[j, 0], per[j, F["gnorm2"]], want[j, 1]) for j in bad[:5]]
    assert np.array_equal(per[:, F["raters"]], [len(u) for u, _ in items])


@pytest.mark.gpu
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("k,lam", [(7, 32.0), (12, 1.0), (100, 32.0)])
def test_start_point_values_match_the_oracle_anchor(oracle, solver, k, lam):
    """obj0 and gnorm2 of a steps = 1 call in fp64 on the random fixture against the oracle on the appended data (no loop and no
    formula of the checker's own), to 1e-10 relative."""
    M = model(k, lam, solver)
    X, items, names = fixture(solver)
    V0 = start("dyadic", len(items), k)
    rows, stats, per = foldin((k, lam, solver, "dyadic"), V0, 1, pcr.PCR_F64)
    for j, (users, vals) in enumerate(items):
        if names[j] == "dup" or len(users) == 0:
            continue
        Fj, g, _ = oracle_anchor(oracle, M, users, vals, V0[j], np.zeros(k))
        assert abs(per[j, F["obj0"]] - Fj) <= 1e-10 * max(abs(Fj), 1.0), (names[j], per[j, F["obj0"]], Fj)
        assert abs(per[j, F["gnorm2"]] - float(g @ g)) <= 1e-10 * max(float(g @ g), 1.0), (names[j], per[j, F["gnorm2"]], float(g @ g))


@pytest.mark.gpu
@pytest.mark.parametrize("cell", CELLS, ids=CELL_IDS)
def test_steps_one_and_two_match_the_numpy_loop_in_fp64(cell):
    """fold_in_items(steps = 1) from V_prev against one step of the numpy loop from the same V_prev, for steps 1 and 2 (the
    device's own result is fed back): every row within 1e-7 (the project's per-row bound), the CG and line-search counts, the
    status and the step count equal, obj0 and obj to 1e-11."""
    k, lam, solver, st = cell
    M, items = model(k, lam, solver), fixture(solver)[1]
    V0 = start(st, len(items), k)
    for j in (1, 2):
        Vo, tab = ref_steps(cell, 1)[0] if j == 1 else ir.fold_in_items(M, items, V0, 1, **cg_knobs())
        Vg, stats, per = foldin(cell, V0, 1, pcr.PCR_F64)
        ratio = row_ratio(Vg, Vo, FP64_ROW)
        print(f"[itemfold] {cell} step {j}: largest per-row |dV| / bound = {ratio.max():.3e} (item {ratio.argmax()})")
        assert ratio.max() <= 1.0, (j, int(ratio.argmax()), ratio.max())
        for f in ("raters", "steps", "cg", "ls", "status"):
            assert np.array_equal(per[:, F[f]], tab[:, F[f]]), (j, f, per[:, F[f]], tab[:, F[f]])
        for f in ("obj0", "obj"):
            rel = np.abs(per[:, F[f]] - tab[:, F[f]]) / np.maximum(np.abs(tab[:, F[f]]), 1e-300)
            assert rel[tab[:, F[f]] != 0].max(initial=0.0) <= 1e-11 and (per[tab[:, F[f]] == 0, F[f]] == 0).all(), (j, f, rel.max())
        V0 = Vg


@pytest.mark.gpu
@pytest.mark.parametrize("cell", CELLS, ids=CELL_IDS)
def test_step_one_matches_the_numpy_loop_in_fp32(cell):
    """Step 1 in fp32 storage against the fp64 numpy loop: rows to the project's 5e-3 per-row bound, obj0 and obj to its 2e-5
    objective tolerance; an item whose reference |g|^2 at the start is within 1e-3 of the 1e-4 threshold is exempt from the status
    comparison (as in tests/test_foldin.py)."""
    k, lam, solver, st = cell
    items = fixture(solver)[1]
    Vo, tab = ref_steps(cell, 1)[0]
    Vg, stats, per = foldin(cell, start(st, len(items), k), 1, pcr.PCR_F32)
    ratio = row_ratio(Vg, Vo, FP32_ROW)
    print(f"[itemfold] {cell} fp32 step 1: largest per-row |dV| / bound = {ratio.max():.3e} (item {ratio.argmax()})")
    assert ratio.max() <= 1.0, (int(ratio.argmax()), ratio.max())
    near = np.abs(tab[:, F["gnorm2"]] / 1e-4 - 1.0) <= 1e-3
    assert np.array_equal(per[~near, F["status"]], tab[~near, F["status"]]), (per[:, F["status"]], tab[:, F["status"]])
    for f in ("obj0", "obj"):
        rel = np.abs(per[:, F[f]] - tab[:, F[f]]) / np.maximum(np.abs(tab[:, F[f]]), 1e-300)
        print(f"[itemfold] {cell} fp32 step 1: largest relative |d {f}| = {rel[tab[:, F[f]] != 0].max(initial=0.0):.3e}")
        assert rel[tab[:, F[f]] != 0].max(initial=0.0) <= FP32_OBJ, (f, int(rel.argmax()), rel.max())
    assert np.array_equal(Vg.astype(np.float32).astype(np.float64), Vg)        # the storage type's values, widened


@pytest.mark.gpu
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("pname", ["F32", "F64"])
def test_the_loop_is_its_own_single_steps(pname, solver):
    """steps = 3 equals three chained steps = 1 calls bit for bit, rows and tables: an accepted try's carried state is what a fresh
    evaluation at that row gives."""
    k, lam, st = LOOP_CELL
    cell = (k, lam, solver, st)
    n = len(fixture(solver)[1])
    V0 = loop_start(solver)
    V3, s3, p3 = foldin(cell, V0, 3, PREC[pname])
    V, acc, live = V0, np.zeros((n, 8)), np.ones(n, bool)
    for j in range(3):
        V, s1, p1 = foldin(cell, V, 1, PREC[pname])
        if j == 0:
            acc[:, F["obj0"]] = p1[:, F["obj0"]]
        for f in ("steps", "cg", "ls"):
            acc[live, F[f]] += p1[live, F[f]]
        for f in ("raters", "obj", "gnorm2", "status"):
            acc[live, F[f]] = p1[live, F[f]]
        live &= p1[:, F["status"]] == ir.STEP_CAP
    assert np.array_equal(V3, V)
    assert np.array_equal(p3, acc), np.nonzero((p3 != acc).any(1))[0]
    assert (p3[:, F["steps"]] >= 2).any()


HUGE_STEP = 2.0 ** 40


@pytest.mark.gpu
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("pname", ["F32", "F64"])
def test_no_accepted_try_leaves_the_row_as_it_was(pname, solver):
    """Rule 5 where it does not hang on rounding noise: with stepsize = 2^40 the 20 tries are steps of 2^40 .. 2^21 times the
    Newton direction, and F_j, strongly convex, lies above its start at every one of them by many orders of magnitude (lambda/2
    |v|^2 alone grows with the square of the step): no rounding decides.  Every item that does not pass the end test at its start row therefore ends
    STALLED with no step, 20 evaluations, obj = obj0 and the start row as the storage type holds it, bit for bit -- as the
    reference's loop says (statuses equal for every item, |g|^2 at the start to the storage type's tolerance)."""
    k, lam, st = LOOP_CELL
    cell = (k, lam, solver, st)
    X, items, names = fixture(solver)
    V0 = start(st, len(items), k)
    dt = np.float32 if pname == "F32" else np.float64
    rows, tab = ir.fold_in_items(model(k, lam, solver), items, V0, LOOP_STEPS, stepsize=HUGE_STEP, dtype=dt, **cg_knobs())
    assert (tab[:, F["status"]] == ir.STALLED).sum() >= 15 and (np.abs(np.log10(np.maximum(tab[:, F["gnorm2"]], 1e-300) / 1e-4)) > 2).all()
    Vg, stats, per = foldin(cell, V0, LOOP_STEPS, PREC[pname], stepsize=HUGE_STEP)
    assert np.array_equal(per[:, F["status"]], tab[:, F["status"]]), (per[:, F["status"]], tab[:, F["status"]])
    stalled = per[:, F["status"]] == ir.STALLED
    assert (per[:, F["steps"]] == 0).all() and (per[stalled, F["ls"]] == 20).all() and (per[~stalled, F["ls"]] == 0).all()
    assert np.array_equal(Vg, V0.astype(dt).astype(np.float64))
    assert np.array_equal(per[:, F["obj"]], per[:, F["obj0"]])
    rel = np.abs(per[:, F["gnorm2"]] - tab[:, F["gnorm2"]]) / np.maximum(tab[:, F["gnorm2"]], 1e-300)
    assert rel[tab[:, F["gnorm2"]] != 0].max() <= (1e-9 if pname == "F64" else 2 * FP32_ROW), rel.max()
    assert stats["stalled"] == int(stalled.sum()) and stats["steps"] == 0


@pytest.mark.gpu
def test_ends_of_the_capped_loop_in_fp32():
    """fp32 storage, PrimalCR++, from loop_start(), capped at CAP_STEPS: statuses and step counts equal those of the reference's
    loop with fp32 roundings for every item whose decisions the storage type can be trusted with -- no |g|^2 the reference saw
    lies within two decades of the 1e-4 threshold (g after a Newton step is good to a factor in fp32, not to digits: the row
    itself is held to 5e-3), and no accepted try decreased the objective by less than twice the project's fp32 objective
    tolerance, relative.  The compared items hold CONVERGED and STEP_CAP ends.  ("restart" is not among them: its start is the
    noise floor of the REFERENCE's sums, where the reference accepts no try; the device's sums have their own, and it finds one.)
    In the run of LOOP_STEPS no item ends above its start, and a row that ended STALLED is a fixed point of a further call."""
    k, lam, st = LOOP_CELL
    cell = (k, lam, 2, st)
    X, items, names = fixture(2)
    V0 = loop_start(2)
    rows, tab, pers = ir.fold_in_items(model(k, lam, 2), items, V0, CAP_STEPS, want_per=True, dtype=np.float32, **cg_knobs())
    Vc, sc, pc = foldin(cell, V0, CAP_STEPS, pcr.PCR_F32)
    trusted = np.array([all(abs(np.log10(max(g, 1e-300) / 1e-4)) > 2.0 for g in p["gn2_seen"]) and p["min_dec"] > 2 * FP32_OBJ and
                        p["status"] != ir.STALLED for p in pers])
    print(f"[itemfold] fp32 cap {CAP_STEPS}: compared {[names[j] for j in np.nonzero(trusted)[0]]}; device statuses {pc[:, F['status']].astype(int)}")
    assert trusted.sum() >= 15 and set(tab[trusted, F["status"]].astype(int).tolist()) == {ir.CONVERGED, ir.STEP_CAP}
    assert np.array_equal(pc[trusted, F["status"]], tab[trusted, F["status"]]), (pc[:, F["status"]], tab[:, F["status"]])
    assert np.array_equal(pc[trusted, F["steps"]], tab[trusted, F["steps"]])
    Vl, sl, pl = foldin(cell, V0, LOOP_STEPS, pcr.PCR_F32)
    print(f"[itemfold] fp32 loop: statuses {pl[:, F['status']].astype(int)}, steps {pl[:, F['steps']].astype(int)}")
    assert (pl[:, F["obj"]] <= pl[:, F["obj0"]]).all()
    stalled = np.nonzero(pl[:, F["status"]] == ir.STALLED)[0]
    if len(stalled):
        Va, sa, pa = foldin(cell, Vl[stalled], 1, pcr.PCR_F32, items=[items[j] for j in stalled])
        assert np.array_equal(Va, Vl[stalled]) and (pa[:, F["status"]] == ir.STALLED).all() and (pa[:, F["steps"]] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("solver", SOLVERS)
def test_boundary_pairs_in_the_hessian_on_dyadic_inputs(oracle, solver):
    """A pair whose hinge argument is exactly 0 adds nothing to F_j and its gradient but counts in h for PrimalCR++ and not for
    PrimalCR.  On dyadic inputs such pairs are common (asserted).  With cg_max_iter = 1 the step is delta = (g.g / g.Hg) g, so the
    row after one step shows H g: it is compared with the ORACLE's compute_Ha_new on the appended data (its own windows, no
    formula of the checker's), for every item that took its step, fp64."""
    r = 12
    rng = np.random.default_rng(100 * r + solver)
    X, items, names = fixture(solver)
    U, V, V0 = dyadic_matrix(rng, D1, r, density(r)), dyadic_matrix(rng, ir.D2, r, density(r)), dyadic_matrix(rng, len(items), r, density(r))
    M = ir.Model(U, V, X, solver, 32.0)
    rows, stats, per = pcr.fold_in_items(U, V, train_args(X), ir.item_csr(items), 32.0, solver_type=solver, V0=V0, steps=1, cg_max_iter=1,
                                         dtype=pcr.PCR_F64, per_item=True)
    boundary = checked = 0
    for j, (users, vals) in enumerate(items):
        if names[j] == "dup" or per[j, F["steps"]] != 1:
            continue
        it = ir.Item(M, users, vals)
        d = 1.0 - it.sg * ((it.UR @ V0[j])[it.seg] - it.m)
        nb = int(((it.sg != 0) & (d == 0)).sum())
        _, g, _ = oracle_anchor(oracle, M, users, vals, V0[j], np.zeros(r))
        Hg = oracle_anchor(oracle, M, users, vals, V0[j], g)[2]
        assert per[j, F["cg"]] == 1
        want = V0[j] - 0.5 ** (per[j, F["ls"]] - 1) * (float(g @ g) / float(g @ Hg)) * g
        assert np.abs(rows[j] - want).max() <= 1e-12 * max(np.abs(want).max(), 1.0), (names[j], nb, np.abs(rows[j] - want).max())
        if nb:                                                      # the other rule would move the row by far more than the bound
            Ho = Hg + (2.0 if solver == 1 else -2.0) * it.UR.T @ (np.bincount(it.seg[(it.sg != 0) & (d == 0)], minlength=it.n) * (it.UR @ g))
            other = V0[j] - 0.5 ** (per[j, F["ls"]] - 1) * (float(g @ g) / float(g @ Ho)) * g
            if np.abs(other - want).max() > 1e-9 * max(np.abs(want).max(), 1.0):
                boundary += 1
        checked += 1
    assert checked >= 10 and boundary >= 5, (checked, boundary)


@pytest.mark.gpu
@pytest.mark.parametrize("solver", SOLVERS)
def test_properties_of_a_full_run(solver):
    """steps = 30 in fp64: obj <= obj0 for every item; a STALLED row is its start row; CONVERGED rows have gnorm2 < 1e-4 and lie
    within 1e-2 / lambda of v* (strong convexity: |v - v*| <= |grad F_j(v)| / lambda, v* from the numpy Newton run to
    |g| < 1e-12); the stats are the sums of the table."""
    k, lam, st = LOOP_CELL
    cell = (k, lam, solver, st)
    M = model(k, lam, solver)
    X, items, names = fixture(solver)
    V0 = loop_start(solver)
    Vg, stats, per = foldin(cell, V0, LOOP_STEPS, pcr.PCR_F64)
    status = per[:, F["status"]].astype(int)
    print(f"[itemfold] solver {solver}: statuses {np.bincount(status, minlength=3)}, steps {per[:, F['steps']].astype(int)}")
    assert (per[:, F["obj"]] <= per[:, F["obj0"]]).all()
    assert np.array_equal(per[:, F["obj"]] < per[:, F["obj0"]], per[:, F["steps"]] > 0)
    for j in np.nonzero((status == ir.STALLED) & (per[:, F["steps"]] == 0))[0]:
        assert np.array_equal(Vg[j], V0[j])
    for j in np.nonzero(status == ir.CONVERGED)[0]:
        it = ir.Item(M, *items[j])
        if it.n == 0 or (solver == 1 and not it.anypair):
            assert np.array_equal(Vg[j], V0[j]), names[j]
            continue
        assert per[j, F["gnorm2"]] < 1e-4
        vs, gs = ir.minimise(it, Vg[j])
        assert gs < 1e-12, (names[j], gs)
        assert np.linalg.norm(Vg[j] - vs) <= 1e-2 / lam + 1e-12, (names[j], np.linalg.norm(Vg[j] - vs))
        assert abs(per[j, F["obj"]] - it.F(Vg[j])) <= 1e-11 * max(1.0, it.F(Vg[j]))
    assert (status == ir.CONVERGED).any()
    want = dict(items=len(items), converged=int((status == 0).sum()), step_cap=int((status == 1).sum()), stalled=int((status == 2).sum()),
                steps=int(per[:, F["steps"]].sum()), cg=int(per[:, F["cg"]].sum()), ls=int(per[:, F["ls"]].sum()),
                raters=sum(len(u) for u, _ in items), unique_raters=len(np.unique(np.concatenate([u for u, _ in items]))))
    assert {f: stats[f] for f in want} == want
    obj = 0.0
    for x in per[:, F["obj"]]:
        obj += x
    assert stats["obj"] == obj


@pytest.mark.gpu
@pytest.mark.parametrize("pname", ["F32", "F64"])
def test_determinism_and_independence(pname):
    """Two identical calls are bitwise equal; an item gives the same row and table line alone, in the batch, in the reversed batch,
    with its raters listed in reverse, and with the rater table forced into several batches."""
    k, lam, st = LOOP_CELL
    cell = (k, lam, 2, st)
    X, items, names = fixture(2)
    n = len(items)
    V0 = loop_start(2)
    Va, sa, pa = foldin(cell, V0, 10, PREC[pname])
    Vb, sb, pb = foldin(cell, V0, 10, PREC[pname])
    assert np.array_equal(Va, Vb) and np.array_equal(pa, pb) and sa == sb

    def subset(sel, **kw):
        return foldin(cell, V0[sel], 10, PREC[pname], items=[items[j] for j in sel], **kw)

    for j in (1, rater_counts().index(65), rater_counts().index(pcr.PCR_ITEMFOLD_LDS_MAX), rater_counts().index(pcr.PCR_ITEMFOLD_LDS_MAX + 1),
              names.index("dup"), n - 1):
        for sel in ([j], [j] + [q for q in range(0, n, 3) if q != j]):
            V1, _, p1 = subset(sel)
            assert np.array_equal(V1[0], Va[j]) and np.array_equal(p1[0], pa[j]), (names[j], len(sel))
    rev = list(range(n))[::-1]
    Vr, sr, pr = subset(rev)
    assert np.array_equal(Vr, Va[rev]) and np.array_equal(pr, pa[rev])
    Vd, sd, pd = foldin(cell, V0, 10, PREC[pname], items=[(u[::-1], v[::-1]) for u, v in items])      # raters listed in reverse
    assert np.array_equal(Vd[names.index("count500")], Va[names.index("count500")])
    with pcr.tuned(itemfold_table_bytes=4096):
        Vt, stt, pt = foldin(cell, V0, 10, PREC[pname])
    assert np.array_equal(Vt, Va) and np.array_equal(pt, pa) and stt == sa


def _trained():
    R = synth.generate("small", seed=31, d1=300, d2=400, nnz=300 * 40)
    return R, pcr.Dataset.from_ratings(R)


def _new_items(R, rng, n=12):
    items = []
    for j in range(n):
        c = int(rng.integers(0, 90))
        items.append((rng.choice(R.d1, size=c, replace=False), rng.integers(1, 6, size=c).astype(np.float64)))
    return items


@pytest.mark.gpu
@pytest.mark.parametrize("pname", ["F32", "F64"])
def test_solver_entry(pname):
    """Solver.fold_in_items equals fold_in_items() on the solver's own factors bit for bit and leaves get_factors() unchanged; a
    CCDR1 solver and a shard solver are refused with PCR_ERR_STATE."""
    R, ds = _trained()
    k, lam = 8, 50.0
    rng = np.random.default_rng(9)
    U, V = 0.3 * rng.standard_normal((R.d1, k)), 0.3 * rng.standard_normal((R.d2, k))
    new = ir.item_csr(_new_items(R, rng))
    for solver in (2, 1):
        s = pcr.Solver(ds, pcr.Parameter(k=k, precision=PREC[pname], solver_type=solver, **{"lambda": lam}))
        s.set_factors(U, V)
        Us, Vs = s.get_factors()
        Ra, sa, pa = s.fold_in_items(new, steps=5, per_item=True)
        Rm, sm, pm = pcr.fold_in_items(Us, Vs, ds, new, lam, solver_type=solver, steps=5, dtype=PREC[pname], per_item=True)
        assert np.array_equal(Ra, Rm) and np.array_equal(pa, pm) and sa == sm
        assert (pa[:, F["steps"]] > 0).any()
        Rb, sb, pb = s.fold_in_items(new, train=ds, steps=5, per_item=True)
        assert np.array_equal(Ra, Rb)
        U2, V2 = s.get_factors()
        assert np.array_equal(U2, Us) and np.array_equal(V2, Vs)
        other = pcr.Dataset.from_csr(R.d1, R.d2, np.zeros(R.d1 + 1, np.int64), np.zeros(0, np.int32), np.zeros(0))
        with pytest.raises(pcr.PcrError, match=f"error {ERR_ARG}:.*pcr_fold_in_items"):
            s.fold_in_items(new, train=other)
        s.close()
    c = pcr.Solver(ds, pcr.Parameter(k=k, solver_type=pcr.PCR_SOLVER_CCDR1, **{"lambda": lam}))
    with pytest.raises(pcr.PcrError, match=f"error {ERR_STATE}:.*pcr_fold_in_items"):
        c.fold_in_items(new)
    c.close()
    idx, it, val = ds.csr(0)
    tidx, tit, tval = ds.csr(1)
    hi = R.d1 // 3
    dsl = pcr.Dataset.from_csr(hi, R.d2, idx[:hi + 1], it[:idx[hi]], val[:idx[hi]].copy(), tidx[:hi + 1], tit[:tidx[hi]], tval[:tidx[hi]].copy())
    sh = pcr.Solver(dsl, pcr.Parameter(k=k, **{"lambda": lam}), rank=0, nranks=2, shard=(0, R.d1))
    sh.set_local_only(True)
    with pytest.raises(pcr.PcrError, match=f"error {ERR_STATE}:.*pcr_fold_in_items"):
        sh.fold_in_items(new)
    sh.close()


@pytest.mark.gpu
def test_end_to_end(tmp_path):
    """omp-pmf-train, then --fold-in-items: the extended model's new rows equal fold_in_items()'s; recommend() on the stacked V
    serves the new items -- a new item rated as a popular trained item was (its raters' ratings copied) reaches the list of a user
    who did not rate it, where the scores of the stacked model say so."""
    R, ds = _trained()
    d = synth.write_dir(R, str(tmp_path / "data"))
    k, lam = 8, 50.0
    r = run([TRAIN, "-k", str(k), "-t", "3", "-l", str(lam), d, "m.model"], tmp_path)
    assert r.returncode == 0, r.stderr
    U, V = pcr.model_load(str(tmp_path / "m.model"))
    ds = pcr.Dataset.load(d)
    idx, it, val = ds.csr(0)
    user_of = np.repeat(np.arange(R.d1), np.diff(idx))
    popular = np.argsort(-np.bincount(it, minlength=R.d2), kind="stable")[:4]
    items = []
    for q in popular:                                               # every second rater of a popular item rates its clone alike
        sel = np.nonzero(it == q)[0][::2]
        items.append((user_of[sel], val[sel]))
    items.append((np.array([0]), np.array([3.0])))                  # and an item with a single rating
    index, user, rating = ir.item_csr(items)
    lines = [f"{user[z] + 1} {j + 1} {rating[z]:g}" for j in range(len(items)) for z in range(index[j], index[j + 1])]
    (tmp_path / "new.txt").write_text("\n".join(lines) + "\n")
    rows, stats, per = pcr.fold_in_items(U, V, ds, ir.item_csr(items), lam, steps=10, per_item=True)
    r = run([RECOMMEND, "--fold-in-items", "new.txt", "-x", d, "-l", str(lam), "m.model", "x.model"], tmp_path)
    assert r.returncode == 0, r.stderr
    want = ("foldin_items items %d converged %d step_cap %d stalled %d steps %d cg %d ls %d raters %d unique_raters %d obj %s" %
            tuple([stats[f] for f in ("items", "converged", "step_cap", "stalled", "steps", "cg", "ls", "raters", "unique_raters")] + ["%g" % stats["obj"]]))
    assert r.stdout.splitlines() == [want]
    Ux, Vx = pcr.model_load(str(tmp_path / "x.model"))
    assert np.array_equal(Ux, U) and np.array_equal(Vx[:R.d2], V) and np.array_equal(Vx[R.d2:], rows)
    assert (per[:4, F["obj"]] < per[:4, F["obj0"]]).all()
    K = 10
    got, _ = pcr.recommend(U, Vx, K, exclude=(idx, it.astype(np.int32)))
    S = U @ Vx.T
    S[user_of, it] = -np.inf
    kth = -np.sort(-S, axis=1)[:, K - 1]
    served = False
    for j in range(4):
        raters = set(items[j][0].tolist())
        clear = [u for u in range(R.d1) if u not in raters and S[u, R.d2 + j] > kth[u] + 1e-9]      # the scores say: in the top K
        for u in clear:
            assert R.d2 + j in got[u], (j, u)
        served |= len(clear) > 0
    assert served
