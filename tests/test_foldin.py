"""Fold-in of users the model was not trained on (pcr_fold_in_model, pcr_fold_in; include/primalcr.h, "fold-in"; DESIGN.md
section 3.16): argument checks and the fixture's preconditions on the CPU, the device against the oracle step by step, the
loop against its own single steps, the properties of a full run, determinism, the solver entry and the CLI on the GPU.

The reference is tests/foldin_ref.py: the oracle's update_u_new / update_u driven step by step, with the STALLED rule applied
from a plain numpy all-pairs objective."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import foldin_ref as fr
import primalcr_amd as pcr
from conftest import BIN_DIR, ROOT
from primalcr_amd import synth

RECOMMEND = os.path.join(BIN_DIR, "omp-pmf-recommend")
TRAIN = os.path.join(BIN_DIR, "omp-pmf-train")
ERR_ARG, ERR_DEVICE, ERR_STATE, ERR_UNSUPPORTED = -1, -4, -6, -7
D2 = 8300
GRID = [(7, 32.0), (100, 32.0), (12, 1.0), (1, 32.0), (132, 32.0)]
SOLVERS = (2, 1)
STARTS = ("zero", "dyadic")
CELLS = [(k, lam, s, st) for (k, lam) in GRID for s in SOLVERS for st in STARTS]
CELL_IDS = [f"k{k}-l{lam:g}-s{s}-{st}" for k, lam, s, st in CELLS]
PREC = {"F64": pcr.PCR_F64, "F32": pcr.PCR_F32}
FP64_ROW, FP32_ROW = 1e-7, 5e-3          # the project's per-row bounds (test_first_u_step_per_user_under_every_variant)
FP32_OBJ = 2e-5                           # the project's fp32 objective tolerance


def lengths():
    """One user per length of the issue's list, -1 / +0 / +1 around every length at which fold_in changes its code path (the
    library's own constants: api.foldin_boundaries), and a few lengths inside the forms that are no power of two."""
    base = [0, 1, 2, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097, 8200]
    extra = {44, 45, 46, 59, 60, 61, 92, 93, 94, 121, 122, 123, 437, 438, 439, 613, 614, 615}
    for b in pcr.foldin_boundaries():
        extra |= {b - 1, b, b + 1}
    return base + sorted(extra - set(base))


_X, _V, _REF = {}, {}, {}


def users_of(solver):
    """The fixture's users: user 2 has two levels, user 3 one."""
    if solver not in _X:
        two = [1.0, 2.0] if solver == 2 else [1.125, 1.375]
        one = [3.0, 3.0] if solver == 2 else [3.125, 3.125]
        _X[solver] = fr.make_users(D2, lengths(), solver, 11, forced={2: two, 3: one})
    return _X[solver]


def factors(k):
    if k not in _V:
        _V[k] = np.random.default_rng(5).normal(size=(D2, k)) / np.sqrt(k)
    return _V[k]


def start(kind, n, k):
    if kind == "zero":
        return np.zeros((n, k))
    return np.rint(np.random.default_rng(17).normal(0.0, 0.1, size=(n, k)) * 1024.0) / 1024.0      # multiples of 2^-10: exact in fp32


def ref_steps(oracle, cell, nsteps, numpy_too=False):
    """The reference's first steps of a cell, each from the reference's own previous point (shared by the tests that need them)."""
    key = (cell, numpy_too)
    have = _REF.setdefault(key, [])
    k, lam, solver, st = cell
    X, V = users_of(solver), factors(k)
    while len(have) < nsteps:
        U = have[-1][0] if have else start(st, X.d1, k)
        have.append(fr.ref_step(oracle, X, V, lam, solver, U, numpy_too=numpy_too))
    return have[:nsteps]


def foldin(cell, U0, steps, dtype, **kw):
    k, lam, solver, _ = cell
    return pcr.fold_in(factors(k), fr.csr_args(users_of(solver)), lam, solver_type=solver, U0=U0, steps=steps, dtype=dtype, per_user=True, **kw)


def run(cmd, cwd):
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True)


# ------------------------------------------------------------------------------------------------------------------------------
# CPU part
# ------------------------------------------------------------------------------------------------------------------------------

def test_symbols_constants_and_fields():
    L = pcr.lib()
    assert hasattr(L, "pcr_fold_in_model") and hasattr(L, "pcr_fold_in")
    hdr = open(os.path.join(ROOT, "include", "primalcr.h")).read()
    for name, val in (("PCR_FOLDIN_WAVE_MAX", pcr.PCR_FOLDIN_WAVE_MAX), ("PCR_FOLDIN_LDS_MAX", pcr.PCR_FOLDIN_LDS_MAX),
                      ("PCR_FOLDIN_FIELDS", len(pcr.PCR_FOLDIN_FIELDS)),
                      ("PCR_FOLDIN_CONVERGED", 0), ("PCR_FOLDIN_STEP_CAP", 1), ("PCR_FOLDIN_STALLED", 2)):
        assert f"#define {name}" in hdr and int(hdr.split(f"#define {name}")[1].split()[0]) == val, name
    assert pcr.PCR_FOLDIN_FIELDS == ("steps", "cg", "ls", "obj", "gnorm2", "status")
    assert C.sizeof(pcr.FoldinStats) == 64
    b = pcr.foldin_boundaries()
    assert b == [pcr.PCR_FOLDIN_WAVE_MAX, pcr.PCR_FOLDIN_LDS_MAX] and set(b) | {x - 1 for x in b} | {x + 1 for x in b} <= set(lengths())


def test_argument_errors_come_before_any_device_and_name_the_entry():
    V = factors(7)
    idx, it, val = np.array([0, 2, 3], np.int64), np.array([5, 1, 7], np.int32), np.array([1.0, 2.0, 3.0])

    def refused(match, code=ERR_ARG, **kw):
        a = dict(V=V, ratings=(idx, it, val), lam=32.0)
        a.update(kw)
        with pytest.raises(pcr.PcrError, match=match) as e:
            pcr.fold_in(**a)
        assert f"error {code}:" in str(e.value) and "pcr_fold_in_model" in str(e.value), str(e.value)

    refused("outside", ratings=(idx, np.array([5, 1, D2], np.int32), val))
    refused("outside", ratings=(idx, np.array([5, -1, 7], np.int32), val))
    refused("not finite", ratings=(idx, it, np.array([1.0, np.nan, 3.0])))
    refused("not finite", ratings=(idx, it, np.array([1.0, np.inf, 3.0])))
    refused("monotone", ratings=(np.array([0, 3, 2, 3], np.int64), it, val))
    refused(r"index\[0\]", ratings=(np.array([1, 2, 3], np.int64), it, val))
    refused("steps", steps=0)
    refused("steps", steps=-3)
    refused("precision", dtype=7)
    refused("solver type", solver_type=3)
    refused("CCDR1", code=ERR_UNSUPPORTED, solver_type=pcr.PCR_SOLVER_CCDR1)
    many = np.arange(70000, dtype=np.float64)                       # more levels than the level builder's 16 bits (PrimalCR: raw doubles)
    big_V = np.zeros((70000, 2))
    with pytest.raises(pcr.PcrError, match="pcr_fold_in_model.*65535") as e:
        pcr.fold_in(big_V, (np.array([0, 70000], np.int64), np.arange(70000, dtype=np.int32), many), 1.0, solver_type=pcr.PCR_SOLVER_PCR)
    assert f"error {ERR_UNSUPPORTED}:" in str(e.value)
    with pytest.raises(ValueError):
        pcr.fold_in(V, (idx, it, val), 32.0, U0=np.zeros((3, 7)))
    p = pcr.Parameter(k=7)
    out = np.zeros((2, 7))
    L = pcr.lib()
    assert L.pcr_fold_in_model(C.byref(p), None, D2, 2, idx.ctypes.data, it.ctypes.data, val.ctypes.data, None, 1, out.ctypes.data, None, None) == ERR_ARG
    assert b"pcr_fold_in_model" in L.pcr_last_error()
    assert L.pcr_fold_in_model(C.byref(p), V.ctypes.data, D2, 2, idx.ctypes.data, it.ctypes.data, val.ctypes.data, None, 1, None, None, None) == ERR_ARG
    assert L.pcr_fold_in(None, 2, idx.ctypes.data, it.ctypes.data, val.ctypes.data, None, 1, out.ctypes.data, None, None) == ERR_ARG


def test_without_a_device_the_calls_fail_with_err_device():
    """Valid arguments on a process that sees no GPU: PCR_ERR_DEVICE (never a CPU path)."""
    code = ("import sys, numpy as np; sys.path.insert(0, sys.argv[1])\n"
            "import primalcr_amd as pcr\n"
            "try:\n"
            "    pcr.fold_in(np.ones((6, 3)), (np.array([0, 2, 2]), np.array([1, 4]), np.array([1.0, 2.0])), 1.0)\n"
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
    assert "omp-pmf-recommend --fold-in data_dir -l lambda [-s 1|2] [--steps S] [-K topk] [--f32] [--scores] model_file output_file\n" in r.stdout
    assert "omp-pmf-recommend --fold-in data_dir -l lambda [-s 1|2] [--steps S] --eval data_dir [-c ...] [--threshold v] [--f32] model_file [output_file]\n" in r.stdout
    (tmp_path / "users").write_text("1\n")
    for extra in (["-x", "d"], ["-u", "users"], ["--diversity"], ["--mmr", "0.5"], ["--tradeoff", "0,1"], ["--eval", "d", "--ranks"]):
        r = run([RECOMMEND, "--fold-in", "d", "-l", "1"] + extra + ["m", "o"], tmp_path)
        assert r.returncode == 1 and "--fold-in does not go with" in r.stderr, (extra, r.stderr)
    r = run([RECOMMEND, "--fold-in", "d", "m", "o"], tmp_path)
    assert r.returncode == 1 and "--fold-in needs -l" in r.stderr
    for bad in (["-l", "x"], ["-s", "0"], ["-s", "3"], ["--steps", "0"]):
        r = run([RECOMMEND, "--fold-in", "d"] + bad + ["m", "o"], tmp_path)
        assert r.returncode == 1 and bad[0] in r.stderr, (bad, r.stderr)
    r = run([RECOMMEND, "-l", "5", "m", "o"], tmp_path)
    assert r.returncode == 1 and "go with --fold-in" in r.stderr
    R = synth.generate("tiny", seed=3)                              # 60 x 40
    d = synth.write_dir(R, str(tmp_path / "data"))
    rng = np.random.default_rng(2)
    pcr.model_save(str(tmp_path / "wrong.model"), rng.standard_normal((5, 4)), rng.standard_normal((R.d2 + 1, 4)))
    r = run([RECOMMEND, "--fold-in", d, "-l", "1", "wrong.model", "out"], tmp_path)
    assert r.returncode == 1 and "items, the model" in r.stderr, r.stderr


@pytest.mark.parametrize("cell", CELLS, ids=CELL_IDS)
def test_fixture_preconditions_on_the_reference(oracle, cell):
    """What the GPU comparisons rest on, shown on the reference alone: steps 1 and 2 of every user with at least two levels
    accept their first try with a relative decrease >= 1e-12 (1000 x the fp64 noise of a converged step); |g|^2 is never within
    1e-6 (steps 1-3) of the 1e-4 threshold -- nor within 1e-3 at step 1, the fp32 exemption's width; the numpy objective agrees
    with the oracle's obj_u_new to 1e-9."""
    k, lam, solver, st = cell
    X = users_of(solver)
    s = ref_steps(oracle, cell, 3, numpy_too=True)
    nlev = np.array([fr.n_levels(X, i, solver) for i in range(X.d1)])
    for j in (0, 1):
        info = s[j][1]
        moved = (nlev >= 2) & (info["status"] == fr.STEP_CAP)
        if j == 0:
            assert moved[nlev >= 2].all(), "every user with two levels takes step 1"
        assert (info["ls"][moved] == 1).all(), (j, info["ls"][moved])
        dec = (info["obj0"][moved] - s[j + 1][1]["obj0"][moved]) / info["obj0"][moved]
        assert dec.min(initial=np.inf) >= 1e-12, (j, dec.min())                # (k = 1: most users have converged after one step)
        assert np.abs(info["obj"][moved] / s[j + 1][1]["obj0"][moved] - 1.0).max(initial=0.0) <= 1e-9
        assert (info["status"][nlev < 2] == fr.CONVERGED).all() or solver == 2
    for j in range(3):
        gn2 = s[j][1]["gn2"]
        assert np.abs(gn2 / 1e-4 - 1.0).min() > 1e-6, (j, gn2)
        assert ((gn2 < 1e-4) == (s[j][1]["status"] == fr.CONVERGED))[nlev >= 2].all()
    assert np.abs(s[0][1]["gn2"] / 1e-4 - 1.0).min() > 1e-3


LOOP_CELL = (12, 1.0, "dyadic")           # (k, lambda, start) of the tests of the whole loop: it has users of every end


def sub_users(X, users):
    n = np.diff(X.idx)
    return fr.CSR(len(users), D2, np.concatenate([[0], np.cumsum(n[users])]), np.concatenate([X.item[X.idx[i]:X.idx[i + 1]] for i in users]),
                  np.concatenate([X.val[X.idx[i]:X.idx[i + 1]] for i in users]))


def test_fixture_has_converged_and_stalled_users(oracle):
    """The reference's loop (PrimalCR++) on two cells: at least one user ends CONVERGED, and in each cell at least one long user
    ends STALLED within 6 steps (its gradient's noise floor is above the absolute threshold, and 20 tries find no strict
    decrease)."""
    X = users_of(2)
    n = np.diff(X.idx)
    long_users = [int(i) for i in np.nonzero(n >= 1000)[0]]
    for k, lam, st in (LOOP_CELL, (132, 32.0, "zero")):
        _, per, _ = fr.ref_fold_in(oracle, sub_users(X, long_users), factors(k), lam, 2, start(st, X.d1, k)[long_users], 6)
        assert (per["status"] == fr.STALLED).any(), (k, per["status"])
    short = [int(i) for i in np.nonzero((n > 2) & (n <= 129))[0]]
    k, lam, st = LOOP_CELL
    _, per, _ = fr.ref_fold_in(oracle, sub_users(X, short), factors(k), lam, 2, start(st, X.d1, k)[short], 10)
    assert (per["status"] == fr.CONVERGED).any()


# ------------------------------------------------------------------------------------------------------------------------------
# GPU part
# ------------------------------------------------------------------------------------------------------------------------------

def row_ratio(U, Uo, fac):
    return np.abs(U - Uo).max(1) / (fac * np.maximum(np.abs(Uo).max(1), 1e-3 * np.abs(Uo).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("cell", CELLS, ids=CELL_IDS)
def test_steps_one_and_two_match_the_oracle_in_fp64(oracle, cell):
    """fold_in(steps = 1) from U_prev against one oracle step from the same U_prev, for steps 1 and 2 (the device's own result is
    fed back): every row within 1e-7 of the oracle's row (the project's per-row bound), the CG and line-search counts equal,
    obj to 1e-11, status and steps as the reference says -- for every user of the cell."""
    k, lam, solver, st = cell
    X, V = users_of(solver), factors(k)
    U = start(st, X.d1, k)
    for j in (1, 2):
        Uo, info = fr.ref_step(oracle, X, V, lam, solver, U) if j == 2 else ref_steps(oracle, cell, 1)[0]
        Ug, stats, pu = foldin(cell, U, 1, pcr.PCR_F64)
        ratio = row_ratio(Ug, Uo, FP64_ROW)
        print(f"[foldin] {cell} step {j}: largest per-row |dU| / bound = {ratio.max():.3e} (user {ratio.argmax()}, len {np.diff(X.idx)[ratio.argmax()]})")
        assert ratio.max() <= 1.0, (j, int(ratio.argmax()), ratio.max())
        assert np.array_equal(pu[:, 1], info["cg"]) and np.array_equal(pu[:, 2], info["ls"]), (j, pu[:, 1:3].T, info["cg"], info["ls"])
        assert np.array_equal(pu[:, 5], info["status"]), (j, pu[:, 5], info["status"])
        assert np.array_equal(pu[:, 0], (info["status"] == fr.STEP_CAP).astype(float))
        rel = np.abs(pu[:, 3] - info["obj"]) / np.maximum(np.abs(info["obj"]), 1e-300)
        assert rel[info["obj"] != 0].max(initial=0.0) <= 1e-11 and (pu[info["obj"] == 0, 3] == 0).all(), (j, rel.max())
        U = Ug


@pytest.mark.gpu
@pytest.mark.parametrize("cell", CELLS, ids=CELL_IDS)
def test_step_one_matches_the_oracle_in_fp32(oracle, cell):
    """Step 1 in fp32 storage, to the project's 5e-3 per-row bound; a user whose reference |g|^2 at the start is within 1e-3 of
    the 1e-4 threshold would be exempt from the status comparison (2.5 x the project's fp32 g tolerance, squared up) -- the CPU
    part shows that the fixture has none."""
    k, lam, solver, st = cell
    X = users_of(solver)
    Uo, info = ref_steps(oracle, cell, 1)[0]
    Ug, stats, pu = foldin(cell, start(st, X.d1, k), 1, pcr.PCR_F32)
    ratio = row_ratio(Ug, Uo, FP32_ROW)
    print(f"[foldin] {cell} fp32 step 1: largest per-row |dU| / bound = {ratio.max():.3e} (user {ratio.argmax()})")
    assert ratio.max() <= 1.0, (int(ratio.argmax()), ratio.max())
    assert np.array_equal(pu[:, 5], info["status"]), (pu[:, 5], info["status"])
    assert np.array_equal(Ug.astype(np.float32).astype(np.float64), Ug)        # the storage type's values, widened


@pytest.mark.gpu
@pytest.mark.parametrize("r", [12, 100])
@pytest.mark.parametrize("pname", ["F32", "F64"])
def test_first_step_on_the_dyadic_case(oracle, pname, r):
    """On the dyadic case of tests/exact_data.py (V and the scores at the start are exact in both types) fold_in(U0 = c.U,
    steps = 1) against oracle.update_U_new, by test_exact_parity's method for update_U: per row, the project's bound; in fp64
    the inner counts equal the oracle's."""
    from test_exact_parity import TOL, oracle_steps, reference
    c = reference(oracle, r, 2)
    Uo, _, iu, _, _ = oracle_steps(oracle, r)
    Ug, stats, pu = pcr.fold_in(c.V, fr.csr_args(c.X), c.lam, U0=c.U, steps=1, dtype=PREC[pname], per_user=True)
    moved = pu[:, 5] != fr.STALLED                                   # (a stalled user stays; the oracle's moves on, quirk q5)
    ratio = row_ratio(Ug, Uo, TOL[PREC[pname]]["fac"])
    print(f"[foldin] dyadic {pname} r={r}: largest per-row |dU| / bound = {ratio[moved].max():.3e}; stalled users {int((~moved).sum())}")
    assert ratio[moved].max() <= 1.0
    assert (pu[~moved, 2] == 20).all() and np.array_equal(Ug[~moved], c.U[~moved].astype(np.float32 if pname == "F32" else np.float64))
    if pname == "F64":
        assert (stats["cg"], stats["ls"]) == (iu["cg"], iu["ls"])


@pytest.mark.gpu
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("pname", ["F32", "F64"])
def test_the_loop_is_its_own_single_steps(pname, solver):
    """fold_in(steps = S), S = 2, 3, 6, is bit for bit what S chained calls of steps = 1 return, each from the last one's
    output, a user stopping at its first status other than STEP_CAP: U, steps, cg, ls, obj and status."""
    cell = (LOOP_CELL[0], LOOP_CELL[1], solver, LOOP_CELL[2])
    X = users_of(solver)
    U = start(cell[3], X.d1, cell[0])
    done = np.zeros(X.d1, bool)
    tot = np.zeros((X.d1, 6))
    seen = set()
    for s in range(1, 7):
        Un, _, pu = foldin(cell, U, 1, PREC[pname])
        live = ~done
        U = np.where(live[:, None], Un, U)
        tot[live, :3] += pu[live, :3]
        tot[live, 3:] = pu[live, 3:]
        done |= pu[:, 5] != fr.STEP_CAP
        if s in (2, 3, 6):
            Us, st, ps = foldin(cell, start(cell[3], X.d1, cell[0]), s, PREC[pname])
            assert np.array_equal(Us, U), (s, np.nonzero((Us != U).any(1))[0])
            assert np.array_equal(ps[:, [0, 1, 2, 3, 5]], tot[:, [0, 1, 2, 3, 5]]), s
            seen |= set(ps[:, 5].astype(int).tolist())
    assert fr.CONVERGED in seen and (fr.STALLED in seen or pname == "F64")      # (fp32 reaches its noise floor within six steps)


_FULL, _START_OBJ = {}, {}


def full_reference(oracle, solver):
    if solver not in _FULL:
        X = users_of(solver)
        k, lam, st = LOOP_CELL
        _FULL[solver] = fr.ref_fold_in(oracle, X, factors(k), lam, solver, start(st, X.d1, k), 10)
    return _FULL[solver]


@pytest.mark.gpu
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("pname", ["F32", "F64"])
def test_properties_of_a_full_run(oracle, pname, solver):
    """steps = 10: no user ends above the objective it started from (numpy); obj is the numpy objective at the returned row; a
    CONVERGED user's numpy gradient is below the threshold; a STALLED user stopped short of the cap at an objective no larger
    than one step earlier; every user's final objective is the emulated reference's; the summary is the per-user table's sums."""
    k, lam, st0 = LOOP_CELL
    cell = (k, lam, solver, st0)
    X, V = users_of(solver), factors(k)
    f64 = pname == "F64"
    U0 = start(st0, X.d1, k)
    Ug, stats, pu = foldin(cell, U0, 10, PREC[pname])
    Ur, per, _ = full_reference(oracle, solver)
    for i in range(X.d1):
        Vr, val = fr.user_rows(X, V, i)
        o_out, g = fr.pair_obj_grad(Ug[i], Vr, val, lam, solver)
        o_in = _START_OBJ.setdefault((solver, i), fr.pair_obj_grad(U0[i], Vr, val, lam, solver, False)[0]) if (solver, i) not in _START_OBJ else _START_OBJ[(solver, i)]
        assert o_out <= o_in, (i, o_out, o_in)
        assert abs(pu[i, 3] - o_out) <= (1e-10 if f64 else FP32_OBJ) * abs(o_out), (i, pu[i, 3], o_out)
        if f64 and pu[i, 5] == fr.CONVERGED and Vr.shape[0] and (solver == 2 or fr.n_levels(X, i, solver) >= 2):
            assert float(g @ g) < 1e-4 * (1 + 1e-6), (i, float(g @ g))
        if pu[i, 5] == fr.STALLED:                                  # a point it was at before a step: that of steps - 1 more single steps
            assert pu[i, 0] < 10
        assert abs(pu[i, 3] - per["obj"][i]) <= (1e-9 if f64 else 1e-3) * abs(per["obj"][i]), (i, pu[i, 3], per["obj"][i])
    stalled = np.nonzero((pu[:, 5] == fr.STALLED) & (pu[:, 0] >= 1))[0]
    for sb in np.unique(pu[stalled, 0].astype(int) - 1):            # ... and obj <= the previous step's: the run capped one step earlier
        if sb >= 1:
            _, _, pb = foldin(cell, U0, int(sb), PREC[pname])
            mine = stalled[pu[stalled, 0].astype(int) - 1 == sb]
            assert (pu[mine, 3] <= pb[mine, 3]).all(), (sb, pu[mine, 3], pb[mine, 3])
    assert stats["users"] == X.d1 and stats["converged"] == int((pu[:, 5] == 0).sum()) and stats["step_cap"] == int((pu[:, 5] == 1).sum())
    assert stats["stalled"] == int((pu[:, 5] == 2).sum()) and stats["steps"] == int(pu[:, 0].sum()) and stats["cg"] == int(pu[:, 1].sum())
    assert stats["ls"] == int(pu[:, 2].sum())
    acc = 0.0
    for v in pu[:, 3]:
        acc += v
    assert stats["obj"] == acc


@pytest.mark.gpu
@pytest.mark.parametrize("pname", ["F32", "F64"])
def test_determinism_and_independence(pname):
    cell = (12, 1.0, 2, "dyadic")
    X, V = users_of(2), factors(12)
    idx, it, val = fr.csr_args(X)
    U0 = start("dyadic", X.d1, 12)
    kw = dict(lam=1.0, steps=10, dtype=PREC[pname], per_user=True)
    Ua, sa, pa = pcr.fold_in(V, (idx, it, val), U0=U0, **kw)
    Ub, sb, pb = pcr.fold_in(V, (idx, it, val), U0=U0, **kw)
    assert np.array_equal(Ua, Ub) and np.array_equal(pa, pb) and sa == sb

    def subset(users, reverse_items=False):
        ii = np.concatenate([[0], np.cumsum(np.diff(idx)[users])]).astype(np.int64)
        sl = [np.arange(idx[u], idx[u + 1])[::-1 if reverse_items else 1] for u in users]
        sel = np.concatenate(sl) if sl else np.zeros(0, np.int64)
        return pcr.fold_in(V, (ii, it[sel], val[sel]), U0=U0[users], **kw)

    n = X.d1
    for u in (4, 9, 12, int(np.argmax(np.diff(idx) == pcr.PCR_FOLDIN_LDS_MAX + 1)), n - 1):
        for users in ([u], [u] + [v for v in range(0, n, 3) if v != u], [v for v in range(1, n, 4) if v != u] + [u]):
            U1, _, p1 = subset(np.array(users))
            at = users.index(u)
            assert np.array_equal(U1[at], Ua[u]) and np.array_equal(p1[at], pa[u]), (u, len(users))
    perm = np.random.default_rng(3).permutation(n)
    Up, sp, pp = subset(perm)
    assert np.array_equal(Up, Ua[perm]) and np.array_equal(pp, pa[perm])
    Ud, sd, pd = subset(np.arange(n), reverse_items=True)           # rows given item-descending
    assert np.array_equal(Ud, Ua) and np.array_equal(pd, pa)


def _trained(tmp_path=None, prec=pcr.PCR_F64):
    R = synth.generate("small", seed=31, d1=300, d2=400, nnz=300 * 40)
    ds = pcr.Dataset.from_ratings(R)
    return R, ds


@pytest.mark.gpu
@pytest.mark.parametrize("pname", ["F32", "F64"])
def test_solver_entry(pname):
    """Solver.fold_in equals fold_in(V, ...) with the solver's parameters bit for bit, and leaves the solver as a twin that never
    folded anything in."""
    R, ds = _trained()
    k, lam = 8, 50.0
    rng = np.random.default_rng(9)
    U, V = 0.3 * rng.standard_normal((R.d1, k)), 0.3 * rng.standard_normal((R.d2, k))
    X = users_of(2)
    sub = (X.idx[:24], X.item[:X.idx[23]].astype(np.int32) % R.d2, X.val[:X.idx[23]])      # (duplicated items: two ratings each)
    for solver in (2, 1):
        prm = dict(k=k, precision=PREC[pname], solver_type=solver, **{"lambda": lam})
        a, b = pcr.Solver(ds, pcr.Parameter(**prm)), pcr.Solver(ds, pcr.Parameter(**prm))
        a.set_factors(U, V); b.set_factors(U, V)
        Us, ss, ps = a.fold_in(sub, steps=5, per_user=True)
        Um, sm, pm = pcr.fold_in(V, sub, lam, solver_type=solver, steps=5, dtype=PREC[pname], per_user=True)
        assert np.array_equal(Us, Um) and np.array_equal(ps, pm) and ss == sm
        Ua, Va = a.get_factors(); Ub, Vb = b.get_factors()
        assert np.array_equal(Ua, Ub) and np.array_equal(Va, Vb)
        ra, rb = a.iterate(1), b.iterate(1)
        key = ("obj", "cg_v", "ls_v", "cg_u", "ls_u")
        assert [[x[f] for f in key] for x in ra] == [[x[f] for f in key] for x in rb]
        assert all(np.array_equal(x, y) for x, y in zip(a.get_factors(), b.get_factors()))
        a.close(); b.close()
    c = pcr.Solver(ds, pcr.Parameter(k=k, solver_type=pcr.PCR_SOLVER_CCDR1, **{"lambda": lam}))
    with pytest.raises(pcr.PcrError, match=f"error {ERR_STATE}:.*pcr_fold_in"):
        c.fold_in(sub)
    c.close()


@pytest.mark.gpu
def test_end_to_end(tmp_path):
    """Train 3 iterations, fold the training users themselves back in from zero: the fold-in optimises what the U step only
    stepped toward; recommend_new_users and the CLI's --fold-in give the lists and metrics of the Python calls."""
    R, ds = _trained()
    d = synth.write_dir(R, str(tmp_path / "data"))
    k, lam = 8, 50.0
    s = pcr.Solver(ds, pcr.Parameter(k=k, precision=pcr.PCR_F64, **{"lambda": lam}))
    s.set_factors(pcr.initial(R.d1, k), pcr.initial(R.d2, k))
    s.iterate(3)
    U, V = s.get_factors()
    s.close()
    idx, it, val = ds.csr(0)
    Un, stats, pu = pcr.fold_in(V, ds, lam, steps=10, per_user=True)
    for i in range(R.d1):
        Vr, v = V[it[idx[i]:idx[i + 1]]], val[idx[i]:idx[i + 1]]
        o_new, o_tr = fr.pair_obj_grad(Un[i], Vr, v, lam, 2, False)[0], fr.pair_obj_grad(U[i], Vr, v, lam, 2, False)[0]
        assert o_new <= o_tr * (1 + 1e-9), (i, o_new, o_tr)
    items, scores, U2, st2 = pcr.recommend_new_users(V, ds, lam, 10)
    ri, rs = pcr.recommend(Un, V, 10, exclude=ds)
    assert np.array_equal(U2, Un) and st2 == stats and np.array_equal(items, ri) and np.array_equal(scores, rs)
    pcr.model_save(str(tmp_path / "m.model"), U, V)
    r = run([RECOMMEND, "--fold-in", d, "-l", str(lam), "m.model", "lists.txt"], tmp_path)
    assert r.returncode == 0, r.stderr
    want = ("foldin users %d converged %d step_cap %d stalled %d steps %d cg %d ls %d obj %s" %
            (stats["users"], stats["converged"], stats["step_cap"], stats["stalled"], stats["steps"], stats["cg"], stats["ls"], "%g" % stats["obj"]))
    assert r.stdout.splitlines() == [want]
    lines = open(tmp_path / "lists.txt").read().splitlines()
    assert lines == [" ".join([str(u + 1)] + [str(j + 1) for j in row if j >= 0]) for u, row in enumerate(ri)]
    r = run([RECOMMEND, "--fold-in", d, "-l", str(lam), "--eval", d, "-c", "5,10", "m.model"], tmp_path)
    assert r.returncode == 0, r.stderr
    ev = pcr.evaluate_topn(Un, V, ds, cutoffs=(5, 10), exclude=ds)
    out = r.stdout.splitlines()
    assert out[0] == want and len(out) == 3
    for line, e in zip(out[1:], ev):
        f = line.split()
        assert f[0] == "cutoff" and int(f[1]) == e["cutoff"] and int(f[3]) == e["users"] and int(f[7]) == e["hits"]
        assert f[9] == "%g" % e["precision"] and f[11] == "%g" % e["recall"] and f[17] == "%g" % e["ndcg"], (line, e)
