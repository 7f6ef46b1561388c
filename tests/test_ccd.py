"""CCDR1 (solver type 0, ccd-r1.cpp:97-212) on the device: C ABI, CLI and Python binding.

CPU part: initial_col against libc's drand48, the default settings, the CLI's refusals and usage text.
GPU part (-m gpu): omp-pmf-train -s 0 against the reference binary's golden runs (tests/golden/ccd_*, made by
tools/make_ccd_golden.py), fp32 against fp64, determinism and invariants, and two larger shapes.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from ccd_data import ratings
from conftest import BIN_DIR, ROOT
from primalcr_amd import synth

TRAIN = os.path.join(BIN_DIR, "omp-pmf-train")
PREDICT = os.path.join(BIN_DIR, "omp-pmf-predict")
REF_TRAIN = os.path.join(ROOT, "oracle", "_ref", "omp-pmf-train")
GOLDEN = os.path.join(ROOT, "tests", "golden")
CCD_SETS = ["edge5", "real", "mid5", "synth3", "synth4", "unsorted", "long"]

LINE = re.compile(r"iter (\d+) rank (\d+) time (\S+) loss (\S+) obj (\S+) diff (\S+) gnorm (\S+) reg (\S+) "
                  r"(?:rmse (\S+)\(Testing\) pairwise error (\S+) NDCG (\S+))?$")


def run(cmd, cwd):
    return subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=600)


# ---------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("n,k", [(37, 5), (250000, 10)])        # 185 values (one thread), 2.5 M (several, jump-ahead)
def test_initial_col_equals_libc_drand48(n, k):
    import primalcr_amd as pcr
    X = pcr.initial_col(n, k)
    # libc's own unseeded stream, in a fresh process (its state is global to the process)
    code = ("import ctypes, sys\n"
            "import numpy as np\n"
            "c = ctypes.CDLL(None); c.drand48.restype = ctypes.c_double\n"
            f"a = np.fromiter((0.1 * c.drand48() for _ in range({n * k})), np.float64, {n * k})\n"
            "sys.stdout.buffer.write(a.tobytes())\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, check=True, timeout=300).stdout
    ref = np.frombuffer(out, np.float64)
    assert X.shape == (n, k)
    assert np.array_equal(X.ravel().view(np.uint64), ref.view(np.uint64))
    assert X[0, 0] == 0.1 * 11 * 2.0 ** -48                         # state 0, not POSIX's 0x1234ABCD330E


def test_ccd_params_default():
    import primalcr_amd as pcr
    p = pcr.CcdParameter()
    assert (p.maxinneriter, p.eps, p.do_nmf) == (5, 1e-3, 0)        # pmf.h:36,39,47
    q = pcr.CcdParameter(maxinneriter=2, do_nmf=1)
    assert (q.maxinneriter, q.eps, q.do_nmf) == (2, 1e-3, 1)


@pytest.mark.parametrize("extra,flag", [(["--gpus", "2"], "--gpus"), (["--init-model", "m0"], "--init-model"),
                                        (["--snapshot-every", "1"], "--snapshot-every"), (["--devices", "0,1"], "--devices")])
def test_cli_s0_refuses_what_ccdr1_does_not_have(extra, flag, tmp_path):
    """Refused with exit 1 and one line, before a data set is read or a device touched (the data directory does not exist)."""
    r = run([TRAIN, "-s", "0"] + extra + [str(tmp_path / "no_data"), str(tmp_path / "m.model")], tmp_path)
    assert r.returncode == 1
    assert flag in r.stderr and "-s 0" in r.stderr and len(r.stderr.strip().splitlines()) == 1
    assert "can't open" not in r.stderr


def test_usage_text_lists_the_ccdr1_options(tmp_path):
    r = run([TRAIN], tmp_path)
    assert r.returncode == 1 and r.stdout.startswith("Usage: omp-pmf-train [options] data_dir [model_filename]")
    for flag in ("-s type", "-k rank", "-n threads", "-l lambda", "-t max_iter", "-p do_predict", "--cache file", "--snapshot-every n",
                 "0 -- CCDR1", "-T max_iter", "-e epsilon", "-N do_nmf"):
        assert flag in r.stdout


# ---------------------------------------------------------------------------------------------------------------- GPU
def ccd_golden(name):
    meta = json.load(open(os.path.join(GOLDEN, "ccd_" + name + ".json")))
    return meta["cases"], np.load(os.path.join(GOLDEN, "ccd_" + name + ".npz"))


def read_model(path):
    raw = open(path, "rb").read()
    d1, k = np.frombuffer(raw, np.int64, 2, 0)
    o = 16
    U = np.frombuffer(raw, np.float64, d1 * k, o).reshape(d1, k); o += 8 * d1 * k
    d2, k2 = np.frombuffer(raw, np.int64, 2, o); o += 16
    return U, np.frombuffer(raw, np.float64, d2 * k2, o).reshape(d2, k2)


def parse(stdout):
    """stdout of a -s 0 run -> (head, per-rank records, tail); every line accounted for."""
    lines = stdout.rstrip("\n").split("\n")
    assert lines[0] == "starts!" and lines[-1].startswith("Wall-time: ") and lines[-1].endswith(" secs"), stdout[-300:]
    recs = []
    for ln in lines[1:-1]:
        m = LINE.match(ln)
        assert m, repr(ln)
        g = m.groups()
        recs.append((int(g[0]), int(g[1])) + tuple(float(x) if x is not None else None for x in g[2:]))
    return recs


def compare_lines(ours, ref, rtol=2e-5):
    """Same (iter, rank) sequence; loss, obj, reg, rmse to rtol; diff to rtol of obj; NDCG / pairwise error (printed %lf) to the
    print resolution plus rtol; time masked."""
    a, b = parse(ours), parse(ref)
    assert [r[:2] for r in a] == [r[:2] for r in b]
    for x, y in zip(a, b):
        for i in (3, 4, 7):                                           # loss, obj, reg
            assert x[i] == pytest.approx(y[i], rel=rtol, abs=1e-12), (x, y)
        assert abs(x[5] - y[5]) <= rtol * abs(y[4]) + 1e-12, (x, y)   # diff
        assert x[6] == y[6] == 0.0                                    # gnorm (never computed by the reference)
        assert (x[8] is None) == (y[8] is None)
        if y[8] is not None:
            assert x[8] == pytest.approx(y[8], rel=rtol), (x, y)      # rmse
            assert abs(x[9] - y[9]) <= 2e-6 + rtol and abs(x[10] - y[10]) <= 2e-6 + rtol, (x, y)
    return a


def run_ours(name, args, tmp_path, f64=True, tag="ours"):
    d = os.path.join(str(tmp_path), "data")
    if not os.path.exists(d):
        synth.write_dir(ratings(name), d)
    model = os.path.join(str(tmp_path), tag + ".model")
    r = run([TRAIN] + args + (["--f64"] if f64 else []) + [d, model], tmp_path)
    assert r.returncode == 0, r.stderr
    return r.stdout, model, d


GOLDEN_RUNS = [(n, t) for n in CCD_SETS for t in ccd_golden(n)[0]]


@pytest.mark.gpu
@pytest.mark.parametrize("name,tag", GOLDEN_RUNS)
def test_cli_s0_matches_the_reference(name, tag, tmp_path):
    """-s 0 --f64 against the reference binary: the same per-rank lines, the model to 1e-7, predictions to 2e-6."""
    cases, g = ccd_golden(name)
    args = cases[tag]["args"]
    out, model, d = run_ours(name, args, tmp_path)
    recs = compare_lines(out, cases[tag]["stdout"])
    assert "the rank is" not in out and "nnz" not in out
    assert not os.path.exists(tmp_path / "U.txt") and not os.path.exists(tmp_path / "V.txt")
    U, V = read_model(model)

    def same_model(Ur, Vr):
        assert U.shape == Ur.shape and V.shape == Vr.shape
        if tag == "t0":                                               # no iteration: W = initial_col, H = 0, bit for bit
            assert np.array_equal(U, Ur) and np.array_equal(V, Vr) and not V.any()
            assert recs == []
        else:
            assert np.abs(U - Ur).max() <= 1e-7 * np.abs(Ur).max(), np.abs(U - Ur).max()
            assert np.abs(V - Vr).max() <= 1e-7 * max(np.abs(Vr).max(), 1e-300), np.abs(V - Vr).max()
    if "U_" + tag in g.files:                                         # (models are stored for the base runs and -t 0)
        same_model(g["U_" + tag], g["V_" + tag])
    pred = os.path.join(str(tmp_path), "pred.txt")
    r = run([PREDICT, os.path.join(d, "test.ratings"), model, pred], tmp_path)
    assert r.returncode == 0, r.stderr
    # the reference's predictions are stored as the integers of its %lf text (micro-units)
    assert np.abs(np.loadtxt(pred, ndmin=1) - g["pred_" + tag] * 1e-6).max() <= 2e-6
    if name == "unsorted":                                            # the raw test triplets survive the binary cache
        for rnd in ("write", "read"):
            cache = os.path.join(str(tmp_path), "ds.cache")
            r = run([TRAIN] + args + ["--f64", "--cache", cache, d, os.path.join(str(tmp_path), "c.model")], tmp_path)
            assert r.returncode == 0 and os.path.exists(cache), r.stderr
            assert [x[:2] + x[3:] for x in parse(r.stdout)] == [x[:2] + x[3:] for x in recs], rnd
    if tag == "e05":                                                # ranks skipped after five first-iteration breaks
        assert len(recs) < 3 * 8
    if os.path.exists(REF_TRAIN):                                     # the live reference: its golden run, and the model of every case
        r = run([REF_TRAIN] + args + [d, os.path.join(str(tmp_path), "ref.model")], tmp_path)
        assert r.returncode == 0
        compare_lines(r.stdout, cases[tag]["stdout"], rtol=1e-12)
        same_model(*read_model(os.path.join(str(tmp_path), "ref.model")))


@pytest.mark.gpu
def test_fp32_agrees_with_fp64(tmp_path):
    cases, _ = ccd_golden("mid5")
    args = cases["base"]["args"]
    a = parse(run_ours("mid5", args, tmp_path, f64=True, tag="f64")[0])
    b = parse(run_ours("mid5", args, tmp_path, f64=False, tag="f32")[0])
    assert [r[:2] for r in a] == [r[:2] for r in b]
    for x, y in zip(a, b):
        assert abs(x[4] - y[4]) <= 1e-3 * abs(x[4])                   # obj
        assert abs(x[9] - y[9]) <= 1e-3 and abs(x[10] - y[10]) <= 1e-3    # pairwise error, NDCG


def _solver(R, k, f64=True, **kw):
    import primalcr_amd as pcr
    ds = pcr.Dataset.from_ratings(R)
    p = pcr.Parameter(solver_type=pcr.PCR_SOLVER_CCDR1, k=k, precision=pcr.PCR_F64 if f64 else pcr.PCR_F32, **kw)
    s = pcr.Solver(ds, p)
    s.set_factors(pcr.initial_col(R.d1, k), None)
    return s


@pytest.mark.gpu
def test_abi_determinism_invariants_and_state_errors():
    import primalcr_amd as pcr
    R = ratings("mid5")
    outs = []
    for _ in range(2):
        s = _solver(R, 8, maxiter=3, do_predict=1, verbose=1, **{"lambda": 0.05})
        s.set_ccd_params(maxinneriter=5, eps=1e-3)
        recs, lines = s.train()
        assert s.counter("ccd_residual_mismatch") == 0
        U, V = s.get_factors()
        outs.append((U, V, [re.sub(r"time \S+ ", "", ln) for ln in lines]))
        assert recs[3]["cg_u"] > 0 and recs[3]["cg_v"] >= recs[3]["cg_u"] and recs[3]["seconds"] > 0
        for fn, args in ((s.comp_m, ()), (s.objective, ()), (s.obtain_g, ()), (s.update_V, ()), (s.update_U, ()),
                         (s.compute_Ha, (np.zeros((R.d2, 8)),)), (s.solve_delta, (np.zeros((R.d2, 8)),))):
            with pytest.raises(pcr.PcrError, match="error -6"):
                fn(*args)
        # pcr_iterate continues the run: the objective keeps falling, one record per outer iteration
        it = s.iterate(2)
        assert len(it) == 2 and it[1]["obj"] <= it[0]["obj"] <= recs[3]["obj"] * (1 + 1e-12)
        assert s.counter("ccd_residual_mismatch") == 0
        s.close()
    assert np.array_equal(outs[0][0].view(np.uint64), outs[1][0].view(np.uint64))
    assert np.array_equal(outs[0][1].view(np.uint64), outs[1][1].view(np.uint64))
    assert outs[0][2] == outs[1][2]
    # more than one rank: unsupported
    ds = pcr.Dataset.from_ratings(R)
    with pytest.raises(pcr.PcrError, match="error -7"):
        pcr.Solver(ds, pcr.Parameter(solver_type=0, k=4), rank=0, nranks=2)


@pytest.mark.gpu
def test_profile_slots_and_iterate_without_a_host_round_trip_per_rank():
    R = ratings("synth3")
    s = _solver(R, 6, maxiter=1, do_predict=0, verbose=0, **{"lambda": 0.05})
    s.profile(True)
    rec = s.iterate(1)[0]
    prof = s.profile_all()
    for slot in ("ccd/init", "ccd/begin", "ccd/vsweep", "ccd/usweep", "ccd/decide", "ccd/resid", "ccd/final"):
        assert slot in prof and prof[slot][1] > 0, prof
    assert prof["ccd/vsweep"][1] == prof["ccd/usweep"][1] == 6 * 5 and prof["ccd/resid"][1] == 6
    assert rec["cg_u"] == 6 and 6 <= rec["cg_v"] <= 30
    # recommend() and evaluate_topn() are timed in this solver's own profile (not in the PrimalCR++ solver it holds)
    s.recommend(10)
    s.evaluate_topn((5, 10))
    prof = s.profile_all()
    for slot in ("recommend/score", "recommend/merge", "recommend/metrics"):
        assert slot in prof and prof[slot][1] > 0, prof
    s.close()


def _objective_never_increases(lines, rtol=1e-12):
    recs = [parse_line(ln) for ln in lines]
    assert recs
    for r in recs[1:]:                                                # (the first line's diff is -obj: oldobj starts at 0, :109)
        assert r[5] >= -rtol * abs(r[4]), r
    return recs


def parse_line(ln):
    m = LINE.match(ln)
    assert m, ln
    return (int(m.group(1)), int(m.group(2))) + tuple(float(x) if x is not None else None for x in m.groups()[2:])


@pytest.mark.gpu
def test_ml1m_shape_against_the_reference(tmp_path):
    """The ml1m shape, -k 100 -t 2 -l 0.05 --f64 (lines without evaluation: -p 0 -q 1): lines and model against the reference
    binary run live (16 threads); the objective never increases."""
    if not os.path.exists(REF_TRAIN):
        pytest.skip("the reference binary is built by oracle/Makefile where the reference sources are present")
    R = synth.generate("ml1m", seed=7)
    d = synth.write_dir(R, str(tmp_path / "data"))
    args = ["-s", "0", "-k", "100", "-t", "2", "-l", "0.05", "-p", "0", "-q", "1"]
    r = run([REF_TRAIN] + args + ["-n", "16", d, str(tmp_path / "ref.model")], tmp_path)
    assert r.returncode == 0
    o = run([TRAIN] + args + ["--f64", d, str(tmp_path / "ours.model")], tmp_path)
    assert o.returncode == 0, o.stderr
    recs = compare_lines(o.stdout, r.stdout)
    assert all(x[5] >= -1e-12 * abs(x[4]) for x in recs[1:])       # (the first line's diff is -obj)
    U, V = read_model(str(tmp_path / "ours.model"))
    Ur, Vr = read_model(str(tmp_path / "ref.model"))
    assert np.abs(U - Ur).max() <= 1e-7 * np.abs(Ur).max() and np.abs(V - Vr).max() <= 1e-7 * np.abs(Vr).max()


@pytest.mark.gpu
def test_netflix_shaped_slice_completes_and_f32_agrees():
    """A Netflix-shaped slice (long-tailed items, a few million ratings): the run completes, the objective never increases
    (lines without evaluation), fp32 agrees with fp64."""
    R = synth.generate_fast("netflix", seed=11, d1=24000, nnz=3_000_000)
    objs = {}
    for f64 in (True, False):
        s = _solver(R, 16, f64=f64, maxiter=2, do_predict=0, verbose=1, **{"lambda": 0.05})
        _, lines = s.train()
        recs = _objective_never_increases(lines) if f64 else [parse_line(ln) for ln in lines]
        assert s.counter("ccd_residual_mismatch") == 0
        objs[f64] = [r[4] for r in recs]
        s.close()
    assert len(objs[True]) == len(objs[False])
    assert np.allclose(objs[False], objs[True], rtol=1e-3)
