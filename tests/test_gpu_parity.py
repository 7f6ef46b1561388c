"""GPU parity tests (run with -m gpu on an MI355X): the HIP path, called through the C ABI
(libprimalcr.so via primalcr_amd.api), against the CPU oracle on the same inputs and against the
committed golden vectors of the unmodified reference.

Tolerances (written here, as the north star asks): PCR_F64 runs the reference's arithmetic type and
must agree to summation-order rounding; PCR_F32 stores U, V, m and the CG vectors in fp32 (fp64
accumulation) and must agree to fp32 tolerance.
"""
import re

import numpy as np
import pytest

import primalcr_amd as pcr
from conftest import GOLDEN_CASES, load_golden
from primalcr_amd import synth

pytestmark = pytest.mark.gpu

TOL = {
    pcr.PCR_F64: dict(m=1e-13, obj=1e-11, vec=1e-10, cg=1e-7, fac=1e-7),
    pcr.PCR_F32: dict(m=2e-6, obj=2e-5, vec=2e-4, cg=5e-3, fac=5e-3),
}
NUM = r"[-+]?(?:\d+\.?\d*|\.\d+)(?:e[-+]?\d+)?"


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)) if a.size else 0.0


def make_solver(g, precision, solver=2, **kw):
    ds = pcr.Dataset.from_triplets(int(g["d1"]), int(g["d2"]), g["user"], g["item"], g["val"],
                                   g["tuser"], g["titem"], g["tval"])
    p = pcr.Parameter(k=int(g["r"]), solver_type=solver, precision=precision, **{"lambda": float(g["lam"])}, **kw)
    return pcr.Solver(ds, p)


@pytest.mark.parametrize("precision", [pcr.PCR_F64, pcr.PCR_F32])
@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_v_side_vs_golden(name, precision):
    g, _ = load_golden(name)
    t = TOL[precision]
    s = make_solver(g, precision)
    s.set_factors(g["U0"], g["V0"])
    m = s.comp_m()
    assert rel(m, g["m"]) < t["m"]
    assert abs(s.objective() / float(g["obj"]) - 1) < t["obj"]
    assert rel(s.obtain_g(), g["g"]) < t["vec"]
    assert rel(s.compute_Ha(g["a"]), g["Ha"]) < t["vec"]
    delta, its = s.solve_delta(g["g"])
    assert rel(delta, g["delta"]) < t["cg"]
    # update_V_new: V, objective and the m handed to the U step
    s.set_factors(g["U0"], g["V0"])
    objV, info = s.update_V()
    assert info["accepted"] == 1
    assert abs(objV / float(g["objV"]) - 1) < max(t["obj"], t["cg"] * 1e-2)
    _, V1 = s.get_factors()
    assert rel(V1, g["V1"]) < t["fac"]


@pytest.mark.parametrize("precision", [pcr.PCR_F64, pcr.PCR_F32])
@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_u_side_vs_golden(name, precision):
    g, _ = load_golden(name)
    t = TOL[precision]
    s = make_solver(g, precision)
    s.set_factors(g["U0"], g["V1"])        # update_U_new(X, m1, ..., V1, U0): m1 = scores of (U0, V1)
    s.comp_m(want=False)
    objU, info = s.update_U()
    U1, _ = s.get_factors()
    assert rel(U1, g["U1"]) < t["fac"]
    assert abs(objU / float(g["objU"]) - 1) < max(t["obj"], t["fac"] * 1e-2)
    assert info["ls"] >= 1


@pytest.mark.parametrize("precision", [pcr.PCR_F64, pcr.PCR_F32])
@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_solver1_vs_golden(name, precision):
    g, _ = load_golden(name)
    t = TOL[precision]
    s = make_solver(g, precision, solver=1)
    s.set_factors(g["U0"], g["V0"])
    s.comp_m(want=False)
    assert abs(s.objective() / float(g["obj_s1"]) - 1) < t["obj"]
    assert rel(s.obtain_g(), g["g_s1"]) < t["vec"]
    assert rel(s.compute_Ha(g["a"]), g["Ha_s1"]) < t["vec"]


@pytest.mark.parametrize("precision", [pcr.PCR_F64, pcr.PCR_F32])
@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_evaluator_vs_golden(name, precision):
    g, _ = load_golden(name)
    s = make_solver(g, precision)
    atol = 1e-12 if precision == pcr.PCR_F64 else 2e-3      # fp32 scores can flip near-tied pairs
    for tag, U, V in (("eval0", g["U0"], g["V0"]), ("eval1", g["U1"], g["V1"])):
        s.set_factors(U, V)
        e, n = s.evaluate(0)
        assert abs(e - g[tag + "_train"][0]) < atol
        if not (name == "edge5" and tag == "eval0"):        # exact score ties: NDCG tie order unspecified
            assert abs(n - g[tag + "_train"][1]) < atol
            et, nt = s.evaluate(1)
            assert abs(et - g[tag + "_test"][0]) < atol and abs(nt - g[tag + "_test"][1]) < atol


@pytest.mark.parametrize("solver", [2, 1])
@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_train_vs_reference_cli_f64(name, solver):
    """pcr_train in fp64 from the reference's init reproduces omp-pmf-train -n 1: objective, pairwise
    error, NDCG per iteration, the final factors and the log lines."""
    g, meta = load_golden(name)
    d1, d2, r = int(g["d1"]), int(g["d2"]), int(g["r"])
    s = make_solver(g, pcr.PCR_F64, solver=solver, maxiter=meta["iters"], threads=1)
    s.set_factors(pcr.initial(d1, r), pcr.initial(d2, r))
    recs, lines = s.train()
    text = meta[f"stdout_s{solver}"]
    objs = [float(x) for x in re.findall(r"^Iter \d+ time \S+ obj (\S+)$", text, re.M)]
    tr = [(float(a), float(b)) for a, b in re.findall(r"^\(Training\) pairwise error is (\S+) and ndcg is (\S+)$", text, re.M)]
    te = [(float(a), float(b)) for a, b in re.findall(r"^\(Testing\) pairwise error is (\S+) and ndcg is (\S+)$", text, re.M)]
    for k, rec in enumerate(recs):
        assert abs(rec["obj"] / objs[k] - 1) < 2e-5
        assert abs(rec["train_err"] - tr[k][0]) < 2e-6 and abs(rec["train_ndcg"] - tr[k][1]) < 2e-6
        assert abs(rec["test_err"] - te[k][0]) < 2e-6 and abs(rec["test_ndcg"] - te[k][1]) < 2e-6
    U, V = s.get_factors()
    assert rel(U, g[f"cli_U_s{solver}"]) < 1e-6 and rel(V, g[f"cli_V_s{solver}"]) < 1e-6
    # the log lines the reference prints from inside pcrpp()/pcr() (pcrpp.cpp:849-890), verbatim format
    ref_lines = [l for l in text.split("\n") if l.startswith(("running", "using", "Iter", "(Tr", "(Te"))]
    ours = [re.sub(r"time \S+", "time T", l) for l in lines]
    theirs = [re.sub(r"time \S+", "time T", l) for l in ref_lines]
    assert len(ours) == len(theirs)
    for a, b in zip(ours, theirs):
        if a != b:       # 6-significant-digit prints may differ in the last digit
            assert re.sub(NUM, "#", a) == re.sub(NUM, "#", b)
            fa = [float(x) for x in re.findall(NUM, a)]
            fb = [float(x) for x in re.findall(NUM, b)]
            assert np.allclose(fa, fb, rtol=2e-5, atol=2e-6)


@pytest.mark.parametrize("precision", [pcr.PCR_F64, pcr.PCR_F32])
def test_against_oracle_mixed_lengths(oracle, precision):
    """A seeded set whose users span every length class (wave / 256 / 1024-thread workgroups and the
    global-scratch path for > 4096 ratings), HIP vs oracle function by function."""
    rng = np.random.default_rng(5)
    d1, d2, r, lam = 40, 6000, 12, 30.0
    lens = np.concatenate([[0, 1, 2, 5000, 4097, 4096, 1500, 1024, 1025, 300, 256, 257, 64, 65], rng.integers(3, 200, d1 - 14)])
    user = np.repeat(np.arange(d1), lens)
    item = np.concatenate([rng.choice(d2, n, replace=False) for n in lens])
    val = rng.integers(1, 6, user.shape[0]).astype(np.float64)
    X = oracle.build_csr(d1, d2, user, item, val)
    U = oracle.initial(d1, r) * 0.3; V = oracle.initial(d2, r) * 0.3
    ds = pcr.Dataset.from_triplets(d1, d2, user, item, val)
    s = pcr.Solver(ds, pcr.Parameter(k=r, precision=precision, **{"lambda": lam}))
    t = TOL[precision]
    s.set_factors(U, V)
    m = s.comp_m()
    mo = oracle.comp_m(U, V, X)
    assert rel(m, mo) < t["m"]
    assert abs(s.objective() / oracle.objective_new(mo, U, V, X, lam) - 1) < t["obj"]
    assert rel(s.obtain_g(), oracle.obtain_g_new(U, V, X, mo, lam)) < t["vec"]
    a = rng.normal(size=V.shape)
    assert rel(s.compute_Ha(a), oracle.compute_Ha_new(a, mo, U, X, lam)) < t["vec"]
    Uo, objo, info_o = oracle.update_U_new(X, mo, lam, 1.0, V, U)
    objU, info = s.update_U()
    Ug, _ = s.get_factors()
    assert rel(Ug, Uo) < t["fac"]
    assert abs(objU / objo - 1) < max(t["obj"], t["fac"] * 1e-2)
    if precision == pcr.PCR_F64:
        assert info["cg"] == info_o["cg"] and info["ls"] == info_o["ls"]
    e, n = s.evaluate(0)
    eo, no = oracle.eval(Ug, V, X)
    assert abs(e - eo) < (1e-12 if precision == pcr.PCR_F64 else 2e-3)
    assert abs(n - no) < (1e-12 if precision == pcr.PCR_F64 else 2e-3)


def test_real_valued_levels_and_zero_model(oracle):
    """Known answers: objective at U = V = 0 equals #Omega; real-valued ratings are
    bucketed by lround (quirk q2)."""
    R = synth.generate("small", seed=3, real_valued=True)
    ds = pcr.Dataset.from_ratings(R)
    X = oracle.build_csr(R.d1, R.d2, R.user, R.item, R.val)
    s = pcr.Solver(ds, pcr.Parameter(k=8, precision=pcr.PCR_F64))
    s.set_factors(np.zeros((R.d1, 8)), np.zeros((R.d2, 8)))
    s.comp_m(want=False)
    assert s.objective() == float(oracle.count_pairs(X)) == float(ds.count_pairs())


@pytest.mark.parametrize("nranks", [2, 4, 5])
def test_ranks_with_empty_shards(nranks):
    """More ranks than users with ratings (one user holds nearly everything): the nnz-balanced partition hands some ranks an
    EMPTY user range -- zero users, zero ratings, every launch of theirs a grid of nothing.  They must create, run every entry
    point and contribute exact zeros: the partial gradients still add up to the one-rank gradient, and with the two-process CLI
    the job still trains (pcrpp.cpp:825-833 is the loop being sharded)."""
    rng = np.random.default_rng(0)
    d1, d2, r, lam = 5, 300, 8, 3.0
    lens = np.array([250, 0, 3, 0, 0])
    user = np.repeat(np.arange(d1), lens)
    item = np.concatenate([rng.choice(d2, n, replace=False) for n in lens])
    val = rng.integers(1, 6, len(user)).astype(np.float64)
    ds = pcr.Dataset.from_triplets(d1, d2, user, item, val)
    bounds = pcr.partition_users(np.concatenate([[0], np.cumsum(lens)]), nranks)
    assert bounds[0] == 0 and bounds[-1] == d1 and (np.diff(bounds) >= 0).all()
    if nranks > 2:
        assert (np.diff(bounds) == 0).any()
    par = dict(k=r, precision=pcr.PCR_F64, **{"lambda": lam})
    U0, V0 = pcr.initial(d1, r), pcr.initial(d2, r)
    one = pcr.Solver(ds, pcr.Parameter(**par))
    one.set_factors(U0, V0); one.comp_m(want=False)
    g1 = one.obtain_g(); one.update_U(); U1, _ = one.get_factors()
    g_sum, U_sh = 0.0, U0.copy()
    for q in range(nranks):
        s = pcr.Solver(ds, pcr.Parameter(**par), rank=q, nranks=nranks)
        assert (s.first_user, s.n_users) == (bounds[q], bounds[q + 1] - bounds[q])
        s.set_local_only(True)
        s.set_factors(U0, V0)
        m = s.comp_m()
        assert len(m) == s.nnz_local
        g_sum = g_sum + s.obtain_g()
        s.update_U()
        Uq, _ = s.get_factors()
        U_sh[s.first_user:s.first_user + s.n_users] = Uq[s.first_user:s.first_user + s.n_users]
        s.close()
    assert rel(g_sum, g1) < 1e-12 and rel(U_sh, U1) < 1e-12


@pytest.mark.parametrize("nranks", [2, 3])
def test_user_sharding_on_one_gpu(oracle, nranks):
    """The N-rank user sharding verified in ONE process on one GPU (shard-local mode, host-side sums
    stand in for the RCCL all-reduce): shard partials of m, objective, g, Ha add up to the single-rank
    result, and every shard's U step reproduces its rows of the single-rank U step."""
    R = synth.generate("small", seed=9)
    r, lam = 12, 40.0
    ds = pcr.Dataset.from_ratings(R)
    U0, V0 = pcr.initial(R.d1, r) * 0.5, pcr.initial(R.d2, r) * 0.5
    par = dict(k=r, precision=pcr.PCR_F64, **{"lambda": lam})
    full = pcr.Solver(ds, pcr.Parameter(**par))
    full.set_factors(U0, V0)
    m_full = full.comp_m(); obj_full = full.objective(); g_full = full.obtain_g()
    a = np.random.default_rng(1).normal(size=V0.shape)
    Ha_full = full.compute_Ha(a)
    full.update_U()
    U_full, _ = full.get_factors()
    shards = [pcr.Solver(ds, pcr.Parameter(**par), rank=q, nranks=nranks) for q in range(nranks)]
    idx, _, _ = ds.csr(0)
    bounds = pcr.partition_users(idx, nranks)
    m_parts, g_sum, Ha_sum, obj_sum = [], 0.0, 0.0, 0.0
    U_sh = np.zeros_like(U0)
    for q, s in enumerate(shards):
        assert (s.first_user, s.n_users) == (bounds[q], bounds[q + 1] - bounds[q])
        s.set_local_only(True)
        s.set_factors(U0, V0)
        m_parts.append(s.comp_m())
        obj_sum += s.objective()
        g_sum = g_sum + s.obtain_g()
        Ha_sum = Ha_sum + s.compute_Ha(a)
        s.update_U()
        Uq, _ = s.get_factors()
        U_sh[s.first_user:s.first_user + s.n_users] = Uq[s.first_user:s.first_user + s.n_users]
    assert np.array_equal(np.concatenate(m_parts), m_full)
    # every shard adds lambda/2 |V|^2 to its local objective; count it once
    obj_sum -= (nranks - 1) * lam / 2.0 * float((V0 ** 2).sum())
    assert abs(obj_sum / obj_full - 1) < 1e-12
    assert rel(g_sum, g_full) < 1e-12 and rel(Ha_sum, Ha_full) < 1e-12
    assert rel(U_sh, U_full) < 1e-12
    # pcr_solver_create_shard: a rank that holds ONLY its own users (renumbered from 0) is the same solver, bit for bit
    idx, item, val = ds.csr(0)
    tidx, titem, tval = ds.csr(1)
    for q, s in enumerate(shards):
        u0, u1 = int(bounds[q]), int(bounds[q + 1])
        loc = pcr.Dataset.from_csr(u1 - u0, R.d2, idx[u0:u1 + 1] - idx[u0], item[idx[u0]:idx[u1]], val[idx[u0]:idx[u1]],
                                   tidx[u0:u1 + 1] - tidx[u0], titem[tidx[u0]:tidx[u1]], tval[tidx[u0]:tidx[u1]])
        t = pcr.Solver(loc, pcr.Parameter(**par), rank=q, nranks=nranks, shard=(u0, R.d1))
        assert (t.first_user, t.n_users, t.nnz_local, t.d1) == (u0, u1 - u0, s.nnz_local, R.d1)
        t.set_local_only(True)
        t.set_factors_local(U0[u0:u1], V0)
        assert np.array_equal(t.comp_m(), m_parts[q])
        s.set_factors(U0, V0); s.comp_m()
        assert t.objective() == s.objective()
        assert np.array_equal(t.obtain_g(), s.obtain_g())
        t.update_U(); s.update_U()
        assert np.array_equal(t.get_factors_local()[0], s.get_factors()[0][u0:u1])
        assert t.evaluate(1, 10) == s.evaluate(1, 10)
        t.close()
    with pytest.raises(pcr.PcrError):
        pcr.Solver(ds, pcr.Parameter(**par), rank=0, nranks=2, shard=(10, R.d1))      # the shard does not fit the job's user range


def test_fp32_training_matches_reference_quality(oracle):
    """North star: NDCG@10 / pairwise error of the fp32 path match the reference (its fp64 restatement,
    same init, same iteration count) within fp32 tolerance -- 1e-3 -- and the objective
    trajectory within 1e-3 relative."""
    R = synth.generate("small", seed=17, d1=1500, d2=800, nnz=120000, mu=4.0, sigma=0.9)
    r, lam, iters = 32, 200.0, 3
    X = oracle.build_csr(R.d1, R.d2, R.user, R.item, R.val)
    XT = oracle.build_csr_test(R.d1, R.d2, R.tuser, R.titem, R.tval)
    U0, V0 = pcr.initial(R.d1, r), pcr.initial(R.d2, r)
    _, _, ref = oracle.train(X, U0, V0, lam, iters, XT)
    s = pcr.Solver(pcr.Dataset.from_ratings(R), pcr.Parameter(k=r, maxiter=iters, precision=pcr.PCR_F32, **{"lambda": lam}))
    s.set_factors(U0, V0)
    recs, _ = s.train()
    for a, b in zip(recs, ref):
        assert abs(a["obj"] / b["obj"] - 1) < 1e-3
        for key in ("train_err", "train_ndcg", "test_err", "test_ndcg"):
            assert abs(a[key] - b[key]) < 1e-3, (key, a[key], b[key])
    assert [a["cg_v"] for a in recs] == [b["cg_v"] for b in ref]


def _mixed_set(seed=11, d1=700, d2=6000):
    rng = np.random.default_rng(seed)
    lens = np.concatenate([[0, 1, 2, 5000, 4500, 4097, 4096, 3000, 2049, 2048, 1500, 1025, 1024, 700, 513, 512, 300, 257, 256, 129, 128, 65, 64, 33, 32],
                           np.clip(rng.lognormal(4.0, 1.0, d1 - 25).astype(np.int64), 3, 900)])
    user = np.repeat(np.arange(d1), lens)
    item = np.concatenate([rng.choice(d2, n, replace=False) for n in lens])
    val = rng.integers(1, 6, user.shape[0]).astype(np.float64)
    return d1, d2, user, item, val


VARIANTS = [
    {},                                                          # default launch configuration
    {"ustep_mode": "2"},                                     # throughput variants: 256 threads / 512 threads at 4 rows in flight
    {"ustep_mode": "1"},                                     # latency variants everywhere
    {"cluster_k": "1"},                                      # no workgroup clusters
    {"ubins": "64:64:0,512:256:0"},                          # no LDS-resident rows, coarser classes
    {"ubins": "16:64:1,48:64:1,200:256:0,700:256:0"},        # other class bounds
    {"spmm_tiles": "5"}, {"spmm_tiles": "16"}, {"spmm_tiles": "64"},   # user tiles of the SpMM (incl. more tiles than XCDs)
    {"spmm_chunk": "32"}, {"spmm_chunk": "128"},         # ratings per SpMM lane group (the default adapts to the shard: 64 here)
    {"lanes": "1"},                                          # every class on the solver's stream
    {"ustep_gram": "128"}, {"ustep_gram": "40"}, {"ustep_gram": "64", "window_cache": "0"},   # dual (Gram matrix on MFMA) form for short users
    {"window_cache": "0"}, {"prepare_merged": "0"}, {"pipeline": "0"},   # searching sweeps, per-class prepare, host round trip per U step
    {"sddmm_csc": "1"}, {"sddmm_csc": "1", "spmm_tiles": "16"},   # the CG's SDDMM over the tile-major CSC (wide item tables)
    {"allreduce_chunks": "3"}, {"allreduce_chunks": "5", "spmm_tiles": "16"}, {"allreduce_chunks": "4", "sddmm_csc": "1"},   # SpMM item range by item range (the N > 1 overlap form)
    {"allreduce_chunks": "3", "spmm_tiles": "8"},            # ... with exactly one tile per XCD (the tile <-> XCD affinity inside every range's plan)
    {"cluster_users": "64"},                                 # as many clusters as the chip holds (members on every XCD)
    {"resort_window": "0"}, {"resort_window": "2"}, {"resort_window": "64"},   # the sorts' nearly-sorted fast path: off, narrow, widest
    {"spmm_tiles": "2"}, {"spmm_tiles": "4"},                # tiles bound to groups of 4 / 2 XCDs
    {"plan_key64": "1"}, {"plan_key64": "1", "allreduce_chunks": "3", "spmm_tiles": "16"},   # the device-built plan with 64-bit (tile, item) keys
    {"vblock_users": "8"}, {"vblock_users": "40", "spmm_tiles": "4"}, {"vblock_users": "33", "allreduce_chunks": "3"},   # the blocked-user V step: dense MFMA kernels for the longest users
]


def test_launch_variants_agree(oracle):
    """The length classes, workgroup variants, cluster size, SpMM tiling and stream placement are scheduling choices:
    two outer iterations in fp64 must give the same factors and objectives under every one of them (to summation-order
    rounding), and the first U step must match the oracle."""
    d1, d2, user, item, val = _mixed_set()
    r, lam = 12, 30.0
    X = oracle.build_csr(d1, d2, user, item, val)
    U0 = oracle.initial(d1, r) * 0.3; V0 = oracle.initial(d2, r) * 0.3
    ds = pcr.Dataset.from_triplets(d1, d2, user, item, val)
    results = []
    for env in VARIANTS:
        with pcr.tuned(**env):                                   # pcr_tune(): read when the solver is created
            s = pcr.Solver(ds, pcr.Parameter(k=r, precision=pcr.PCR_F64, **{"lambda": lam}))
        s.set_factors(U0, V0)
        objs = []
        for _ in range(2):
            oV, iv = s.update_V(); oU, iu = s.update_U()
            objs += [oV, oU, iv["cg"], iv["ls"], iu["cg"], iu["ls"]]
        U, V = s.get_factors()
        results.append((env, np.array(objs), U, V))
    _, o0, U_ref, V_ref = results[0]
    for env, o, U, V in results[1:]:
        assert np.allclose(o, o0, rtol=1e-10, atol=0), (env, o, o0)
        assert rel(U, U_ref) < 1e-8 and rel(V, V_ref) < 1e-8, env
    # oracle: V step then U step from the same start
    m0 = oracle.comp_m(U0, V0, X)
    V1, m1, objV, info_v = oracle.update_V_new(X, lam, 1.0, U0, V0)
    U1, objU, info_u = oracle.update_U_new(X, m1, lam, 1.0, V1, U0)
    s = pcr.Solver(ds, pcr.Parameter(k=r, precision=pcr.PCR_F64, **{"lambda": lam}))
    s.set_factors(U0, V0)
    oV, _ = s.update_V(); oU, iu = s.update_U()
    Ug, Vg = s.get_factors()
    assert abs(oV / objV - 1) < 1e-9 and abs(oU / objU - 1) < 1e-9
    assert rel(Vg, V1) < 1e-7 and rel(Ug, U1) < 1e-7
    assert iu["cg"] == info_u["cg"] and iu["ls"] == info_u["ls"]


@pytest.mark.parametrize("precision", [pcr.PCR_F64, pcr.PCR_F32])
def test_nearly_sorted_fast_path_walks_the_same_trajectory(oracle, precision):
    """From the third outer iteration on most users are re-sorted by windowed rank counting instead of the bitonic network
    (resort_window; verified per user, falls back otherwise).  Any (level, m)-sorted order gives the same sums, so eight outer
    iterations with the fast path (default, and a narrow window that falls back often) must equal the run that always sorts
    fully -- to summation-order rounding in fp64 with identical inner counts, and the fp64 run must match the oracle."""
    d1, d2, user, item, val = _mixed_set(seed=21, d1=500, d2=5200)
    r, lam, iters = 12, 30.0, 8
    ds = pcr.Dataset.from_triplets(d1, d2, user, item, val)
    U0 = oracle.initial(d1, r) * 0.3; V0 = oracle.initial(d2, r) * 0.3
    runs = {}
    for w in (0, 8, 3):
        with pcr.tuned(resort_window=w):
            s = pcr.Solver(ds, pcr.Parameter(k=r, precision=precision, do_predict=0, **{"lambda": lam}))
        s.set_factors(U0, V0)
        recs = s.iterate(iters)
        runs[w] = (recs, s.get_factors())
        s.close()
    tol = 1e-9 if precision == pcr.PCR_F64 else 2e-3
    for w in (8, 3):
        for a, b in zip(runs[0][0], runs[w][0]):
            assert abs(a["obj"] / b["obj"] - 1) < tol, (w, a, b)
            if precision == pcr.PCR_F64:
                assert (a["cg_v"], a["ls_v"], a["cg_u"], a["ls_u"]) == (b["cg_v"], b["ls_v"], b["cg_u"], b["ls_u"]), w
        assert rel(runs[w][1][0], runs[0][1][0]) < tol * 10 and rel(runs[w][1][1], runs[0][1][1]) < tol * 10
    if precision == pcr.PCR_F64:
        X = oracle.build_csr(d1, d2, user, item, val)
        _, _, ref = oracle.train(X, U0, V0, lam, iters, do_predict=0)
        for a, b in zip(runs[8][0], ref[1:]):
            assert abs(a["obj"] / b["obj"] - 1) < 1e-8


def test_state_left_by_u_step_equals_a_fresh_prepare(oracle):
    """k_ustep leaves the sorted state of (U_new, V) behind and update_V starts from it (no SDDMM + sort of its own).
    A second solver that is handed the same factors through set_factors must rebuild that state and take the same V step."""
    d1, d2, user, item, val = _mixed_set(seed=12, d1=300)
    r, lam = 10, 20.0
    ds = pcr.Dataset.from_triplets(d1, d2, user, item, val)
    U0 = oracle.initial(d1, r) * 0.3; V0 = oracle.initial(d2, r) * 0.3
    for precision, tol in ((pcr.PCR_F64, 1e-9), (pcr.PCR_F32, 5e-4)):
        a = pcr.Solver(ds, pcr.Parameter(k=r, precision=precision, **{"lambda": lam}))
        a.set_factors(U0, V0)
        a.update_V(); a.update_U()
        U1, V1 = a.get_factors()
        obj_state = a.objective()                    # from the state k_ustep left
        gA = a.obtain_g()
        oA, iA = a.update_V()
        b = pcr.Solver(ds, pcr.Parameter(k=r, precision=precision, **{"lambda": lam}))
        b.set_factors(U1, V1)
        b.comp_m()                                   # fresh SDDMM + sort
        assert abs(obj_state / b.objective() - 1) < tol * 1e-2
        assert rel(gA, b.obtain_g()) < tol
        oB, iB = b.update_V()
        assert abs(oA / oB - 1) < tol * 1e-1
        assert rel(a.get_factors()[1], b.get_factors()[1]) < tol * 10
        if precision == pcr.PCR_F64:
            assert iA == iB


def test_pipelined_iterations_equal_the_step_by_step_loop(oracle):
    """pcr_iterate (U step queued without a host round trip, its objective read at the next line search) must walk the
    same trajectory as update_V / update_U called one by one, bit for bit, and report the same counts."""
    d1, d2, user, item, val = _mixed_set(seed=13, d1=400)
    r, lam = 10, 20.0
    ds = pcr.Dataset.from_triplets(d1, d2, user, item, val)
    U0 = oracle.initial(d1, r) * 0.3; V0 = oracle.initial(d2, r) * 0.3
    for precision in (pcr.PCR_F64, pcr.PCR_F32):
        a = pcr.Solver(ds, pcr.Parameter(k=r, precision=precision, **{"lambda": lam}))
        a.set_factors(U0, V0)
        step = []
        for _ in range(4):
            _, iv = a.update_V(); o, iu = a.update_U()
            step.append((o, iv["cg"], iv["ls"], iu["cg"], iu["ls"]))
        b = pcr.Solver(ds, pcr.Parameter(k=r, precision=precision, **{"lambda": lam}))
        b.set_factors(U0, V0)
        recs = b.iterate(3) + b.iterate(1)           # also across two calls
        assert [(x["obj"], x["cg_v"], x["ls_v"], x["cg_u"], x["ls_u"]) for x in recs] == step
        assert all(x["seconds"] > 0 for x in recs) and recs[2]["seconds"] > recs[0]["seconds"]
        Ua, Va = a.get_factors(); Ub, Vb = b.get_factors()
        assert np.array_equal(Ua, Ub) and np.array_equal(Va, Vb)


@pytest.mark.parametrize("knobs", [{}, {"ustep_gram": 128}], ids=["default", "gram"])
def test_line_search_failure_quirks(oracle, knobs):
    """(Every form of the U step: the dual form must take its gradient coefficients from the STALE scores of the rejected V_new
    but every b = V_I s and every line-search score from the V that was kept -- a fuzz case caught it using the stale ones.)
    q5: a V step whose 20 line-search tries all fail keeps V but hands the m of the LAST TRIED V_new to the U step
    (pcrpp.cpp:430-431, :443); a U step whose tries all fail returns the last tried u (:794-814).  Forced with an absurd
    initial step size; the next V step must rebuild its state (the U step's skipped users still carry the rejected one)."""
    d1, d2, user, item, val = _mixed_set(seed=14, d1=120)
    r, lam, step = 8, 20.0, float(2 ** 40)
    X = oracle.build_csr(d1, d2, user, item, val)
    U0 = oracle.initial(d1, r) * 0.3; V0 = oracle.initial(d2, r) * 0.3
    ds = pcr.Dataset.from_triplets(d1, d2, user, item, val)
    with pcr.tuned(**knobs):
        s = pcr.Solver(ds, pcr.Parameter(k=r, precision=pcr.PCR_F64, stepsize=step, **{"lambda": lam}))
    s.set_factors(U0, V0)
    U, V = U0, V0
    for it in range(2):
        Vn, m, objV, iv = oracle.update_V_new(X, lam, step, U, V)
        gV, giv = s.update_V()
        assert (giv["ls"], giv["accepted"], giv["cg"]) == (iv["ls"], iv["accepted"], iv["cg"]) and iv["accepted"] == 0 and iv["ls"] == 20
        assert abs(gV / objV - 1) < 1e-9
        assert rel(s.get_factors()[1], Vn) < 1e-12 and np.array_equal(Vn, V)          # V unchanged
        Un, objU, iu = oracle.update_U_new(X, m, lam, step, Vn, U)
        gU, giu = s.update_U()
        assert (giu["cg"], giu["ls"]) == (iu["cg"], iu["ls"])
        assert abs(gU / objU - 1) < 1e-9 and rel(s.get_factors()[0], Un) < 1e-9
        U, V = Un, Vn


@pytest.mark.parametrize("knobs", [{}, {"ustep_gram": 128}, {"win16": 0, "ustep_win_lds": 0}],
                         ids=["default", "gram", "win32"])
def test_fuzz_small_shapes_against_oracle(oracle, knobs):
    """Seeded random shapes around the corners of the launch logic: ranks that are not multiples of 4, 1..12 rating
    levels (window cache on and off), real-valued ratings, users of 0..700 ratings, both solvers; two outer iterations in
    fp64 must follow the oracle's trajectory (objectives, inner counts, factors) -- in the default launch configuration and
    with the alternative U-step forms (dual form on MFMA, lock-step passes) switched on."""
    rng = np.random.default_rng(2026)
    for case in range(80):
        d1 = int(rng.integers(3, 60)); d2 = int(rng.integers(20, 900))
        r = int(rng.choice([1, 2, 3, 5, 7, 8, 12, 17, 33, 64]))
        nlev = int(rng.choice([1, 2, 3, 5, 9, 10, 12]))
        solver = int(rng.choice([1, 2]))
        real = bool(rng.integers(0, 2)) and nlev > 1
        lam = float(rng.choice([0.5, 5.0, 50.0, 500.0]))
        lens = np.minimum(rng.choice([0, 1, 2, 3, 10, 40, 64, 65, 130, 256, 257, 300, 700], d1), d2)
        lens[rng.integers(0, d1)] = min(d2, 64)
        user = np.repeat(np.arange(d1), lens)
        item = np.concatenate([rng.choice(d2, n, replace=False) for n in lens]) if user.size else np.zeros(0, np.int64)
        val = rng.integers(1, nlev + 1, user.shape[0]).astype(np.float64)
        if real:
            val = val + rng.uniform(-0.49, 0.49, val.shape[0])           # same lround bucket (solver 2), distinct doubles (solver 1)
        if user.size == 0:
            continue
        X = oracle.build_csr(d1, d2, user, item, val)
        U0 = oracle.initial(d1, r) * 0.4; V0 = oracle.initial(d2, r) * 0.4
        Uo, Vo, recs = oracle.train(X, U0, V0, lam, 2, solver=solver, do_predict=0)
        with pcr.tuned(**knobs):
            s = pcr.Solver(pcr.Dataset.from_triplets(d1, d2, user, item, val),
                           pcr.Parameter(k=r, solver_type=solver, precision=pcr.PCR_F64, **{"lambda": lam}))
        s.set_factors(U0, V0)
        got = s.iterate(2)
        tag = dict(case=case, knobs=knobs, d1=d1, d2=d2, r=r, nlev=nlev, solver=solver, real=real, lam=lam, nnz=int(user.size))
        for g, o in zip(got, recs[1:]):
            # (1e-8: case 17 -- solver 1, r = 64, the objective falls 1e7 -> 1e5 -> 1e4 -- amplifies summation-order rounding to
            # 1.0e-9 / 1.3e-9 depending on the SpMM chunk length, with identical inner counts; see tools/dbg_fuzz.py)
            assert abs(g["obj"] - o["obj"]) <= 1e-8 * max(abs(o["obj"]), 1.0), (tag, g["obj"], o["obj"])
            assert (g["cg_v"], g["ls_v"], g["cg_u"], g["ls_u"]) == (o["cg_v"], o["ls_v"], o["cg_u"], o["ls_u"]), tag
        Ug, Vg = s.get_factors()
        scale = max(np.abs(Uo).max(), np.abs(Vo).max(), 1e-3)            # (a side without any comparable pair is driven to ~1e-17)
        assert np.abs(Ug - Uo).max() < 1e-7 * scale and np.abs(Vg - Vo).max() < 1e-7 * scale, tag


def test_fuzz_evaluator_against_oracle(oracle):
    """compute_pairwise_error_ndcg (util.cpp:434-542) on seeded random shapes: 1..100 distinct rating values per user (the
    O(len T log len) evaluator and the O(len^2) one for > 64 values), users of 0..700 ratings, non-positive real ratings
    (NDCG may exceed 1 or be NaN in the reference, q8), ndcg_k 1..20.  Scores are generic (no exact ties: the reference
    leaves the tie order of its unstable sort unspecified)."""
    rng = np.random.default_rng(77)
    for case in range(40):
        d1 = int(rng.integers(2, 50)); d2 = int(rng.integers(30, 900)); r = int(rng.choice([1, 3, 8, 16, 33]))
        nval = int(rng.choice([1, 2, 5, 9, 30, 65, 100]))
        lens = np.minimum(rng.choice([0, 1, 2, 5, 20, 64, 65, 129, 256, 300, 700], d1), d2)
        lens[rng.integers(0, d1)] = min(d2, 40)
        user = np.repeat(np.arange(d1), lens)
        item = np.concatenate([rng.choice(d2, n, replace=False) for n in lens])
        pool = np.sort(rng.uniform(-2.0, 5.0, nval)) if rng.integers(0, 2) else np.arange(1, nval + 1, dtype=np.float64)
        val = pool[rng.integers(0, nval, user.shape[0])]
        k = int(rng.choice([1, 5, 10, 20]))
        X = oracle.build_csr(d1, d2, user, item, val)
        U = rng.normal(size=(d1, r)); V = rng.normal(size=(d2, r))
        s = pcr.Solver(pcr.Dataset.from_triplets(d1, d2, user, item, val), pcr.Parameter(k=r, precision=pcr.PCR_F64, ndcg_k=k))
        s.set_factors(U, V)
        e, n = s.evaluate(0, k)
        eo, no = oracle.eval(U, V, X, k)
        tag = dict(case=case, d1=d1, d2=d2, r=r, nval=nval, k=k)
        assert abs(e - eo) < 1e-12, (tag, e, eo)
        assert (np.isnan(n) and np.isnan(no)) or abs(n - no) < 1e-9 * max(1.0, abs(no)), (tag, n, no)


@pytest.mark.parametrize("solver,r,real", [(2, 12, False), (2, 100, False), (1, 7, True), (2, 33, True)])
def test_exact_newton_u_step_from_the_explicit_hessian(oracle, solver, r, real):
    """SURVEY 8f-3, the literal object: pcr_tune("ustep_newton") builds every covered user's r x r Hessian
    H = lambda I + 2 sum over active pairs (x_j - x_q)(x_j - x_q)^T on the matrix cores (k_unewton, fp64 MFMA), factors it by
    Cholesky and hands k_ustep the exact Newton direction; users beyond 1024 ratings run their CG to convergence.  Checked
    against the ORACLE's U step with its CG run to convergence (the same Newton step by the reference's own route): factors,
    objective, line-search counts -- on users of 0 .. 5000 ratings, both solvers, integer and real-valued ratings, a rank with
    pad columns and the bench's rank 100."""
    d1, d2, user, item, val = _mixed_set(seed=5, d1=260, d2=5600)
    if real:
        val = val + np.random.default_rng(1).uniform(-0.4, 0.4, val.shape[0])
    lam = 40.0
    X = oracle.build_csr(d1, d2, user, item, val)
    U0 = oracle.initial(d1, r) * 0.3; V0 = oracle.initial(d2, r) * 0.3
    ds = pcr.Dataset.from_triplets(d1, d2, user, item, val)
    try:
        oracle.set_cg(6 * r + 50, 1e-13)
        m0 = oracle.comp_m(U0, V0, X)
        U1, objU, info_o = (oracle.update_U_new(X, m0, lam, 1.0, V0, U0) if solver == 2 else
                            _oracle_update_U_solver1(oracle, X, m0, lam, V0, U0))
    finally:
        oracle.set_cg()
    with pcr.tuned(ustep_newton=1):
        s = pcr.Solver(ds, pcr.Parameter(k=r, solver_type=solver, precision=pcr.PCR_F64, **{"lambda": lam}))
    s.set_factors(U0, V0)
    s.comp_m()
    oU, iu = s.update_U()
    Ug, _ = s.get_factors()
    if solver == 2:
        assert abs(oU / objU - 1) < 1e-9, (oU, objU)
    assert rel(Ug, U1) < 2e-7
    assert iu["ls"] == info_o["ls"]
    # the covered users took no CG iteration at all: what is counted comes from the users beyond 1024 ratings only
    lens = np.diff(X.idx)
    assert iu["cg"] <= int((lens > 1024).sum()) * (2 * r + 10)
    # and the default mode is untouched by the knob's existence: the truncated CG of the reference
    s2 = pcr.Solver(ds, pcr.Parameter(k=r, solver_type=solver, precision=pcr.PCR_F64, **{"lambda": lam}))
    s2.set_factors(U0, V0); s2.comp_m()
    _, iu2 = s2.update_U()
    assert iu2["cg"] > iu["cg"]
    # fp32 storage: the Hessian is still accumulated in fp64 from the fp32 rows
    if solver == 2 and not real:
        with pcr.tuned(ustep_newton=1):
            s3 = pcr.Solver(ds, pcr.Parameter(k=r, solver_type=solver, precision=pcr.PCR_F32, **{"lambda": lam}))
        s3.set_factors(U0, V0); s3.comp_m()
        o3, iu3 = s3.update_U()
        assert abs(o3 / objU - 1) < 2e-4 and rel(s3.get_factors()[0], U1) < 5e-3


def _oracle_update_U_solver1(oracle, X, m, lam, V, U):
    """update_U of PrimalCR (pcr.cpp:587) through the oracle's per-user entry point."""
    Un = U.copy(); obj = 0.0; ls = 0; cg = 0
    for i in range(X.d1):
        un, o, inf = oracle.update_u_new(i, V, X, m, lam, 1.0, U[i], solver=1)
        Un[i] = un; obj += o; ls += inf["ls"]; cg += inf["cg"]
    return Un, obj + lam / 2.0 * (V ** 2).sum(), {"ls": ls, "cg": cg}


@pytest.mark.parametrize("precision,tol", [(pcr.PCR_F64, 1e-10), (pcr.PCR_F32, 3e-5)])
def test_blocked_user_v_step_against_the_oracle(oracle, precision, tol):
    """SURVEY 8f-3, the second object: pcr_tune("vblock_users") takes the users with the most ratings out of the sparse plan and
    computes their share of b = U A^T and of Hp += C^T U as dense GEMMs on the matrix cores (k_vblock_b / k_vblock_hp, fp32 and
    fp64 MFMA) through a static dense (user, item) -> CSR position index.  Gradient, one Hessian-vector product, the CG's direction
    and count and a whole V step + U step against the oracle -- a shard where the block holds most of the ratings (users of 5000,
    4500, ... of 6000 items) and one where no user qualifies (the knob then changes nothing)."""
    d1, d2, user, item, val = _mixed_set(seed=3, d1=300, d2=6000)
    r, lam = 20, 25.0
    X = oracle.build_csr(d1, d2, user, item, val)
    U0 = oracle.initial(d1, r) * 0.3; V0 = oracle.initial(d2, r) * 0.3
    ds = pcr.Dataset.from_triplets(d1, d2, user, item, val)
    m0 = oracle.comp_m(U0, V0, X)
    g_o = oracle.obtain_g_new(U0, V0, X, m0, lam)
    a = oracle.initial(d2, r)[::-1].copy() * 0.1
    Ha_o = oracle.compute_Ha_new(a, m0, U0, X, lam)
    d_o, its_o = oracle.solve_delta_new(g_o, m0, U0, X, lam)
    V1, m1, objV, iv = oracle.update_V_new(X, lam, 1.0, U0, V0)
    U1, objU, iu = oracle.update_U_new(X, m1, lam, 1.0, V1, U0)
    for nb in (24, 64):
        with pcr.tuned(vblock_users=nb):
            s = pcr.Solver(ds, pcr.Parameter(k=r, precision=precision, **{"lambda": lam}))
        s.set_factors(U0, V0)
        s.comp_m()
        assert rel(s.obtain_g(), g_o) < tol
        assert rel(s.compute_Ha(a), Ha_o) < tol
        dg, its = s.solve_delta(g_o)
        assert rel(dg, d_o) < 50 * tol and (precision == pcr.PCR_F32 or its == its_o)
        s.set_factors(U0, V0)
        oV, info = s.update_V()
        oU, info_u = s.update_U()
        Ug, Vg = s.get_factors()
        assert abs(oV / objV - 1) < 20 * tol and abs(oU / objU - 1) < 20 * tol
        assert rel(Vg, V1) < 200 * tol and rel(Ug, U1) < 200 * tol
        if precision == pcr.PCR_F64:
            assert (info["cg"], info["ls"]) == (iv["cg"], iv["ls"]) and (info_u["cg"], info_u["ls"]) == (iu["cg"], iu["ls"])
    # nobody rates a sixteenth of the catalogue: no block, the plain path
    R = synth.generate("small", seed=2, d1=200, d2=4000, nnz=12000, mu=3.5, sigma=0.6)
    ds2 = pcr.Dataset.from_triplets(R.d1, R.d2, R.user, R.item, R.val)
    X2 = oracle.build_csr(R.d1, R.d2, R.user, R.item, R.val)
    Ua, Va = oracle.initial(R.d1, r) * 0.3, oracle.initial(R.d2, r) * 0.3
    with pcr.tuned(vblock_users=64):
        s = pcr.Solver(ds2, pcr.Parameter(k=r, precision=precision, **{"lambda": lam}))
    s.set_factors(Ua, Va); s.comp_m()
    assert rel(s.obtain_g(), oracle.obtain_g_new(Ua, Va, X2, oracle.comp_m(Ua, Va, X2), lam)) < tol


def test_blocked_user_v_step_with_a_pair_rated_twice(oracle):
    """A rating file may hold a (user, item) pair twice; the loader keeps both entries, as the reference's convert() does
    (util.cpp:219-247).  The dense (user, item) -> position index of the blocked-user V step has one slot per pair, so a block
    candidate with such a pair must stay in the sparse plan: gradient, Hessian-vector product and CG direction still equal the
    oracle's, which treats the two entries as two ratings."""
    d1, d2, user, item, val = _mixed_set(seed=3, d1=300, d2=6000)
    longest = int(np.bincount(user, minlength=d1).argmax())
    z = np.flatnonzero(user == longest)[[5, 900]]
    user = np.concatenate([user, user[z]]); item = np.concatenate([item, item[z]])
    val = np.concatenate([val, np.where(val[z] >= 3, val[z] - 2, val[z] + 2)])          # the second entry carries another level
    r, lam = 20, 25.0
    X = oracle.build_csr(d1, d2, user, item, val)
    assert X.nnz == len(user)                                                              # (both entries kept)
    U0 = oracle.initial(d1, r) * 0.3; V0 = oracle.initial(d2, r) * 0.3
    ds = pcr.Dataset.from_triplets(d1, d2, user, item, val)
    m0 = oracle.comp_m(U0, V0, X)
    g_o = oracle.obtain_g_new(U0, V0, X, m0, lam)
    a = oracle.initial(d2, r)[::-1].copy() * 0.1
    Ha_o = oracle.compute_Ha_new(a, m0, U0, X, lam)
    d_o, its_o = oracle.solve_delta_new(g_o, m0, U0, X, lam)
    with pcr.tuned(vblock_users=24):
        s = pcr.Solver(ds, pcr.Parameter(k=r, precision=pcr.PCR_F64, **{"lambda": lam}))
    s.set_factors(U0, V0)
    s.comp_m()
    assert rel(s.obtain_g(), g_o) < 1e-10
    assert rel(s.compute_Ha(a), Ha_o) < 1e-10
    dg, its = s.solve_delta(g_o)
    assert rel(dg, d_o) < 5e-9 and its == its_o


def test_cg_knobs_and_exact_newton_u_step(oracle):
    """cg_max_iter / cg_tol (the reference hard-codes 10 / 0.01).  With the same settings the device and the
    oracle still agree step by step (iteration counts included); with cg_max_iter = r and a tiny tolerance the U step
    is an exact Newton step: its direction solves H delta = g, checked through a second, independent run of the
    Hessian-vector product on the V side (the residual of the returned delta is ~ 0)."""
    R = synth.generate("small", seed=9, d1=150, d2=90, nnz=5000, mu=3.2, sigma=0.9)
    r, lam = 8, 3.0
    X = oracle.build_csr(R.d1, R.d2, R.user, R.item, R.val)
    U = oracle.initial(R.d1, r) * 0.4; V = oracle.initial(R.d2, r) * 0.4
    ds = pcr.Dataset.from_triplets(R.d1, R.d2, R.user, R.item, R.val)
    try:
        for cg_max, tol in ((2, 1e-9), (60, 1e-5)):       # (1e-5: far enough above the rounding floor for equal counts)
            oracle.set_cg(cg_max, tol)
            s = pcr.Solver(ds, pcr.Parameter(k=r, precision=pcr.PCR_F64, cg_max_iter=cg_max, cg_tol=tol, **{"lambda": lam}))
            s.set_factors(U, V)
            mo = oracle.comp_m(U, V, X)
            s.comp_m()
            g = s.obtain_g()
            delta, its = s.solve_delta(g)
            do, its_o = oracle.solve_delta_new(oracle.obtain_g_new(U, V, X, mo, lam), mo, U, X, lam)
            assert its == its_o and rel(delta, do) < 1e-7
            if cg_max == 2:
                assert its == 2                                   # the cap binds
            else:
                assert 10 < its < 60                              # runs past the reference's 10, stops on the tolerance
                assert rel(s.compute_Ha(delta), g) < 1e-4         # an (almost) exact Newton direction
            s.set_factors(U, V)
            Vo, m1, objVo, iv = oracle.update_V_new(X, lam, 1.0, U, V)
            objV, info = s.update_V()
            assert info["cg"] == iv["cg"] and info["ls"] == iv["ls"] and abs(objV / objVo - 1) < 1e-10
            Uo, objUo, iu = oracle.update_U_new(X, m1, lam, 1.0, Vo, U)
            objU, info = s.update_U()
            Ug, Vg = s.get_factors()
            assert info["cg"] == iu["cg"] and info["ls"] == iu["ls"]
            assert rel(Ug, Uo) < 1e-7 and rel(Vg, Vo) < 1e-7 and abs(objU / objUo - 1) < 1e-10
        # r-dimensional systems: CG needs at most r iterations per user (+ rounding), far fewer than the cap of 60
        assert iu["cg"] <= (r + 2) * R.d1
        with pytest.raises(pcr.PcrError):
            pcr.Solver(ds, pcr.Parameter(k=r, cg_tol=-1.0))
    finally:
        oracle.set_cg()


@pytest.mark.parametrize("precision,r", [(pcr.PCR_F32, 200), (pcr.PCR_F32, 260), (pcr.PCR_F64, 140), (pcr.PCR_F64, 257)])
def test_wide_ranks_against_oracle(oracle, precision, r):
    """Ranks at and beyond one pass of a 64-lane group (64 16-byte chunks = 256 floats / 128 doubles per row): k = 200 is
    configs[4]'s rank (one pass, 64 lanes); 260 (fp32) and 140, 257 (fp64) take two or three passes through the row in every
    gather kernel and the per-user r-vectors of k_ustep are longer than a wave.  One outer iteration against the oracle."""
    R = synth.generate("small", seed=21, d1=90, d2=160, nnz=4000, mu=3.3, sigma=1.0)
    lam = 40.0
    X = oracle.build_csr(R.d1, R.d2, R.user, R.item, R.val)
    U0 = oracle.initial(R.d1, r) * 0.1; V0 = oracle.initial(R.d2, r) * 0.1
    ds = pcr.Dataset.from_ratings(R)
    s = pcr.Solver(ds, pcr.Parameter(k=r, precision=precision, **{"lambda": lam}))
    t = TOL[precision]
    s.set_factors(U0, V0)
    mo = oracle.comp_m(U0, V0, X)
    assert rel(s.comp_m(), mo) < t["m"]
    assert rel(s.obtain_g(), oracle.obtain_g_new(U0, V0, X, mo, lam)) < t["vec"]
    a = np.random.default_rng(2).normal(size=V0.shape)
    assert rel(s.compute_Ha(a), oracle.compute_Ha_new(a, mo, U0, X, lam)) < t["vec"]
    V1, m1, objVo, iv = oracle.update_V_new(X, lam, 1.0, U0, V0)
    U1, objUo, iu = oracle.update_U_new(X, m1, lam, 1.0, V1, U0)
    s.set_factors(U0, V0)
    objV, info_v = s.update_V()
    objU, info_u = s.update_U()
    Ug, Vg = s.get_factors()
    assert abs(objV / objVo - 1) < max(t["obj"], t["cg"] * 1e-2) and abs(objU / objUo - 1) < max(t["obj"], t["fac"] * 1e-2)
    assert rel(Vg, V1) < t["fac"] and rel(Ug, U1) < t["fac"]
    if precision == pcr.PCR_F64:
        assert info_v["cg"] == iv["cg"] and info_v["ls"] == iv["ls"] and info_u["cg"] == iu["cg"] and info_u["ls"] == iu["ls"]
    e, n = s.evaluate(0)
    eo, no = oracle.eval(Ug, Vg, X)
    assert abs(e - eo) < (1e-12 if precision == pcr.PCR_F64 else 2e-3) and abs(n - no) < (1e-12 if precision == pcr.PCR_F64 else 2e-3)


@pytest.mark.parametrize("solver", [2, 1])
def test_empty_rating_set(oracle, solver):
    """No ratings at all: the objective is the regulariser alone, the first V step is one CG iteration that lands on
    V = 0 (to rounding), the second one finds nothing to gain and exhausts its 20 line-search tries (q5), users keep
    their factors (q6), the training metrics are 0/0 (util.cpp:537).  Same records as the oracle."""
    d1, d2, r = 5, 7, 4
    e32, e64 = np.zeros(0, np.int32), np.zeros(0)
    X = oracle.build_csr(d1, d2, e32, e32, e64)
    U0 = oracle.initial(d1, r); V0 = oracle.initial(d2, r)
    Uo, Vo, ro = oracle.train(X, U0, V0, 3.0, 2, solver=solver, do_predict=1)
    ds = pcr.Dataset.from_triplets(d1, d2, e32, e32, e64)
    s = pcr.Solver(ds, pcr.Parameter(k=r, precision=pcr.PCR_F64, solver_type=solver, maxiter=2, do_predict=1, **{"lambda": 3.0}))
    s.set_factors(U0, V0)
    recs, _ = s.train()
    Ug, Vg = s.get_factors()
    assert len(recs) == len(ro) == 3
    for a, b in zip(recs, ro):
        assert abs(a["obj"] - b["obj"]) <= 1e-12 * abs(b["obj"])
        assert (a["cg_v"], a["ls_v"], a["cg_u"], a["ls_u"]) == (b["cg_v"], b["ls_v"], b["cg_u"], b["ls_u"])
        assert np.isnan(a["train_err"]) and np.isnan(a["train_ndcg"])
    assert np.array_equal(Ug, U0) and np.abs(Vg).max() < 1e-14


def test_users_beyond_65535_ratings(oracle):
    """Yahoo-shaped data has users with more than 2^16 ratings: positions inside such a user no longer fit 16
    bits and the user lives in the global-scratch classes.  One user who rated every one of 70 000 items, one with 66 000,
    next to short ones; one outer iteration in fp64 against the oracle, counts included."""
    rng = np.random.default_rng(8)
    d2, r, lam = 70000, 4, 10.0
    lens = np.array([66000, d2, 10, 0, 300, 5000])
    d1 = len(lens)
    user = np.repeat(np.arange(d1), lens)
    item = np.concatenate([rng.choice(d2, n, replace=False) for n in lens])
    val = rng.integers(1, 6, user.shape[0]).astype(np.float64)
    X = oracle.build_csr(d1, d2, user, item, val)
    U0 = oracle.initial(d1, r) * 0.2; V0 = oracle.initial(d2, r) * 0.2
    ds = pcr.Dataset.from_triplets(d1, d2, user, item, val)
    s = pcr.Solver(ds, pcr.Parameter(k=r, precision=pcr.PCR_F64, **{"lambda": lam}))
    s.set_factors(U0, V0)
    mo = oracle.comp_m(U0, V0, X)
    assert rel(s.comp_m(), mo) < 1e-13
    assert abs(s.objective() / oracle.objective_new(mo, U0, V0, X, lam) - 1) < 1e-11
    assert rel(s.obtain_g(), oracle.obtain_g_new(U0, V0, X, mo, lam)) < 1e-10
    V1, m1, objVo, iv = oracle.update_V_new(X, lam, 1.0, U0, V0)
    U1, objUo, iu = oracle.update_U_new(X, m1, lam, 1.0, V1, U0)
    s.set_factors(U0, V0)
    objV, info_v = s.update_V()
    objU, info_u = s.update_U()
    Ug, Vg = s.get_factors()
    assert abs(objV / objVo - 1) < 1e-10 and abs(objU / objUo - 1) < 1e-10
    assert rel(Vg, V1) < 1e-7 and rel(Ug, U1) < 1e-7
    assert (info_v["cg"], info_v["ls"], info_u["cg"], info_u["ls"]) == (iv["cg"], iv["ls"], iu["cg"], iu["ls"])
    e, n = s.evaluate(0)
    eo, no = oracle.eval(Ug, Vg, X)
    assert abs(e - eo) < 1e-12 and abs(n - no) < 1e-12


def _one_outer_iteration_vs_oracle(oracle, d1, d2, user, item, val, r, lam, solver, precision=pcr.PCR_F64, scale=0.2, **par):
    X = oracle.build_csr(d1, d2, user, item, val)
    U0 = oracle.initial(d1, r) * scale; V0 = oracle.initial(d2, r) * scale
    U1, V1, ro = oracle.train(X, U0, V0, lam, 1, solver=solver, do_predict=0)
    ds = pcr.Dataset.from_triplets(d1, d2, user, item, val)
    s = pcr.Solver(ds, pcr.Parameter(k=r, precision=precision, solver_type=solver, maxiter=1, do_predict=0, **{"lambda": lam}, **par))
    s.set_factors(U0, V0)
    recs, _ = s.train()
    Ug, Vg = s.get_factors()
    t = TOL[precision]
    assert len(recs) == len(ro) == 2
    for a, b in zip(recs, ro):
        assert abs(a["obj"] / b["obj"] - 1) < max(t["obj"], t["fac"] * 1e-2), (a["obj"], b["obj"])
    assert rel(Vg, V1) < t["fac"] and rel(Ug, U1) < t["fac"]
    if precision == pcr.PCR_F64:
        a, b = recs[1], ro[1]
        assert (a["cg_v"], a["ls_v"], a["cg_u"], a["ls_u"]) == (b["cg_v"], b["ls_v"], b["cg_u"], b["ls_u"])
    return s


def test_cluster_class_mixes_level_counts(oracle):
    """The cluster class of the U step takes the longest users of SEVERAL length classes and runs them in the global-scratch
    form as soon as one of them needs it; its scratch slice must then be sized for the member with the MOST rating levels,
    not for the levels of the users beyond 4096 ratings (round-1 advice): one 5000-rating user with 5 levels next to
    3000- and 2040-rating users whose real-valued ratings are all distinct (PrimalCR: one level per rating), caps close
    to a power of two so that no padding hides an overrun.  One outer iteration against the oracle, counts included."""
    rng = np.random.default_rng(31)
    d2, r, lam = 8200, 6, 20.0
    lens = np.array([5000, 4090, 3000, 2040, 1030, 500, 100, 40, 7])
    d1 = len(lens)
    user = np.repeat(np.arange(d1), lens)
    item = np.concatenate([np.sort(rng.choice(d2, n, replace=False)) for n in lens])
    val = rng.normal(size=user.shape[0]) * 2.0                                 # all distinct: len levels under solver 1
    val[:5000] = rng.integers(1, 6, 5000)                                       # ... except the longest user: 5 levels
    _one_outer_iteration_vs_oracle(oracle, d1, d2, user, item, val, r, lam, solver=1)
    _one_outer_iteration_vs_oracle(oracle, d1, d2, user, item, val, r, lam, solver=2)


def test_u_step_classes_are_the_host_layout_at_this_devices_cu_count(tmp_path):
    """Ties csrc/check/classes_dump (tests/test_classes.py) to the solver: on that test's rating set, default knobs, the classes
    a solver lays out on this device are the ones the host-only layout prints for this device's CU count."""
    import torch

    import classes_data as cd
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    d1, d2, user, item, val = cd.rating_set()
    ds = pcr.Dataset.from_triplets(d1, d2, user, item, val)
    exe = cd.build_dump()
    for prec in cd.PRECISIONS:
        s = pcr.Solver(ds, pcr.Parameter(k=cd.K, precision=pcr.PCR_F64 if prec == "f64" else pcr.PCR_F32))
        rc, classes, _, out = cd.run_dump(exe, tmp_path, prec, {}, ncu)
        assert rc == 0, out
        assert s.ustep_classes() == [c["name"] for c in classes if c["users"] > 0]
        s.close()


@pytest.mark.parametrize("r", [200, 257])
def test_fp64_wide_ranks_with_users_near_4096_ratings(oracle, r):
    """fp64 at configs[4]'s rank and beyond with users of 2049..4096 ratings: the LDS-resident form of k_ustep would need
    more than the CU's 160 KB (22 B per rating + 136 B per rank column), so those classes must fall back to the
    global-scratch form instead of failing the launch (round-1 advice)."""
    rng = np.random.default_rng(r)
    d2, lam = 4300, 50.0
    lens = np.array([4096, 3974, 3000, 2049, 1500, 600, 130, 20])
    d1 = len(lens)
    user = np.repeat(np.arange(d1), lens)
    item = np.concatenate([np.sort(rng.choice(d2, n, replace=False)) for n in lens])
    val = rng.integers(1, 6, user.shape[0]).astype(np.float64)
    _one_outer_iteration_vs_oracle(oracle, d1, d2, user, item, val, r, lam, solver=2, scale=0.05)


def test_cluster_time_out_is_an_error_not_a_hang():
    """A workgroup cluster that loses a member must end in PCR_ERR_DEVICE through the bounded wait of its hand-off, not in
    a hung GPU.  pcr_tune("fault_cluster_member") makes the last member of every cluster leave at once."""
    R = synth.generate("small", seed=4, d1=40, d2=6000, nnz=60000, mu=7.0, sigma=0.6)       # users of ~1000-3000 ratings
    assert (np.bincount(R.user) > 1024).sum() >= 4
    ds = pcr.Dataset.from_ratings(R)
    with pcr.tuned(fault_cluster_member=1):
        s = pcr.Solver(ds, pcr.Parameter(k=8, precision=pcr.PCR_F32))
    s.set_factors(pcr.initial(R.d1, 8), pcr.initial(R.d2, 8))
    s.update_V()
    with pytest.raises(pcr.PcrError, match="timed out"):
        s.update_U()
    s.close()
    s = pcr.Solver(ds, pcr.Parameter(k=8, precision=pcr.PCR_F32))                # and the device is fine afterwards
    s.set_factors(pcr.initial(R.d1, 8), pcr.initial(R.d2, 8))
    s.update_V(); s.update_U()


def test_tight_cg_tolerance_uses_the_summed_residual(oracle):
    """cg_tol far below 1e-5: the V side's one-pass CG update derives |rr|^2 from a recurrence that cancels once the
    residual has dropped by ten orders of magnitude; below 1e-5 the stop test is taken on the directly summed residual
    (k_cg_stop).  Same iteration count as the oracle, whose residual is always summed (pcrpp.cpp:349-350)."""
    R = synth.generate("small", seed=9, d1=150, d2=90, nnz=5000, mu=3.2, sigma=0.9)
    r, lam = 6, 3.0
    X = oracle.build_csr(R.d1, R.d2, R.user, R.item, R.val)
    U = oracle.initial(R.d1, r) * 0.4; V = oracle.initial(R.d2, r) * 0.4
    ds = pcr.Dataset.from_triplets(R.d1, R.d2, R.user, R.item, R.val)
    try:
        oracle.set_cg(400, 1e-9)
        s = pcr.Solver(ds, pcr.Parameter(k=r, precision=pcr.PCR_F64, cg_max_iter=400, cg_tol=1e-9, **{"lambda": lam}))
        s.set_factors(U, V)
        mo = oracle.comp_m(U, V, X)
        s.comp_m()
        g = s.obtain_g()
        delta, its = s.solve_delta(g)
        do, its_o = oracle.solve_delta_new(oracle.obtain_g_new(U, V, X, mo, lam), mo, U, X, lam)
        assert abs(its - its_o) <= 1 and its < 400 and rel(delta, do) < 1e-7
        assert rel(s.compute_Ha(delta), g) < 1e-8                                  # H delta = g to the tolerance asked for
    finally:
        oracle.set_cg()


@pytest.mark.parametrize("precision", [pcr.PCR_F64, pcr.PCR_F32])
@pytest.mark.parametrize("solver,r", [(2, 10), (1, 10), (2, 100), (2, 132)])
def test_gram_u_step_against_oracle(oracle, precision, solver, r):
    """k_ustep_gram (pcr_gram.h): users with few ratings take their Newton step in the span of u_i and their rows of V,
    through the n x n Gram matrix built by MFMA (v_mfma_f32_32x32x2_f32 / v_mfma_f64_16x16x4_f64).  A set whose short
    users hit every tile count (1..128 ratings: 1-4 MFMA tiles a side in fp32, 1-4 in fp64 up to 64), users with no / one /
    all-equal ratings, rank below and above the rating counts (r = 10 < n, r = 100 ~ n, r = 132: k range of a lane not a
    multiple of 4).  Two outer iterations against the oracle, counts included in fp64."""
    rng = np.random.default_rng(5 + r)
    d2, lam = 1500, 25.0
    lens = np.concatenate([[0, 1, 2, 128, 127, 97, 96, 65, 64, 63, 33, 32, 31, 17, 16, 15, 5, 300, 1100], rng.integers(3, 129, 120)])
    d1 = len(lens)
    user = np.repeat(np.arange(d1), lens)
    item = np.concatenate([np.sort(rng.choice(d2, n, replace=False)) for n in lens])
    val = rng.integers(1, 6, user.shape[0]).astype(np.float64)
    val[user == 12] = 2.0                                                      # a user with all-equal ratings
    X = oracle.build_csr(d1, d2, user, item, val)
    U0 = oracle.initial(d1, r) * 0.3; V0 = oracle.initial(d2, r) * 0.3
    Uo, Vo, ro = oracle.train(X, U0, V0, lam, 2, solver=solver, do_predict=0)
    ds = pcr.Dataset.from_triplets(d1, d2, user, item, val)
    with pcr.tuned(ustep_gram=128):
        s = pcr.Solver(ds, pcr.Parameter(k=r, precision=precision, solver_type=solver, maxiter=2, do_predict=0, **{"lambda": lam}))
    s.profile(True)
    s.set_factors(U0, V0)
    recs, _ = s.train()
    assert any(name.startswith("ustep/gram") for name in s.profile_all()), "the dual-form class did not run"
    Ug, Vg = s.get_factors()
    t = TOL[precision]
    for a, b in zip(recs, ro):
        assert abs(a["obj"] / b["obj"] - 1) < max(t["obj"], t["fac"] * 1e-2), (a["obj"], b["obj"])
    assert rel(Vg, Vo) < t["fac"] and rel(Ug, Uo) < t["fac"]
    if precision == pcr.PCR_F64:
        for a, b in zip(recs[1:], ro[1:]):
            assert (a["cg_v"], a["ls_v"], a["cg_u"], a["ls_u"]) == (b["cg_v"], b["ls_v"], b["cg_u"], b["ls_u"])


def test_gram_u_step_line_search_retries(oracle):
    """The dual form's line search never touches a row of V (m_new = (1 - s alpha_d) m - s K a_delta): with an initial step of
    50 most users halve several times; counts, objective and factors as the oracle's, and the state it leaves starts the
    next V step exactly like the per-user kernel's."""
    R = synth.generate("small", seed=12, d1=300, d2=200, nnz=20000, mu=3.8, sigma=0.8)
    r, lam, step = 6, 1e-3, 50.0
    X = oracle.build_csr(R.d1, R.d2, R.user, R.item, R.val)
    U0 = oracle.initial(R.d1, r); V0 = oracle.initial(R.d2, r)
    m0 = oracle.comp_m(U0, V0, X)
    U1, objUo, iu = oracle.update_U_new(X, m0, lam, step, V0, U0)
    ds = pcr.Dataset.from_ratings(R)
    with pcr.tuned(ustep_gram=128):
        s = pcr.Solver(ds, pcr.Parameter(k=r, precision=pcr.PCR_F64, stepsize=step, **{"lambda": lam}))
    s.set_factors(U0, V0)
    s.comp_m(want=False)
    objU, info = s.update_U()
    Ug, _ = s.get_factors()
    assert (info["cg"], info["ls"]) == (iu["cg"], iu["ls"]) and iu["ls"] > 2 * R.d1
    assert abs(objU / objUo - 1) < 1e-9 and rel(Ug, U1) < 1e-7
    oV, iv = s.update_V()
    V2, m2, objVo, ivo = oracle.update_V_new(X, lam, step, U1, V0)
    assert (iv["cg"], iv["ls"]) == (ivo["cg"], ivo["ls"]) and abs(oV / objVo - 1) < 1e-9
