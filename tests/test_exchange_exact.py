"""The rank-to-rank exchange (pcr_p2p.h) held to exact parity on every form, on every rank.

allreduce_T / allreduce_f64 of pcr_solver.hip sum the V-side vectors (g, every Hp of the CG) and the objective's scalars across
the ranks.  With the peer-to-peer communicator that sum has four forms: device-driven (k_p2p_ll: value and sequence number in
one 8-byte word, fp64 as two words), host-synchronised one-shot (messages of at most 256 KB), host-synchronised two-phase
(reduce-scatter + all-gather over slices of per = ceil(n / nranks) elements, double-buffered by call parity), and any of them
item range by item range (allreduce_chunks > 1, on a stream of its own).  pcr_p2p.h promises "every rank obtains
bitwise-identical sums (fixed order), which the replicated CG recurrence relies on"; this file holds it to that.

On the dyadic data of tests/exact_data.py every shard's partial g, Ha and objective is a whole number of quarter (sixteenth)
units, exact in fp32 and fp64 in any order, so the all-reduced result ON EVERY RANK must equal the oracle BIT FOR BIT whatever
the form, the slice size or the order of the ranks: one dropped, doubled or misplaced element, one stale word of the other
parity or of an earlier sequence number, changes an integer.

Part 1 (CPU) proves with the oracle alone that the shards' partials are exact, add up exactly, and that the exchange is needed
and visible everywhere.  Part 2 (GPU) runs the first-order entry points through the live exchange, n ranks as n fresh processes
on device 0, and compares every rank with the oracle in the parent.  Part 3 (GPU) runs two outer iterations on every rank: the
replicas must stay bit-identical to each other and within the project's own bounds of the one-rank run.

Every child runs under a time limit; once a child of this file has ended by a signal or at its limit, every later cell of the
file skips: nothing more is started on the device after a fault or a stall.
"""
import itertools
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import exact_data as ed
import primalcr_amd as pcr
from test_exact_parity import assert_same, is_f32, reference, where_item
from test_gpu_parity import TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREC = {"F64": pcr.PCR_F64, "F32": pcr.PCR_F32}
ESIZE = {"F64": 8, "F32": 4}
ONE_SHOT_BYTES = 256 << 10                  # pcr_p2p.h, P2PComm::allreduce: messages of at most 256 KB skip the second phase
SK_LIST = ((2, 12), (2, 100), (1, 12))      # (solver, k) of test_user_shards_add_up_exactly
CHILD_LIMIT_S = 120
MAX_CHILDREN = 7


def ld_of(k):
    return (k + 3) & ~3


# ------------------------------------------------------------------------------------------------------------------------------
# fixtures: the default dyadic case and the smaller ones of the cells (all through one cache; the oracle runs once per case)
# ------------------------------------------------------------------------------------------------------------------------------

FIXTURES = {"default": dict(d1=700, d2=6000),
            "d6001": dict(d1=700, d2=6001),       # d2 * ld not divisible by 5 or 7: the last slice is shorter
            "t8192": dict(d1=300, d2=8192),       # k = 7, F32: exactly 262 144 bytes, the largest one-shot message
            "t8193": dict(d1=300, d2=8193)}       # ... and the smallest two-phase one


def skew_case(fx, r, solver):
    """A rank without users: 40 users over 300 items, one user rating every item, 7 - 10 users rating nothing.  pcr_partition_users
    leaves rank q empty when one user's ratings span the targets q nnz / n and (q + 1) nnz / n, and the other ranks' users must
    still rate 90 % of the items for the exchange to be visible there, so each rank count has its own layout:
      skew4 (4 ranks): user 0 rates all 300 items, users 1 .. 29 rate 10 items each, 290 distinct ones spread over the item axis
            (nnz = 590, targets 147.5 / 295 / 442.5: bounds 0, 1, 1, 16, 40 -- user 0 holds 50.8 % of the ratings);
      skew3 (3 ranks): users 0 .. 17 rate 15 items each, user 18 rates all 300, users 19 .. 32 rate 20 items each, 280 distinct ones
            (nnz = 850, targets 283.3 / 566.7: bounds 0, 19, 19, 40 -- the heavy user sits in the middle and holds 35 %: at 3 ranks
            a user with more than half of the ratings leaves the others at most 300 ratings on either side, which cannot cover
            90 % of the items on a second rank and keep a rank empty)."""
    rng = np.random.default_rng(5)
    c = ed.Case()
    c.r, c.solver, c.seed, c.real, c.lam = int(r), int(solver), 0, False, ed.LAMBDA
    c.d1, c.d2 = 40, 300
    every = np.arange(300)
    if fx == "skew4":
        pool = every[every % 30 != 29]                                   # 290 items
        rows = [every] + [pool[u + 29 * np.arange(10)] for u in range(29)]
    else:
        pre, post = every[every % 10 != 9], every[every % 15 != 14]      # 270 and 280 items
        rows = [pre[u + 18 * np.arange(15)] for u in range(18)] + [every] + [post[v + 14 * np.arange(20)] for v in range(14)]
    c.user = np.concatenate([np.full(len(x), u, np.int64) for u, x in enumerate(rows)])
    c.item = np.concatenate([np.sort(x) for x in rows]).astype(np.int64)
    c.val = rng.integers(1, 6, c.user.shape[0]).astype(np.float64)
    c.U = ed.dyadic_matrix(rng, c.d1, r, 1.0); c.V = ed.dyadic_matrix(rng, c.d2, r, 1.0)
    c.a = ed.dyadic_matrix(rng, c.d2, r, 1.0); c.a2 = ed.dyadic_matrix(rng, c.d2, r, 1.0)
    return c


_REF = {}


def ref_case(oracle, fx, r, solver):
    """The case and the oracle's objective, g and Ha for both probes.  The default case is test_exact_parity's own (one cache)."""
    if fx == "default":
        return reference(oracle, r, solver)
    key = (fx, r, solver)
    if key not in _REF:
        c = skew_case(fx, r, solver) if fx.startswith("skew") else ed.dyadic_case(r, solver, **FIXTURES[fx])
        c.X = X = oracle.build_csr(c.d1, c.d2, c.user, c.item, c.val)
        c.m = oracle.comp_m(c.U, c.V, X)
        c.obj = oracle.objective_new(c.m, c.U, c.V, X, c.lam, solver=solver)
        c.g = oracle.obtain_g_new(c.U, c.V, X, c.m, c.lam, solver=solver)
        c.Ha = oracle.compute_Ha_new(c.a, c.m, c.U, X, c.lam, solver=solver)
        c.Ha2 = oracle.compute_Ha_new(c.a2, c.m, c.U, X, c.lam, solver=solver)
        c.lens = np.diff(X.idx)
        _REF[key] = c
    return _REF[key]


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the precondition, on the CPU
# ------------------------------------------------------------------------------------------------------------------------------

def shard_partials(oracle, c, nranks):
    """What every rank contributes, computed by the oracle on the rank's rows alone (rank 0 carries the lambda term, as
    Solver::device_gradient / device_hv seed it): [(g_q, Ha_q, loss_q)], and the user bounds."""
    from oracle.oracle_py import CSR
    X = c.X
    b = pcr.partition_users(X.idx, nranks)
    parts = []
    for q in range(nranks):
        u0, u1 = int(b[q]), int(b[q + 1])
        z0, z1 = int(X.idx[u0]), int(X.idx[u1])
        Xs = CSR(u1 - u0, X.d2, X.idx[u0:u1 + 1] - z0, X.item[z0:z1], X.val[z0:z1])
        Us = c.U[u0:u1]
        lam_q = c.lam if q == 0 else 0.0
        if u1 > u0:
            m_s = oracle.comp_m(Us, c.V, Xs)
            g = oracle.obtain_g_new(Us, c.V, Xs, m_s, lam_q, solver=c.solver)
            Ha = oracle.compute_Ha_new(c.a, m_s, Us, Xs, lam_q, solver=c.solver)
            loss = oracle.objective_new(m_s, Us * 0, c.V * 0, Xs, 0.0, solver=c.solver)
        else:
            g, Ha, loss = lam_q * c.V, lam_q * c.a, 0.0
        parts.append((g, Ha, loss))
    return parts, b


def padded(x, ld):
    out = np.zeros((x.shape[0], ld))
    out[:, :x.shape[1]] = x
    return out.ravel()


CPU_CASES = ([("default", n, s, k) for n in (2, 3, 5) for s, k in SK_LIST] + [("d6001", 5, 2, 12), ("d6001", 7, 2, 12)] +
             [("t8192", 3, 2, 7), ("t8193", 3, 2, 7), ("skew4", 4, 2, 12), ("skew3", 3, 2, 12)])


@pytest.mark.parametrize("fx,nranks,solver,k", CPU_CASES, ids=[f"{f}-n{n}-s{s}-k{k}" for f, n, s, k in CPU_CASES])
def test_shard_partials_are_exact_and_the_exchange_is_visible_everywhere(oracle, fx, nranks, solver, k):
    """With the oracle alone: the partial g and Ha of every pcr_partition_users shard are multiples of 1/4 and their own float32
    round trip, and add up to the full result exactly (so do the losses, in sixteenths).  And the exchange is needed and visible:
    at least 90 % of the items have a non-zero partial g row on two ranks or more, every rank's partial has a non-zero entry
    inside every rank's slice [q per, (q + 1) per) of the padded vector, and every rank's partial differs from the total -- a
    rank that skipped the exchange, or one slice of it, cannot pass Part 2.

    The fixtures with a rank without users (skew_case) are held to the same 90 %; the per-slice and differs-from-the-total
    checks apply to the ranks that have users, and the empty rank's partial is asserted to be all zeros: it takes part in every
    exchange contributing nothing."""
    c = ref_case(oracle, fx, k, solver)
    parts, b = shard_partials(oracle, c, nranks)
    ld = ld_of(k)
    n = c.d2 * ld
    per = -(-n // nranks)
    for name, tot, col in (("g", c.g, 0), ("Ha", c.Ha, 1)):
        assert is_f32(tot) and np.abs(tot).max() * ed.UNIT < 2 ** 22, name
        acc = np.zeros_like(tot)
        for q, p in enumerate(parts):
            x = p[col]
            assert is_f32(x) and np.array_equal(x * ed.UNIT, np.rint(x * ed.UNIT)), (name, q)
            acc = acc + x
            assert is_f32(acc), (name, q)                                # the running sums in rank order are fp32-exact too
        assert np.array_equal(acc, tot), name
    reg = c.lam / 2.0 * float((c.U ** 2).sum() + (c.V ** 2).sum())
    assert sum(p[2] for p in parts) + reg == c.obj and all(p[2] * 16 == np.rint(p[2] * 16) for p in parts)
    empty = [q for q in range(nranks) if b[q] == b[q + 1]]
    if fx.startswith("skew"):
        assert empty == [1], b
        # one user rates every item: more than half of all ratings at 4 ranks, more than a third at 3 (skew_case says why)
        assert c.lens.max() == c.d2 and c.lens.max() * (2 if nranks == 4 else 3) > c.lens.sum() and np.sort(c.lens)[-2] <= 20
    else:
        assert not empty, b
    nz_rows = np.stack([np.abs(p[0]).sum(1) > 0 for p in parts])         # rank x item
    share = float((nz_rows.sum(0) >= 2).mean())
    print(f"[exchange-exact] {fx}, {nranks} ranks, solver {solver}, k = {k}: {100 * share:.2f} % of the items have a non-zero partial g row on >= 2 ranks")
    for q, p in enumerate(parts):
        for name, x, tot in (("g", p[0], c.g), ("Ha", p[1], c.Ha)):
            if q in empty:
                assert not x.any(), (name, q)
                continue
            assert not np.array_equal(x, tot), (name, q)
            flat = padded(x, ld)
            for o in range(nranks):
                assert flat[o * per:min(n, (o + 1) * per)].any(), f"{name}: rank {q}'s partial is zero in all of rank {o}'s slice"
    assert share >= 0.9, share


# ------------------------------------------------------------------------------------------------------------------------------
# the job harness
# ------------------------------------------------------------------------------------------------------------------------------

WORKER = r'''
import json, sys, time
import numpy as np
sys.path.insert(0, sys.argv[1])
import primalcr_amd as pcr
job = json.load(open(sys.argv[2])); q = int(sys.argv[3])
n = job["nranks"]
PREC = {"F64": pcr.PCR_F64, "F32": pcr.PCR_F32}
cases, out = {}, {}

def case(path):
    if path not in cases:
        c = dict(np.load(path))
        c["ds"] = pcr.Dataset.from_triplets(int(c["d1"]), int(c["d2"]), c["user"], c["item"], c["val"])
        cases[path] = c
    return cases[path]

for i, sv in enumerate(job["solvers"]):
    t0 = time.time()
    print(f"@@ solver {i}", file=sys.stderr, flush=True)
    c = case(sv["case"])
    par = pcr.Parameter(k=sv["k"], solver_type=sv["solver"], precision=PREC[sv["prec"]], device=q if job.get("per_device") else 0,
                        **{"lambda": float(c["lam"])})
    with pcr.tuned(lanes=1, debug=1, **sv["knobs"]):
        s = pcr.Solver(c["ds"], par, rank=q, nranks=n)
        if "uid" in sv:
            s.comm_init(open(sv["uid"], "rb").read())
        else:
            s.comm_init_p2p(sv["name"])
    assert s.comm_nranks() == n, (s.comm_nranks(), n)
    out[f"{i}.first_user"], out[f"{i}.n_users"] = s.first_user, s.n_users
    s.set_factors(c["U"], c["V"])
    if sv["mode"] == "first":
        s.comp_m(False)
        out[f"{i}.obj1"] = s.objective()
        out[f"{i}.g1"] = s.obtain_g()
        out[f"{i}.Ha"] = s.compute_Ha(c["a"])
        out[f"{i}.Ha2"] = s.compute_Ha(c["a2"])
        out[f"{i}.g2"] = s.obtain_g()
        out[f"{i}.obj2"] = s.objective()
        s.set_local_only(True)
        out[f"{i}.g_local"] = s.obtain_g()
        s.set_local_only(False)
        out[f"{i}.g3"] = s.obtain_g()
    elif sv["mode"] == "steps":
        s.comp_m(False)
        d, it = s.solve_delta(c["g"])
        out[f"{i}.delta"], out[f"{i}.delta_it"] = d, it
        s.set_factors(c["U"], c["V"])
        objs, counts = [], []
        for _ in range(2):
            oV, iv = s.update_V(); oU, iu = s.update_U()
            objs += [oV, oU]; counts += [iv["cg"], iv["ls"], iv["accepted"], iu["cg"], iu["ls"]]
        out[f"{i}.objs"], out[f"{i}.counts"] = np.array(objs), np.array(counts, np.int64)
        out[f"{i}.U"], out[f"{i}.V"] = s.get_factors_local()
    else:
        recs = s.iterate(2)
        out[f"{i}.objs"] = np.array([r["obj"] for r in recs])
        out[f"{i}.counts"] = np.array([[r["cg_v"], r["ls_v"], r["cg_u"], r["ls_u"]] for r in recs], np.int64).ravel()
        out[f"{i}.U"], out[f"{i}.V"] = s.get_factors_local()
    # how many vector exchanges one obtain_g() issues: one per item range (the "allreduce" slot counts launches once profiling is on)
    s.comp_m(False)
    s.profile(True, period=1000); s.profile_reset()
    s.obtain_g()
    out[f"{i}.exchanges_per_vector"] = s.profile_launches("allreduce")
    s.profile(False)
    s.close()
    out[f"{i}.seconds"] = time.time() - t0
np.savez(job["out"] + f"/rank{q}.npz", **out)
'''

_STOP = {"reason": None}            # set once a child ended by a signal or at its limit: every later cell of this file skips
_COUNTER = itertools.count()
P2P_LINE = re.compile(r"^\[pcr\] p2p: (\d+) ranks, vectors up to (\d+) bytes (device-driven|-- every exchange host-synchronised)", re.M)


@pytest.fixture(scope="module")
def casedir(tmp_path_factory):
    return tmp_path_factory.mktemp("exchange_cases")


def case_file(casedir, c, fx):
    path = casedir / f"{fx}_k{c.r}_s{c.solver}.npz"
    if not path.exists():
        np.savez(path, d1=c.d1, d2=c.d2, user=c.user, item=c.item, val=c.val, U=c.U, V=c.V, a=c.a, a2=c.a2, lam=c.lam, g=c.g)
    return str(path)


def run_job(cell, tmp_path, nranks, solvers, per_device=False):
    """nranks fresh children, one per rank; returns ([rank's results], [rank 0's stderr per solver])."""
    if _STOP["reason"]:
        pytest.skip(_STOP["reason"])
    assert nranks <= MAX_CHILDREN
    t0 = time.time()
    (tmp_path / "worker.py").write_text(WORKER)
    for sv in solvers:
        if "uid" not in sv:
            sv["name"] = f"/pcr_xe_{os.getpid()}_{next(_COUNTER)}"
    (tmp_path / "job.json").write_text(json.dumps(dict(nranks=nranks, solvers=solvers, out=str(tmp_path), per_device=per_device)))
    # (output into files, not pipes: a rank blocked on a full pipe while the parent waits for another rank would stall the job)
    logs = [open(tmp_path / f"rank{q}.log", "w") for q in range(nranks)]
    procs = [subprocess.Popen([sys.executable, str(tmp_path / "worker.py"), ROOT, str(tmp_path / "job.json"), str(q)], stdout=logs[q],
                              stderr=subprocess.STDOUT, text=True, cwd=str(tmp_path)) for q in range(nranks)]
    late = False
    try:
        deadline = time.time() + CHILD_LIMIT_S
        for p in procs:
            try:
                p.communicate(timeout=max(0.1, deadline - time.time()))
            except subprocess.TimeoutExpired:
                late = True
                break
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        for p in procs:
            p.wait()
        for f in logs:
            f.close()
    outs = [(tmp_path / f"rank{q}.log").read_text() for q in range(nranks)]
    codes = [p.returncode for p in procs]
    errs = "\n".join(f"--- rank {q} (exit {codes[q]}):\n{outs[q][-1500:]}" for q in range(nranks) if codes[q] != 0)
    if late or any(rc < 0 for rc in codes):
        _STOP["reason"] = (f"cell {cell}: a child " + (f"ran into its {CHILD_LIMIT_S} s limit" if late else "ended by a signal") +
                           f" (exit codes {codes}); nothing more of this file is started on the device")
        pytest.fail(_STOP["reason"] + "\n" + errs)
    if any("timed out" in outs[q] for q in range(nranks) if codes[q] != 0):
        _STOP["reason"] = f"cell {cell}: an exchange timed out (exit codes {codes}); nothing more of this file is started on the device"
        pytest.fail(_STOP["reason"] + "\n" + errs)
    assert not any(codes), f"cell {cell}: exit codes {codes}\n{errs}"
    res = [dict(np.load(tmp_path / f"rank{q}.npz")) for q in range(nranks)]
    sections = re.split(r"^@@ solver \d+\n", outs[0], flags=re.M)[1:]
    assert len(sections) == len(solvers), outs[0][-1500:]
    print(f"[exchange-exact] cell {cell}: {nranks} children, {len(solvers)} solvers, {time.time() - t0:.1f} s "
          f"(slowest solver on rank 0: {max(float(res[0][f'{i}.seconds']) for i in range(len(solvers))):.2f} s)")
    return res, sections


def assert_form(cell, section, nranks, want, vec_bytes):
    """The debug line of rank 0 names the form this job took; want: 'll' (vectors and scalars device-driven), 'host' (every
    exchange host-synchronised), 'mixed' (limit 1 MB: scalars device-driven, the vectors above it host-synchronised)."""
    notes = [l for l in section.splitlines() if l.startswith("[pcr] p2p")]
    m = P2P_LINE.findall(section)
    assert len(m) == 1 and int(m[0][0]) == nranks, (cell, notes)
    limit, form = int(m[0][1]), m[0][2]
    if want == "host":
        assert form.endswith("host-synchronised") and limit == 0, (cell, notes)
        return
    assert form == "device-driven" and not any("ranks share device" in l or "host-synchronised exchange" in l for l in notes), \
        f"cell {cell} is a device-driven cell, but the job was switched to the host-synchronised exchange: {notes}"
    if want == "ll":
        assert limit >= vec_bytes, (cell, limit, vec_bytes, notes)
    else:
        assert limit == 1 << 20 and limit < vec_bytes, (cell, limit, vec_bytes, notes)


def assert_ranges(cell, res, i, nranks, knobs, d2):
    """The item ranges were really taken: one obtain_g() issued one vector exchange per range on every rank (the solver drops
    allreduce_chunks silently under the blocked-user V step, and the plan clamps it to 64 and to d2)."""
    want = max(1, min(int(knobs.get("allreduce_chunks", 0)) or 1, 64, d2))
    got = [int(res[q][f"{i}.exchanges_per_vector"]) for q in range(nranks)]
    assert got == [want] * nranks, f"cell {cell}: {got} vector exchanges per obtain_g() on the ranks, {want} item range(s) expected"


def vector_form(want, nbytes):
    return "device-driven" if want == "ll" else "one-shot" if nbytes <= ONE_SHOT_BYTES else "two-phase"


def owner_text(ex):
    """where(c, flat) for assert_same: test_exact_parity's item text plus which message and slice the element travelled in."""
    def where(c, z):
        it, col = divmod(int(z), c.r)
        ld, nr = ld_of(c.r), ex["nranks"]
        n_rng = max(1, min(ex["chunks"] or 1, 64, c.d2))
        cuts = [c.d2 * r // n_rng for r in range(n_rng + 1)]
        rg = max(r for r in range(n_rng) if cuts[r] <= it)
        pos, n_msg = (it - cuts[rg]) * ld + col, (cuts[rg + 1] - cuts[rg]) * ld
        if ex["want"] == "ll":
            per, kind = -(-c.d2 * ld // nr), "device-driven"
        elif n_msg * ex["esize"] <= ONE_SHOT_BYTES:
            return f"{where_item(c, z)}; item range {rg}, one-shot: every rank sums element {pos} of the message itself"
        else:
            per, kind = -(-n_msg // nr), "two-phase"
        return f"{where_item(c, z)}; {kind}, item range {rg}, element {pos} of the message: slice owner rank {pos // per} (per = {per})"
    return where


def check_first_order(cell, res, i, c, sv, ex):
    nranks = ex["nranks"]
    where = owner_text(ex)
    for q in range(nranks):
        R = res[q]
        tag = f"cell {cell}, rank {q} of {nranks}, {sv['prec']}, solver {sv['solver']}, k = {sv['k']}"
        for name in ("obj1", "obj2"):
            obj = float(R[f"{i}.{name}"])
            assert obj == c.obj, f"{tag}: objective() ({name}) {obj!r}, oracle {c.obj!r} ({(obj - c.obj) * 16:g} sixteenths)"
        for key, name, ref in (("g1", "obtain_g()", c.g), ("Ha", "compute_Ha(a)", c.Ha), ("Ha2", "compute_Ha(a2)", c.Ha2),
                               ("g2", "obtain_g() after the probes", c.g), ("g3", "obtain_g() after set_local_only(False)", c.g)):
            assert_same(tag, name, R[f"{i}.{key}"], ref, c, where)
        assert not np.array_equal(R[f"{i}.g_local"], c.g), f"{tag}: obtain_g() under set_local_only(True) equals the total -- the sum did not go through the exchange"
    # (the objective's scalars travel in the scalar box set / slot, of which rank 0 owns everything: the last rank has it all from a peer)
    assert float(res[nranks - 1][f"{i}.obj1"]) == c.obj and float(res[nranks - 1][f"{i}.obj2"]) == c.obj
    # the shard-local partials are the ones that add up to the total
    assert_same(f"cell {cell}", "sum of the ranks' local-only g", sum(res[q][f"{i}.g_local"] for q in range(nranks)), c.g, c, where)
    b = pcr.partition_users(c.X.idx, nranks)
    assert [(int(res[q][f"{i}.first_user"]), int(res[q][f"{i}.n_users"])) for q in range(nranks)] == [(int(b[q]), int(b[q + 1] - b[q])) for q in range(nranks)]


def first_order_cell(oracle, casedir, tmp_path, cell, nranks, want, prec, specs, knobs, per_device=False, rccl=False):
    """specs: [(fixture, solver, k, expected vector form or None)]; one job, one solver per spec."""
    solvers, cs = [], []
    for j, (fx, solver, k, _) in enumerate(specs):
        c = ref_case(oracle, fx, k, solver)
        cs.append(c)
        sv = dict(case=case_file(casedir, c, fx), k=k, solver=solver, prec=prec, knobs=knobs, mode="first")
        if rccl:
            (tmp_path / f"uid{j}").write_bytes(pcr.comm_unique_id())
            sv["uid"] = str(tmp_path / f"uid{j}")
        solvers.append(sv)
    for (fx, solver, k, form), c in zip(specs, cs):
        nbytes = c.d2 * ld_of(k) * ESIZE[prec]
        if form is not None and not knobs.get("allreduce_chunks"):
            assert vector_form(want, nbytes) == form, (fx, k, prec, nbytes)
    res, sections = run_job(cell, tmp_path, nranks, solvers, per_device)
    for i, (sv, c) in enumerate(zip(solvers, cs)):
        nbytes = c.d2 * ld_of(sv["k"]) * ESIZE[prec]
        if not rccl:
            assert_form(cell, sections[i], nranks, want, nbytes)
        assert_ranges(cell, res, i, nranks, knobs, c.d2)
        ex = dict(nranks=nranks, want="ll" if want == "ll" else "host", chunks=int(knobs.get("allreduce_chunks", 0)), esize=ESIZE[prec])
        check_first_order(cell, res, i, c, sv, ex)


def form_id(want, prec, specs):
    """'s2k7:192000B:one-shot+...': per solver of the job, the bytes of its full V-side vector and the form that follows."""
    return "+".join(f"{'' if fx == 'default' else fx + ':'}s{s}k{k}:{c_bytes(fx, k, prec)}B:{vector_form(want, c_bytes(fx, k, prec))}" for fx, s, k, _ in specs)


def c_bytes(fx, k, prec):
    d2 = 300 if fx.startswith("skew") else FIXTURES[fx]["d2"]
    return d2 * ld_of(k) * ESIZE[prec]


# ------------------------------------------------------------------------------------------------------------------------------
# 2. first-order entry points through the live exchange, exact on every rank
# ------------------------------------------------------------------------------------------------------------------------------

DEFAULT3 = [("default", s, k, None) for s, k in SK_LIST]
LADDER = {"F32": [("default", 2, 1, "one-shot"), ("default", 2, 7, "one-shot"), ("default", 2, 12, "two-phase"), ("default", 1, 12, "two-phase"),
                  ("default", 2, 100, "two-phase")],
          "F64": [("default", 2, 1, "one-shot"), ("default", 2, 7, "two-phase"), ("default", 2, 12, "two-phase"), ("default", 1, 12, "two-phase"),
                  ("default", 2, 100, "two-phase")]}
CELLS = []


def cell(name, nranks, want, prec, specs, knobs):
    ident = f"{name}-n{nranks}-{prec}-{form_id(want, prec, specs)}"
    CELLS.append(pytest.param(ident, nranks, want, prec, specs, knobs, id=ident))


for _n in (2, 3):                                                                   # 1. device-driven, default knobs
    for _p in ("F32", "F64"):
        cell("1-device-driven", _n, "ll", _p, DEFAULT3 + ([("default", 2, 1, None), ("default", 2, 132, None)] if _n == 3 else []), {})
for _p in ("F32", "F64"):                                                           # 2. host-synchronised: one-shot and two-phase
    cell("2-host-ladder", 3, "host", _p, LADDER[_p], {"p2p_ll": 0})
for _n, _p in ((5, "F32"), (5, "F64"), (7, "F32")):                                 # 3. unequal slices, two-phase
    cell("3-unequal-slices", _n, "host", _p, [("d6001", 2, 12, "two-phase"), ("d6001", 1, 12, "two-phase")], {"p2p_ll": 0})
cell("4-threshold", 3, "host", "F32", [("t8192", 2, 7, "one-shot"), ("t8193", 2, 7, "two-phase")], {"p2p_ll": 0})
for _p in ("F32", "F64"):                                                           # 5. two forms in one job
    cell("5-two-forms", 2, "mixed", _p, [("default", 2, 100, "two-phase")], {"p2p_ll": 1})
for _p in ("F32", "F64"):                                                           # 6. item ranges over both forms
    for _ch in (3, 7):
        cell(f"6-item-ranges-{_ch}", 2, "ll", _p, [("default", 2, 12, None), ("default", 2, 100, None)], {"allreduce_chunks": _ch})
        cell(f"6-item-ranges-{_ch}", 3, "host", _p, [("default", 2, 12, None), ("default", 2, 100, None)], {"allreduce_chunks": _ch, "p2p_ll": 0})
cell("7-rank-without-users", 4, "host", "F32", [("skew4", 2, 12, "one-shot")], {"p2p_ll": 0})
cell("7-rank-without-users", 3, "ll", "F32", [("skew3", 2, 12, None)], {})


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("ident,nranks,want,prec,specs,knobs", CELLS)
def test_first_order_entry_points_are_exact_on_every_rank(oracle, casedir, tmp_path, ident, nranks, want, prec, specs, knobs):
    """objective(), obtain_g(), compute_Ha(a), compute_Ha(a2), obtain_g() and objective() again: equal to the oracle bit for
    bit on EVERY rank of the job, in the form the cell is named for (asserted from rank 0's debug line; a device-driven cell
    fails with the note's text if the job was switched to the host-synchronised exchange).  Under set_local_only(True) every
    rank's obtain_g() differs from the oracle -- the sum really went through the exchange -- the local partials add up to it
    exactly, and after set_local_only(False) it is exact again.  The cell id carries the bytes of the full V-side vector and
    the form that follows from them (with item ranges every range is a message of its own: a third or a seventh of that).

    That the item ranges were really taken is asserted too: with profiling on, the "allreduce" slot counts one launch per range
    for one obtain_g() (1 in every other cell).  Cell 6 over the device-driven form runs with 2 ranks: the item ranges' stream is one more hardware queue per rank.  The
    sub-range messages are shorter than per, so rank 0 owns whole ranges there.  A failure names cell, rank, entry point, the
    first differing (item, column), its raters, and the slice owner of that element."""
    first_order_cell(oracle, casedir, tmp_path, ident, nranks, want, prec, specs, knobs)


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("comm", ["p2p", "rccl"])
@pytest.mark.parametrize("prec", ["F32", "F64"])
def test_first_order_entry_points_are_exact_across_two_devices(oracle, casedir, tmp_path, prec, comm):
    """Cell 8: cell 1's 2-rank list with one rank per physical device, over comm_init_p2p (xGMI between the boxes) and over RCCL
    (the unique id handed to the children through a file).  Skipped where the machine has one device."""
    import torch
    ndev = torch.cuda.device_count()
    if ndev < 2:
        pytest.skip(f"needs two devices, torch.cuda.device_count() = {ndev}")
    first_order_cell(oracle, casedir, tmp_path, f"8-two-devices-{comm}-{prec}", 2, "ll", prec, DEFAULT3, {}, per_device=True, rccl=comm == "rccl")


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the replicas stay identical
# ------------------------------------------------------------------------------------------------------------------------------

_ONE = {}


def one_rank(c, prec, k):
    """The one-process run of the same calls (default knobs): what the project compares an N-rank job with."""
    key = (c.d2, prec, k)
    if key not in _ONE:
        par = dict(k=k, solver_type=2, precision=PREC[prec], **{"lambda": c.lam})
        ds = pcr.Dataset.from_triplets(c.d1, c.d2, c.user, c.item, c.val)
        s = pcr.Solver(ds, pcr.Parameter(**par))
        s.set_factors(c.U, c.V); s.comp_m(False)
        delta, it = s.solve_delta(c.g)
        s.set_factors(c.U, c.V)
        objs, counts = [], []
        for _ in range(2):
            oV, iv = s.update_V(); oU, iu = s.update_U()
            objs += [oV, oU]; counts += [iv["cg"], iv["ls"], iv["accepted"], iu["cg"], iu["ls"]]
        U, V = s.get_factors()
        s.close()
        t = pcr.Solver(ds, pcr.Parameter(**par))
        t.set_factors(c.U, c.V)
        recs = t.iterate(2)
        Ui, Vi = t.get_factors()
        t.close()
        _ONE[key] = dict(delta=delta, delta_it=it, steps=(np.array(objs), np.array(counts, np.int64), U, V),
                         iterate=(np.array([r["obj"] for r in recs]), np.array([[r["cg_v"], r["ls_v"], r["cg_u"], r["ls_u"]] for r in recs], np.int64).ravel(), Ui, Vi))
    return _ONE[key]


def first_difference(a, b):
    bad = np.flatnonzero(np.asarray(a).ravel() != np.asarray(b).ravel())
    return None if not bad.size else int(bad[0])


REPLICA_CONFIGS = [("device-driven", 2, "ll", "default", {}), ("device-driven", 3, "ll", "default", {}),
                   ("two-phase", 5, "host", "d6001", {"p2p_ll": 0}),
                   ("item-ranges-3-device-driven", 2, "ll", "default", {"allreduce_chunks": 3}),
                   ("item-ranges-3-host", 3, "host", "default", {"allreduce_chunks": 3, "p2p_ll": 0})]
_WORST = {"F32": 0.0, "F64": 0.0}


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("prec", ["F32", "F64"])
@pytest.mark.parametrize("name,nranks,want,fx,knobs", REPLICA_CONFIGS, ids=[f"{c[0]}-n{c[1]}" for c in REPLICA_CONFIGS])
def test_replicas_stay_identical_over_two_iterations(oracle, casedir, tmp_path, name, nranks, want, fx, knobs, prec):
    """From the dyadic start, on every rank of a job: solve_delta(g), then update_V(); update_U() twice, and in a second solver
    iterate(2), at k = 12 and k = 100 -- on the order of a hundred exchanges per solver, both call parities and a run of LL
    sequence numbers.  ACROSS RANKS the full V, the CG direction, the objectives of the half steps and every cg / ls count are
    bit-identical (the replicated recurrence has nothing else to keep the replicas together).  AGAINST ONE RANK, the project's
    own numbers: fp64 max |d| < 1e-9 max |.| on the factors (tests/test_cli.py) and equal CG / line-search counts; fp32
    TOL[PCR_F32]["fac"] of tests/test_gpu_parity.py; the ranks' U rows concatenated against the one-rank U under the same
    bounds, and so is the solve_delta direction.  Every cell also asserts the number of vector exchanges one obtain_g() issues
    (one per item range).  The largest difference to the one-rank run is printed."""
    cell = f"replicas-{name}-n{nranks}-{prec}"
    solvers, cs = [], []
    for k in (12, 100):
        c = ref_case(oracle, fx, k, 2)
        for mode in ("steps", "iterate"):
            solvers.append(dict(case=case_file(casedir, c, fx), k=k, solver=2, prec=prec, knobs=knobs, mode=mode))
            cs.append(c)
    res, sections = run_job(cell, tmp_path, nranks, solvers)
    bound = 1e-9 if prec == "F64" else TOL[pcr.PCR_F32]["fac"]
    for i, (sv, c) in enumerate(zip(solvers, cs)):
        k, mode = sv["k"], sv["mode"]
        tag = f"cell {cell}, k = {k}, {mode}"
        assert_form(cell, sections[i], nranks, want, c.d2 * ld_of(k) * ESIZE[prec])
        assert_ranges(cell, res, i, nranks, knobs, c.d2)
        where = owner_text(dict(nranks=nranks, want=want, chunks=int(knobs.get("allreduce_chunks", 0)), esize=ESIZE[prec]))
        keys = ["V", "objs", "counts"] + (["delta", "delta_it"] if mode == "steps" else [])
        for q in range(1, nranks):
            for key in keys:
                a, b = res[0][f"{i}.{key}"], res[q][f"{i}.{key}"]
                z = first_difference(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if b.dtype == np.float64 else b)
                if z is not None:
                    at = where(c, z) if key in ("V", "delta") else f"entry {z}"
                    pytest.fail(f"{tag}: {key} of rank {q} differs from rank 0's; first at {at}: {b.ravel()[z]!r} against {a.ravel()[z]!r}")
        one = one_rank(c, prec, k)
        o_objs, o_counts, o_U, o_V = one[mode]
        U = np.concatenate([res[q][f"{i}.U"] for q in range(nranks)])
        V = res[0][f"{i}.V"]
        assert U.shape == o_U.shape
        eU, eV = np.abs(U - o_U).max() / np.abs(o_U).max(), np.abs(V - o_V).max() / np.abs(o_V).max()
        _WORST[prec] = max(_WORST[prec], eU, eV)
        print(f"[exchange-exact] {tag}: max |dU| / max |U| = {eU:.3e}, max |dV| / max |V| = {eV:.3e} against one rank (bound {bound:g}); "
              f"counts {res[0][f'{i}.counts'].tolist()} against {o_counts.tolist()}; largest {prec} difference so far {_WORST[prec]:.3e}")
        assert eU < bound and eV < bound, (tag, eU, eV, bound)
        if mode == "steps":
            eD = np.abs(res[0][f"{i}.delta"] - one["delta"]).max() / np.abs(one["delta"]).max()
            print(f"[exchange-exact] {tag}: solve_delta direction max |d| / max |.| = {eD:.3e}, {int(res[0][f'{i}.delta_it'])} iterations against {one['delta_it']}")
            assert eD < bound, (tag, eD, bound)                      # the bound of the factors: the direction is what moves V
        if prec == "F64":
            assert np.array_equal(res[0][f"{i}.counts"], o_counts), (tag, res[0][f"{i}.counts"], o_counts)
            if mode == "steps":
                assert int(res[0][f"{i}.delta_it"]) == one["delta_it"], tag
