"""bench.py as the driver starts it.  `python bench.py --gpus N` with N > 1 must start its own ranks (child processes of a
parent that never touches a GPU) and print rank 0's JSON line; the N = 2 path -- per-rank shard generation,
pcr_solver_create_shard, every exchange step, the max-over-ranks clock, the line -- is rehearsed with two ranks on the one
GPU through the peer-to-peer exchange (RCCL refuses two ranks on one device) and compared with ONE rank training the same
2 x 2000 users."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import primalcr_amd as pcr
from primalcr_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def run_bench(*args, timeout=600):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return subprocess.run([sys.executable, BENCH, *args], capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)


def test_initial_rows_are_the_rows_of_initial():
    full = pcr.initial(37, 5)
    assert np.array_equal(pcr.initial_rows(37, 5, 0, 37), full)
    assert np.array_equal(pcr.initial_rows(37, 5, 11, 9), full[11:20])
    assert pcr.initial_rows(37, 5, 37, 0).shape == (0, 5)
    with pytest.raises(pcr.PcrError):
        pcr.initial_rows(37, 5, 30, 8)


def test_user_blocks_of_one_item_catalogue():
    """Rank q's block of the weak-scaling workload: its own users (seed + q), the item ground truth of seed 0's set."""
    a = synth.generate("tiny", seed=5)
    b = synth.generate("tiny", seed=6, item_seed=5)
    c = synth.generate("tiny", seed=6)
    assert np.array_equal(synth.generate("tiny", seed=5, item_seed=5).val, a.val)
    assert np.array_equal(b.item, c.item) and np.array_equal(b.user, c.user)          # the same users and item sets ...
    assert not np.array_equal(b.val, c.val)                                            # ... rated against another catalogue


def test_yahoo_shape_partitions_into_eight_balanced_shards_without_generating_it():
    """configs[4] on 8 GPUs: every rank needs only the per-user counts (1.8 M integers) to find its nnz-balanced user range."""
    ctr, cte = synth.generate_fast("yahoo", counts_only=True)
    assert ctr.shape == (1_800_000,) and int(ctr.sum()) == 700_000_000
    index = np.concatenate([[0], np.cumsum(ctr)])
    b = pcr.partition_users(index, 8)
    nnz = np.diff(index[b])
    assert b[0] == 0 and b[-1] == 1_800_000 and (np.diff(b) > 0).all()
    assert np.abs(nnz / 87_500_000 - 1).max() < 0.002, nnz


@pytest.mark.timeout(300)
def test_gpus_flag_starts_its_own_ranks_and_fails_loudly_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible: the N = 2 run itself is test_two_ranks_on_one_gpu_equal_one_rank")
    p = run_bench("--gpus", "2", "--steps", "1", "--warmup", "0", "--no-cpu")
    assert p.returncode != 0
    assert "starting 2 ranks" in p.stderr and "no GPU visible" in p.stderr and "must be launched with" not in p.stderr
    assert "[rank 0]" in p.stderr and "[rank 1]" in p.stderr and "exited with code 1" in p.stderr      # every rank says why it stops
    last = json.loads(p.stdout.strip().split("\n")[-1])                             # ... and a driver that reads the last line sees it too
    assert last["value"] is None and "error" in last and last["n_gpus"] == 2


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n,fault,want", [(8, "5:9", "rank 5 killed by signal 9 (SIGKILL)"), (6, "0:exit:3", "rank 0 exited with code 3"),
                                          (3, "2:15", "rank 2 killed by signal 15 (SIGTERM)")])
def test_a_rank_that_dies_is_named_and_takes_the_job_down(n, fault, want):
    """Round 4's 6-rank rehearsal ended with an empty stdout and no message (the pool's process guard had killed the whole
    command: 6 ranks + the torch.distributed.run agent = 7 processes on the card).  Whatever ends a rank now -- a signal from
    outside included -- the launcher names the rank and the cause, stops the other ranks (none is left behind) and prints
    {"error": ...} as the last stdout line.  The fault hook ends the rank before it imports torch: no GPU is touched."""
    import time
    t0 = time.time()
    p = run_bench("--gpus", str(n), "--fault", fault, "--steps", "1", "--warmup", "0", "--no-cpu", timeout=120)
    assert p.returncode == 1 and time.time() - t0 < 100
    assert f"starting {n} ranks" in p.stderr and want in p.stderr and "stopping the other ranks" in p.stderr
    last = json.loads(p.stdout.strip().split("\n")[-1])
    assert last["value"] is None and want.split(" (")[0] in last["error"] and last["rank"] == int(fault.split(":")[0]) and last["n_gpus"] == n


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_two_ranks_on_one_gpu_equal_one_rank():
    users, nnz, r, steps, warmup = 2000, 250000, 100, 2, 1
    p = run_bench("--gpus", "2", "--comm", "p2p", "--devices", "0,0", "--rendezvous", "gloo", "--steps", str(steps), "--warmup",
                  str(warmup), "--users", str(users), "--nnz", str(nnz), "--full", "--no-cpu", "--no-f64", "--all-legs",   # (--all-legs: with the row-counting replay)
                  "--netflix-users", "6000", "--netflix-nnz", "600000")
    assert p.returncode == 0, p.stderr[-3000:]
    assert len([l for l in p.stdout.strip().split("\n") if l.startswith("{")]) == 1          # ONE line per run, whatever the legs
    line = json.loads(p.stdout.strip().split("\n")[-1])
    # configs[3] in the N > 1 line: the Netflix-shaped set cut into 2 nnz-balanced user ranges (strong scaling), its own exchange block
    nf = line["netflix"]
    assert "error" not in nf and nf["scaling"] == "strong" and nf["comm_nranks"] == 2 and nf["steps"] == 3 and nf["ms_per_step"] > 0 and nf["value"] > 0
    assert len(nf["shards"]) == 2 and nf["shards"][0][0] == 0 and nf["shards"][1][0] == nf["shards"][0][1] and nf["shards"][0][1] + nf["shards"][1][1] == 6000
    assert sum(sh[2] for sh in nf["shards"]) == 600000 and abs(nf["shards"][0][2] - 300000) < 6000           # balanced by ratings, not by users
    assert nf["exchange"]["vector_bytes"] == 17770 * 100 * 4 and nf["exchange"]["allreduces_per_step"] >= 3 and "x2" in nf["workload"]
    assert line["n_gpus"] == 2 and line["comm_nranks"] == 2 and line["scaling"] == "weak" and line["config"]["exchange"] == "p2p"
    assert line["steps"] == steps and line["warmup"] == warmup
    assert line["shards"] == [[0, users, nnz], [users, users, nnz]]
    # (which slot has the most GPU time is a close call between a U-step class and the rating-parallel kernels when the ranks keep
    # to one stream each; only the gather kernels carry a `binding`)
    assert line["roofline"] and line["roofline"]["kernel"]
    full = json.load(open(os.path.join(ROOT, line["full_record"])))
    gather_slots = {k: v for k, v in full["kernels"].items() if k.partition("/")[0] in ("sddmm", "spmm")}
    assert gather_slots and all(v["binding"]["level"] == "l2-gather" and 0 < v["binding"]["frac"] < 1.5 for v in gather_slots.values())
    if line["roofline"]["kernel"] in gather_slots:
        assert line["roofline"]["binding"]["level"] == "l2-gather"
    assert line["gather"]["level"] == "l2-gather"
    # what the exchange steps cost, for the day a scaling curve has to be decomposed: 1 gradient + 10 Hessian-vector all-reduces of
    # the d2 x ld vector per step, plus the objective's scalar blocks
    ex = line["exchange"]
    assert ex["vector_bytes"] == 3952 * 100 * 4 and ex["vector_allreduces_per_step"] == 1 + line["inner_per_step"]["cg_v"] and ex["allreduces_per_step"] >= ex["vector_allreduces_per_step"] + 2
    assert 0 < ex["allreduce_us_avg"] < 5000 and 0 < ex["share_of_step"] < 1 and ex["us_per_step"] == pytest.approx(ex["allreduce_us_avg"] * ex["allreduces_per_step"], rel=0.02)
    assert len(json.dumps(line, separators=(",", ":"))) < 5120 and line["cpu_baseline"] is None and line["full_record"]
    # the same 2 x 2000 users in ONE solver
    blocks = [synth.generate("ml1m", seed=synth.SEED + q, d1=users, nnz=nnz, item_seed=synth.SEED if q else None) for q in range(2)]
    cat = lambda f: np.concatenate([getattr(blocks[0], f), getattr(blocks[1], f)])
    ds = pcr.Dataset.from_triplets(2 * users, blocks[0].d2, np.concatenate([blocks[0].user, blocks[1].user + users]), cat("item"), cat("val"),
                                   np.concatenate([blocks[0].tuser, blocks[1].tuser + users]), cat("titem"), cat("tval"))
    assert ds.count_pairs() * steps / (line["ms_per_step"] * 1e-3 * steps) == pytest.approx(line["value"], rel=1e-9)
    s = pcr.Solver(ds, pcr.Parameter(k=r, precision=pcr.PCR_F32, do_predict=0, **{"lambda": 5000.0}))
    s.set_factors(pcr.initial(2 * users, r), pcr.initial(blocks[0].d2, r))
    recs = s.iterate(warmup + steps)
    err, ndcg = s.evaluate(1, 10)
    assert recs[-1]["obj"] == pytest.approx(line["objective"], rel=2e-5)             # fp32 storage: summation order differs
    assert ndcg == pytest.approx(line["ndcg10_test"], abs=2e-4) and err == pytest.approx(line["pairwise_error_test"], abs=2e-4)
    assert line["inner_per_step"]["cg_v"] == sum(x["cg_v"] for x in recs[warmup:]) / steps


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_a_layout_rccl_refuses_falls_back_to_the_peer_to_peer_exchange():
    """`--comm rccl` is the default of an N > 1 run, and RCCL has never met a second rank here.  If any rank cannot join its
    communicator -- two ranks on ONE device is a layout ncclCommInitRank refuses with an error code -- the ranks agree through the
    launcher's process group and the whole job takes the direct peer-to-peer exchange: a measurement with `config.exchange` saying
    so instead of an {"error": ...} line."""
    p = run_bench("--gpus", "2", "--comm", "rccl", "--devices", "0,0", "--rendezvous", "gloo", "--steps", "2", "--warmup", "1", "--users", "800",
                  "--nnz", "100000", "--no-cpu", "--no-f64", "--no-rows", "--no-netflix")
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads([l for l in p.stdout.strip().split("\n") if l.startswith("{")][-1])
    assert "error" not in line and line["value"] > 0 and line["n_gpus"] == 2 and line["comm_nranks"] == 2
    assert line["config"]["exchange"].startswith("p2p (fallback") and "peer-to-peer exchange" in p.stderr
    assert line["shards"] == [[0, 800, 100000], [800, 800, 100000]]


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_a_failing_netflix_leg_never_costs_the_headline():
    """the second leg of an N > 1 run is wrapped -- a rank that fails inside it (the hook raises on rank 1, so
    rank 0 is left waiting in the leg's first collective) yields netflix = {"error": ...} in the ONE line, with the ml1m record
    (value, shards, exchange) intact and exit code 0; nobody is left on the GPU."""
    import time
    t0 = time.time()
    p = run_bench("--gpus", "2", "--comm", "p2p", "--devices", "0,0", "--rendezvous", "gloo", "--steps", "2", "--warmup", "1", "--users", "800",
                  "--nnz", "100000", "--full", "--no-cpu", "--no-f64", "--no-rows", "--netflix-users", "3000", "--netflix-nnz", "200000", "--fault-netflix", "1")
    assert p.returncode == 0 and time.time() - t0 < 300, p.stderr[-3000:]
    lines = [l for l in p.stdout.strip().split("\n") if l.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["value"] > 0 and line["n_gpus"] == 2 and line["comm_nranks"] == 2 and line["shards"] == [[0, 800, 100000], [800, 800, 100000]]
    assert "fault hook" in line["netflix"]["error"] and "rank 1" in line["netflix"]["error"]


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_five_ranks_on_one_gpu_through_the_bench_launcher():
    """The widest job this pool lets a test start: its process guard allows 6 processes on the card, this pytest process holds
    one (NOTES.md, round 5: that guard -- 6 ranks + the torch.distributed.run agent = 7 -- is what ended round 4's 6-rank
    rehearsal without a word).  bench.py starts its ranks as direct children now; five of them share the GPU through the
    peer-to-peer exchange with a gloo rendezvous, the line reports 5 ranks, 5 shards, an exchange block, and its objective is the
    one ONE solver reaches on the same 5 x 500 users."""
    n, users, nnz, steps, warmup = 5, 500, 60000, 2, 1
    p = run_bench("--gpus", str(n), "--comm", "p2p", "--devices", ",".join(["0"] * n), "--rendezvous", "gloo", "--steps", str(steps),
                  "--warmup", str(warmup), "--users", str(users), "--nnz", str(nnz), "--full", "--no-cpu", "--no-f64", "--no-rows", "--no-netflix")
    assert p.returncode == 0, p.stderr[-3000:]
    assert f"starting {n} ranks (direct children" in p.stderr
    line = json.loads(p.stdout.strip().split("\n")[-1])
    assert "error" not in line and line["n_gpus"] == n and line["comm_nranks"] == n and line["config"]["exchange"] == "p2p"
    assert line["shards"] == [[q * users, users, nnz] for q in range(n)] and line["exchange"]["allreduces_per_step"] >= 12
    blocks = [synth.generate("ml1m", seed=synth.SEED + q, d1=users, nnz=nnz, item_seed=synth.SEED if q else None) for q in range(n)]
    cat = lambda f: np.concatenate([getattr(b, f) for b in blocks])
    ds = pcr.Dataset.from_triplets(n * users, blocks[0].d2, np.concatenate([b.user + q * users for q, b in enumerate(blocks)]), cat("item"), cat("val"))
    s = pcr.Solver(ds, pcr.Parameter(k=100, precision=pcr.PCR_F32, do_predict=0, **{"lambda": 5000.0}))
    s.set_factors(pcr.initial(n * users, 100), pcr.initial(blocks[0].d2, 100))
    recs = s.iterate(warmup + steps)
    assert recs[-1]["obj"] == pytest.approx(line["objective"], rel=2e-5)


def run_bench_under_torchrun(nproc, *args, timeout=600):
    """The driver's launch for N > 1: python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1
    --master-port P bench.py --gpus N ... (one rank per process; bench.py is one of the ranks and starts nothing itself)."""
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1",
                           "--master-port", str(port), BENCH, "--gpus", str(nproc), *args], capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)


@pytest.mark.timeout(300)
def test_under_the_drivers_launcher_a_job_without_gpus_says_so():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible: test_two_ranks_under_the_drivers_launcher runs the job itself")
    p = run_bench_under_torchrun(2, "--steps", "1", "--warmup", "0", "--no-cpu")
    if "[rank " not in p.stderr:             # (the launcher itself failed -- its rendezvous port taken between our probe and its bind: once more)
        p = run_bench_under_torchrun(2, "--steps", "1", "--warmup", "0", "--no-cpu")
    assert p.returncode != 0
    assert "[rank 0]" in p.stderr and "[rank 1]" in p.stderr and "no GPU visible" in p.stderr and "starting 2 ranks" not in p.stderr, p.stderr[-1500:]
    errs = [json.loads(l) for l in p.stdout.strip().split("\n") if l.startswith("{")]
    assert len(errs) == 1 and errs[0]["value"] is None and "no GPU visible" in errs[0]["error"]        # rank 0's line, nobody else's


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_two_ranks_under_the_drivers_launcher():
    """`python -m torch.distributed.run --nproc-per-node 2 ... bench.py --gpus 2` -- how the driver starts the N > 1 points of the
    scaling curve: bench.py is one of the ranks (RANK / WORLD_SIZE from the launcher), rank 0 prints the one line.  Two ranks on the
    one GPU through the peer-to-peer exchange; the line equals the one bench.py's own launcher gives for the same job."""
    common = ("--comm", "p2p", "--devices", "0,0", "--rendezvous", "gloo", "--steps", "2", "--warmup", "1", "--users", "800", "--nnz", "100000",
              "--full", "--no-cpu", "--no-f64", "--no-rows", "--netflix-users", "3000", "--netflix-nnz", "200000")
    a = run_bench_under_torchrun(2, *common)
    assert a.returncode == 0, a.stderr[-3000:]
    assert "starting 2 ranks" not in a.stderr
    la = json.loads([l for l in a.stdout.strip().split("\n") if l.startswith("{")][-1])
    b = run_bench("--gpus", "2", *common)
    assert b.returncode == 0, b.stderr[-3000:]
    lb = json.loads(b.stdout.strip().split("\n")[-1])
    for line in (la, lb):
        assert "error" not in line and line["n_gpus"] == 2 and line["comm_nranks"] == 2 and line["shards"] == [[0, 800, 100000], [800, 800, 100000]]
        assert "error" not in line["netflix"] and line["netflix"]["comm_nranks"] == 2          # both launchers carry the strong-scaling leg
    assert la["netflix"]["shards"] == lb["netflix"]["shards"] and la["netflix"]["objective"] == lb["netflix"]["objective"]
    assert la["objective"] == lb["objective"] and la["ndcg10_test"] == lb["ndcg10_test"] and la["inner_per_step"] == lb["inner_per_step"]


def _two_devices():
    try:
        import torch
        return torch.cuda.device_count() >= 2
    except Exception:
        return False


@pytest.mark.gpu
@pytest.mark.timeout(900)
@pytest.mark.skipif(not _two_devices(), reason="needs two physical GPUs (the driver's multi-GPU node)")
@pytest.mark.parametrize("comm,chunks", [("rccl", 1), ("rccl", 3), ("p2p", 1), ("p2p", 3)])
def test_two_physical_gpus_equal_one_rank(comm, chunks):
    """RCCL with more than one rank, the peer-to-peer exchange across xGMI and the item-range overlap have only ever run
    where a second GPU exists: when there is one, hold them to the one-rank trajectory."""
    users, nnz, steps, warmup = 2000, 250000, 2, 1
    common = ["--steps", str(steps), "--warmup", str(warmup), "--users", str(users), "--nnz", str(nnz), "--full", "--no-cpu", "--no-f64", "--precision", "f64",
              "--no-profile", "--no-netflix"]
    two = run_bench("--gpus", "2", "--comm", comm, "--tune", f"allreduce_chunks={chunks}", *common)
    assert two.returncode == 0, two.stderr[-3000:]
    a = json.loads(two.stdout.strip().split("\n")[-1])
    assert a["n_gpus"] == 2 and a["comm_nranks"] == 2
    blocks = [synth.generate("ml1m", seed=synth.SEED + q, d1=users, nnz=nnz, item_seed=synth.SEED if q else None) for q in range(2)]
    cat = lambda f: np.concatenate([getattr(blocks[0], f), getattr(blocks[1], f)])
    ds = pcr.Dataset.from_triplets(2 * users, blocks[0].d2, np.concatenate([blocks[0].user, blocks[1].user + users]), cat("item"), cat("val"),
                                   np.concatenate([blocks[0].tuser, blocks[1].tuser + users]), cat("titem"), cat("tval"))
    s = pcr.Solver(ds, pcr.Parameter(k=100, precision=pcr.PCR_F64, do_predict=0, **{"lambda": 5000.0}))
    s.set_factors(pcr.initial(2 * users, 100), pcr.initial(blocks[0].d2, 100))
    recs = s.iterate(warmup + steps)
    assert recs[-1]["obj"] == pytest.approx(a["objective"], rel=1e-10)
    assert s.evaluate(1, 10)[1] == pytest.approx(a["ndcg10_test"], abs=1e-9)


def _canned_full_record():
    """A full bench record as round 3 printed it on ONE stdout line (45 KB: the driver keeps ~8.6 KB and could not parse it)."""
    return json.loads(open(os.path.join(ROOT, "profiles", "r03_d_bench.json")).read().strip().split("\n")[-1])


def test_stdout_line_is_compact_and_carries_what_the_driver_reads():
    """The driver parses the LAST stdout line and keeps only a few KB of stdout: the line must stay small whatever the
    number of kernels, classes and sub-records, and still hold every contract field, `roofline` and `cpu_baseline`."""
    sys.path.insert(0, ROOT)
    import bench
    full = _canned_full_record()
    assert len(json.dumps(full)) > 40000
    # an N = 8 job's extras on top (exchange profile, shards), a cold-start clock, and absurdly many kernels
    full["exchange_profile"] = {"allreduce_us_avg": 31.25, "allreduces_per_step": 14.0, "timed": 18, "vector_bytes": 1580800,
                                "vector_allreduces_per_step": 11.0, "scalar_allreduces_per_step": 3.0, "us_per_step": 437.5, "share_of_step": 0.2261}
    full["shards"] = [[6040 * q, 6040, 939809] for q in range(8)]
    full["cold_start"] = {"iterations": 5, "ms_per_step": 1.71234567}
    full["ms_per_step_first5"] = 1.71234567
    for i in range(200):
        full["kernels"][f"ustep/extra{i}"] = dict(full["kernels"]["sddmm"])
    # round 5: the fp64 leg (the reference's arithmetic type) is first-class, the Netflix leg says what its CPU baseline was timed
    # on, the drop-in CLI's end-to-end wall time is in the line
    full["profile_overhead_pct"] = 5.12345
    full["f64"]["speedup_vs_cpu_baseline"] = 1046.789
    full["netflix"]["speedup_vs_cpu_baseline"] = 2145.4
    full["netflix"]["cpu_baseline"]["sample"] = ("omp-pmf-train -s 2 -k 100 -l 5000 -t 2 -p 0 -n 16 on its first 4800 users (1000003 ratings, "
                                                 "353000111 ordered pairs); 'Iter 2 time' = 7.575 s")
    full["cli"] = {"command": "omp-pmf-train ...", "wall_s": 2.3456789, "load_s": 0.0212345, "init_s": 0.0431, "create_s": 0.61234, "train_s": 0.91,
                   "iter_s": 0.0151234, "eval_s": 0.89, "write_s": 0.35, "process_s": 2.1, "largest_phase": "eval_s", "ndcg10_test": 0.9598123,
                   "reference_wall_s": 61.2345, "speedup_wall": 26.1, "reference": {"ndcg10_test": 0.959811, "wall_s": 61.2345, "cores": 16}}
    line = bench.compact_line(full, "bench_full.json")
    text = json.dumps(line, separators=(",", ":"))
    assert len(text) < bench.LINE_CAP <= 5120, len(text)
    back = json.loads(text)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "cpu_baseline", "full_record"):
        assert k in back, k
    assert back["value"] == full["value"] and back["ms_per_step"] == full["ms_per_step"]          # the headline is not rounded
    assert back["config"]["workload"].startswith("ml1m-shaped")
    rf = back["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert rf["frac"] == pytest.approx(rf["achieved"] / rf["peak"], rel=5e-3)
    assert rf["traffic"] and rf["kernel"].startswith("ustep/") and rf["binding"]["level"] == "l2-gather"
    assert rf["achieved"] == pytest.approx(rf["algorithmic_bytes_per_launch"] / (rf["avg_launch_us"] * 1e-6) / 1e9, rel=2e-3)
    assert rf["traffic_source"] == "stored-pmc:profiles/r03_traffic.json"           # round 3's record replayed stored PMC passes ...
    live = dict(full, roofline=dict(full["roofline"], traffic_source="live: rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE passes started by this run"))
    assert bench.compact_line(live, None)["roofline"]["traffic_source"] == "live-pmc"   # ... this round's run measures them itself
    cb = back["cpu_baseline"]
    assert cb["kind"] == "reference" and cb["cores"] == 16 and cb["value"] > 0 and cb["unit"] == "pairs/s" and cb["sample"]
    assert cb["single_thread"]["s_per_iter"] > cb["s_per_iter"]
    assert back["ms_per_step_first5"] == pytest.approx(1.7123, rel=1e-3)
    assert back["f64"]["ms_per_step"] > back["ms_per_step"] and back["netflix"]["ms_per_step"] > 100
    assert back["netflix"]["cpu_baseline"]["value"] > 0 and back["netflix"]["roofline"]["kernel"].startswith("ustep/")
    assert back["exchange"]["allreduces_per_step"] == 14.0 and len(back["shards"]) == 8
    assert len(back["top_kernels"]) <= 3
    f64 = back["f64"]
    assert f64["roofline"]["achieved"] > 0 and f64["roofline"]["frac"] == pytest.approx(f64["roofline"]["achieved"] / 8000.0, rel=5e-3)
    assert "traffic" in f64["roofline"] and "traffic_over_algorithmic" in f64["roofline"] and f64["roofline"]["binding"]["frac"] > 0
    assert set(f64["roofline_phase"]) == {"u_step", "v_step"} and all(set(v) == {"wall_us", "frac"} for v in f64["roofline_phase"].values())
    assert f64["speedup_vs_cpu_baseline"] == pytest.approx(1046.8, rel=1e-3) and f64["roofline_iteration_frac"] > 0
    assert back["netflix"]["roofline_iteration_frac"] > 0 and back["netflix"]["cpu_baseline"]["sample"] == "first 4800 users (1000003 ratings) of the shape"
    assert back["netflix"]["speedup_vs_cpu_baseline"] == pytest.approx(2145.4, rel=1e-3)
    c = back["cli"]
    assert c["wall_s"] == pytest.approx(2.346, rel=1e-3) and c["reference_wall_s"] == pytest.approx(61.23, rel=1e-3) and c["largest_phase"] == "eval_s"
    assert c["reference_ndcg10_test"] == pytest.approx(0.959811) and c["error"] is None
    assert all(k in c for k in ("load_s", "init_s", "create_s", "train_s", "iter_s", "eval_s", "write_s", "speedup_wall"))
    assert back["profile_overhead_pct"] == pytest.approx(5.12, rel=1e-2)
    # a record that outgrows the cap loses optional blocks, never the contract's fields
    full["config"]["workload"] = "x" * 3000
    small = bench.compact_line(full, "bench_full.json")
    assert len(json.dumps(small, separators=(",", ":"))) < bench.LINE_CAP and len(small["config"]["workload"]) == 240
    cap, bench.LINE_CAP = bench.LINE_CAP, 2600
    try:
        small = bench.compact_line(full, "bench_full.json")
    finally:
        bench.LINE_CAP = cap
    assert len(json.dumps(small, separators=(",", ":"))) < 2600
    assert small["roofline"] and small["cpu_baseline"] and "top_kernels" not in small and "roofline_phase" not in small


def test_live_pmc_pass_is_summed_per_kernel_and_priced_per_launch(tmp_path):
    """roofline.traffic of the default run comes from ONE rocprofv3 --pmc pass the bench starts itself (both 32-byte-unit counters,
    byte-exact per profiles/r06_dram_calib.md): the per-dispatch CSV is summed per kernel symbol and divided by the dispatches; a
    slot is priced 32 B x (reads + writes).  The HBM side comes from the memory controllers' activity beside a sustained replay:
    busy % x 83 GB/s, bytes per iteration, and the part of the fabric-side bytes the Infinity Cache served."""
    import collections
    sys.path.insert(0, ROOT)
    import bench
    name = "void k_ustep<float, 256, false, 1, false, 4, 1>(Shard<float>, Geo, int const*)"
    head = "Correlation_Id,Dispatch_Id,Agent_Id,Queue_Id,Process_Id,Thread_Id,Grid_Size,Kernel_Id,Kernel_Name,Workgroup_Size,LDS_Block_Size,Scratch_Size,VGPR_Count,Accum_VGPR_Count,SGPR_Count,Counter_Name,Counter_Value,Start_Timestamp,End_Timestamp\n"
    rows = lambda ctr, vals, kname=name: "".join(f'{i},{i},1,1,1,1,51200,7,"{kname}",256,0,0,128,0,96,{ctr},{v},0,1\n' for i, v in enumerate(vals, 1))
    (tmp_path / "p.csv").write_text(head + rows(bench.PMC_READ, [300000, 300000, 300000 + 96]) + rows(bench.PMC_WRITE, [320000, 320000, 320000]) +
                                    rows(bench.PMC_READ, [4], "k_nop()") + rows(bench.PMC_WRITE, [0], "k_nop()"))
    acc = collections.defaultdict(lambda: collections.defaultdict(float))
    bench.pmc_accumulate(str(tmp_path / "p.csv"), bench.PMC_READ, acc)
    k = bench.pmc_per_launch(acc)
    assert set(k) == {name, "k_nop()"}
    assert k[name]["launches"] == 3 and k[name]["read_bytes_per_launch"] == pytest.approx(32 * (3 * 300000 + 96) / 3)
    assert k[name]["write_bytes_per_launch"] == 32 * 320000
    assert bench.traffic_bytes(k[name]) == int(k[name]["read_bytes_per_launch"] + k[name]["write_bytes_per_launch"])
    # a stored FETCH_SIZE / WRITE_SIZE pass of earlier rounds keeps its gfx950 doubling
    assert bench.traffic_bytes({"fetch_bytes_per_launch_raw": 100.0, "write_bytes_per_launch": 50.0}) == 250
    assert bench.slot_kernel_match("ustep/256.1024#1", name, "f32") and not bench.slot_kernel_match("ustep/256.512", name, "f32")
    prof = {"ustep/256.1024#1": (2.0, 5), "wall:ustep": (2.5, 5)}
    run = dict(secs=0.03, inner={"cg_v": 200, "ls_v": 20, "cg_u": 290000, "ls_u": 120800}, prof=prof, steps=20, prof_period=16,
               launches={"ustep/256.1024#1": 20, "wall:ustep": 20}, scope={"ustep/256.1024#1": (135301, 200), "wall:ustep": (-1, -1)},
               shard=(0, 6040, 939809), hbm=dict(busy_percent=0.05, samples=200, steps=700, secs=1.05))
    an = bench.analyse(run, None, dict(d1=6040, d2=3952, nnz=939809, r=100), "f32", 1, None, live=k, live_iters=3)
    rf = an["roofline"]
    assert rf["traffic"] == bench.traffic_bytes(k[name]) and rf["traffic_source"].startswith("live")
    assert rf["traffic_over_algorithmic"] == pytest.approx(rf["traffic"] / rf["algorithmic_bytes_per_launch"], abs=0.01)
    h = an["hbm"]
    assert h["achieved_GBs"] == pytest.approx(0.05 * bench.HBM_GBS_PER_BUSY_PERCENT, abs=0.06) and h["frac"] == pytest.approx(0.05 * bench.HBM_GBS_PER_BUSY_PERCENT / 8000, abs=1e-5)
    assert h["bytes_per_iteration"] == pytest.approx(0.05 * 1e9 * bench.HBM_GBS_PER_BUSY_PERCENT * 1.05 / 700, rel=1e-6)
    assert h["fabric_bytes_per_iteration"] == bench.traffic_bytes(k[name])               # 3 launches / 3 iterations; k_nop is no kernel of the step
    assert h["mall_served_frac"] == pytest.approx(1 - h["bytes_per_iteration"] / h["fabric_bytes_per_iteration"], abs=1e-4)
    assert rf["hbm_achieved_GBs"] == h["achieved_GBs"] and rf["mall_served_frac"] == h["mall_served_frac"]
    assert rf["hbm_bytes"] == pytest.approx(0.05 * 1e9 * bench.HBM_GBS_PER_BUSY_PERCENT * rf["avg_launch_us"] * 1e-6, rel=1e-3)
    line = bench.compact_line({"roofline": rf, "hbm": h, "config": {}})
    assert line["roofline"]["hbm_achieved_GBs"] == h["achieved_GBs"] and line["hbm"]["mall_served_frac"] == h["mall_served_frac"]
    # no sampler on the box (or --no-hbm): the fields are null, never zero
    run["hbm"] = None
    an = bench.analyse(run, None, dict(d1=6040, d2=3952, nnz=939809, r=100), "f32", 1, None, live=k, live_iters=3)
    assert an["hbm"] is None and "hbm_achieved_GBs" not in an["roofline"] and bench._roof(an["roofline"])["hbm_achieved_GBs"] is None


def test_uncounted_gather_figures_are_null_not_zero():
    """--no-rows switches the U step's row counter off: every figure derived from it must read null (unmeasured), never 0.0."""
    sys.path.insert(0, ROOT)
    import bench
    prof = {"sddmm": (0.3, 11), "spmm": (0.3, 11), "ustep/256.512": (2.0, 5), "wall:ustep": (2.5, 5)}
    run = dict(secs=0.03, inner={"cg_v": 200, "ls_v": 20, "cg_u": 290000, "ls_u": 120800}, prof=prof, steps=20, prof_period=16,
               launches={"sddmm": 220, "spmm": 220, "ustep/256.512": 20, "wall:ustep": 20},
               scope={"sddmm": (939809, 6040), "spmm": (939809, 6040), "ustep/256.512": (400000, 1500), "wall:ustep": (-1, -1)},
               shard=(0, 6040, 939809))
    wl = dict(d1=6040, d2=3952, nnz=939809, r=100)
    off = bench.analyse(run, None, wl, "f32", 1, None)
    u = off["roofline_phase"]["u_step"]
    assert u["gather_GBs"] is None and u["gathered_row_bytes_per_step"] is None and u["binding"]["frac"] is None and u["binding"]["achieved_GBs"] is None
    assert off["gather"]["frac"] is None and off["gather"]["achieved_GBs"] is None and off["gather"]["u_side_half_passes"] is None
    assert off["gather"]["u_side_counted"] is False and off["gather"]["v_side_half_passes"] == 22.0
    assert off["roofline_phase"]["v_step"]["gather_GBs"] > 0                  # the V side needs no counter
    on = bench.analyse(run, dict(u_rows=20 * 9.1 * 939809, rows_by_class={"ustep/256.512": 25 * 9.5 * 400000},
                                 launches_counted={"ustep/256.512": 25}), wl, "f32", 1, None)
    assert on["roofline_phase"]["u_step"]["gather_GBs"] > 0 and on["gather"]["frac"] > 0 and on["gather"]["u_side_half_passes"] == 9.1
    line = bench.compact_line(dict(_canned_full_record(), gather=off["gather"], roofline_phase=off["roofline_phase"]), None)
    assert line["gather"]["frac"] is None and line["gather"]["u_side_counted"] is False and line["roofline_phase"]["u_step"]["gather_frac"] is None


def test_every_ustep_class_is_one_kernel_symbol_in_the_committed_profiles():
    """bench.py prices a HIP-event slot with the PMC bytes of 'its' kernel symbol (live passes, or profiles/r04_traffic.json): every U-step length
    class of the committed bench line (ml1m and the Netflix-shaped sub-record) must match exactly one k_ustep symbol of the
    rocprofv3 kernel stats of the same shape, and no symbol may serve two classes."""
    import csv
    sys.path.insert(0, ROOT)
    import bench
    line = json.load(open(os.path.join(ROOT, "profiles", "r04_bench_full.json")))
    for shape, rec in (("ml1m", line), ("netflix", line["netflix"])):
        names = [r["Name"] for r in csv.DictReader(open(os.path.join(ROOT, "profiles", f"r04_b_{shape}_f32_kernel_stats.csv")))
                 if r["Name"].startswith("void k_ustep<float")]
        slots = [k for k in rec["kernels"] if k.startswith("ustep/")]
        assert len(slots) >= 6 and len(names) >= len(slots)
        owner = {}
        for sl in slots:
            hit = [n for n in names if bench.slot_kernel_match(sl, n, "f32")]
            assert len(hit) == 1, (shape, sl, hit)
            assert hit[0] not in owner, (shape, sl, owner[hit[0]])
            owner[hit[0]] = sl
        dom = rec["roofline"]["kernel"]
        if dom.startswith("ustep/"):
            assert rec["roofline"]["traffic"] and rec["roofline"]["traffic_over_algorithmic"] > 1, (shape, rec["roofline"])


_SECOND_LEG_DRIVER = r"""
import json, os, sys, time
sys.path.insert(0, {root!r})
import bench
rank, flag, mode = int(sys.argv[1]), sys.argv[2], sys.argv[3]
held = {{"metric": "pairwise-comparisons/sec", "value": 123.0}}
def emit(netflix):
    print(json.dumps(dict(held, netflix=netflix)), flush=True)
leg = bench.SecondLeg(rank, flag, 4.0 if mode == "deadline" else 60.0, emit)
def fn():
    if mode == "raise" and rank == 1:
        raise RuntimeError("boom in the second leg")
    if mode == "ok":
        return {{"ms_per_step": 1.0}}
    time.sleep(120)            # a collective whose peer is gone: never returns by itself
out = leg.run(fn)
if rank == 0:
    emit(out)
"""


@pytest.mark.timeout(120)
@pytest.mark.parametrize("mode", ["raise", "deadline", "sigterm", "ok"])
def test_second_leg_guard_always_lets_the_held_record_out(mode, tmp_path):
    """bench.SecondLeg, the guard round the Netflix-shaped leg of an N > 1 run, without a GPU: two "ranks" as processes.  A rank that
    raises leaves a note and every watchdog ends its process -- rank 0 printing the held record with netflix = {"error": ...} first;
    so does the deadline, and SIGTERM while the main thread sits in a call that never returns; a leg that succeeds prints its result.
    ONE line on rank 0, exit code 0, within seconds."""
    import signal, time
    drv = tmp_path / "drv.py"
    drv.write_text(_SECOND_LEG_DRIVER.format(root=ROOT))
    flag = str(tmp_path / "leg.failed")
    t0 = time.time()
    ps = [subprocess.Popen([sys.executable, str(drv), str(q), flag, mode], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for q in (0, 1)]
    if mode == "sigterm":
        time.sleep(2.5)
        ps[0].send_signal(signal.SIGTERM)
        time.sleep(0.5)
        ps[1].send_signal(signal.SIGTERM)
    outs = [p.communicate(timeout=60) for p in ps]
    assert time.time() - t0 < 40 and [p.returncode for p in ps] == [0, 0], [o[1][-500:] for o in outs]
    lines = [l for l in outs[0][0].strip().split("\n") if l.startswith("{")]
    assert len(lines) == 1 and outs[1][0].strip() == ""                     # rank 0 speaks, once; rank 1 prints nothing
    line = json.loads(lines[0])
    assert line["value"] == 123.0
    if mode == "ok":
        assert line["netflix"] == {"ms_per_step": 1.0}
    else:
        want = {"raise": "rank 1: RuntimeError: boom in the second leg", "deadline": "time budget", "sigterm": "SIGTERM"}[mode]
        assert want in line["netflix"]["error"], line


def test_dumped_outputs_are_whole_or_a_fixed_sample_within_the_cap(tmp_path, monkeypatch):
    """--dump-outputs without a GPU: the factors and the timed steps' objectives as float64 .npy files; factors beyond the cap
    are cut to the same seeded sample of rows on every call, with the row indices beside them, and everything stays within it."""
    sys.path.insert(0, ROOT)
    import bench
    rng = np.random.default_rng(3)
    steps = 4
    run = {"factors": (rng.standard_normal((20000, 20)), rng.standard_normal((5000, 20))), "objs": list(range(10)), "steps": steps}
    small = {"factors": (run["factors"][0][:300], run["factors"][1][:200]), "objs": run["objs"], "steps": steps}
    bench.dump_outputs(str(tmp_path / "small"), small, 0, 1)
    assert sorted(os.listdir(tmp_path / "small")) == ["U.npy", "V.npy", "objective.npy"]
    assert np.array_equal(np.load(tmp_path / "small" / "U.npy"), small["factors"][0])
    assert np.array_equal(np.load(tmp_path / "small" / "V.npy"), small["factors"][1])
    obj = np.load(tmp_path / "small" / "objective.npy")
    assert obj.dtype == np.float64 and obj.tolist() == [6.0, 7.0, 8.0, 9.0]               # the timed steps only
    monkeypatch.setattr(bench, "DUMP_CAP", 3 << 20)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), run, 0, 1)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["U.npy", "U_rows.npy", "V.npy", "V_rows.npy", "objective.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 3 << 20
    for name, full in (("U", run["factors"][0]), ("V", run["factors"][1])):
        rows = np.load(tmp_path / "a" / f"{name}_rows.npy")
        assert rows.dtype == np.float64 and np.all(np.diff(rows) > 0) and 0 < len(rows) < len(full)
        assert np.array_equal(np.load(tmp_path / "a" / f"{name}.npy"), full[rows.astype(np.int64)])
        for f in (name, name + "_rows"):
            assert np.array_equal(np.load(tmp_path / "a" / f"{f}.npy"), np.load(tmp_path / "b" / f"{f}.npy"))
    bench.dump_outputs(str(tmp_path / "r1"), run, 1, 2)                    # N > 1: a rank other than 0 writes its own rows of U
    assert os.listdir(tmp_path / "r1") == ["U_rank1.npy"] or sorted(os.listdir(tmp_path / "r1")) == ["U_rank1.npy", "U_rank1_rows.npy"]


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_plain_run_times_its_steps_and_dumps_what_they_computed(tmp_path):
    """bench.py without --full: the timed steps and the line, no other leg and no full record; --dump-outputs writes the factors
    and objectives the timed steps left -- those of one solver run for warmup + steps iterations from the same start."""
    users, nnz, r, steps, warmup = 2000, 250000, 100, 3, 2
    out = tmp_path / "out"
    p = run_bench("--precision", "f64", "--steps", str(steps), "--warmup", str(warmup), "--users", str(users), "--nnz", str(nnz),
                  "--dump-outputs", str(out))
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.strip().split("\n") if l.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["metric"] == "pairwise-comparisons/sec" and line["unit"] == "pairs/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f64" and line["steps"] == steps and line["warmup"] == warmup and line["ms_per_step"] > 0
    assert not {"roofline", "cpu_baseline", "f64", "netflix", "cli", "full_record", "ndcg10_test", "kernels"} & set(line)
    assert "[traffic]" not in p.stderr and "[cpu_baseline]" not in p.stderr and "[cli]" not in p.stderr
    R = synth.generate("ml1m", seed=synth.SEED, d1=users, nnz=nnz)
    ds = pcr.Dataset.from_ratings(R)
    assert ds.count_pairs() / (line["ms_per_step"] * 1e-3) == pytest.approx(line["value"], rel=1e-9)
    U, V, obj = (np.load(out / f) for f in ("U.npy", "V.npy", "objective.npy"))
    assert U.shape == (users, r) and V.shape == (R.d2, r) and obj.shape == (steps,) and U.dtype == V.dtype == obj.dtype == np.float64
    assert obj[-1] == pytest.approx(line["objective"], rel=1e-8)
    s = pcr.Solver(ds, pcr.Parameter(k=r, precision=pcr.PCR_F64, do_predict=0, **{"lambda": 5000.0}))
    s.set_factors(pcr.initial(users, r), pcr.initial(R.d2, r))
    recs = s.iterate(warmup + steps)
    Us, Vs = s.get_factors()
    s.close()
    assert np.allclose(obj, [x["obj"] for x in recs[warmup:]], rtol=1e-10, atol=0)
    assert np.abs(U - Us).max() <= 1e-8 * np.abs(Us).max() and np.abs(V - Vs).max() <= 1e-8 * np.abs(Vs).max()
