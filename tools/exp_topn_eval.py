"""Full-catalogue top-N evaluation (pcr_evaluate_topn): device time and wall time against two baselines.

For each shape (ml1m 6 040 x 3 706 and Netflix 480 189 x 17 770, k = 100), K = 10 and 100, fp32 and fp64: a solver over a generated
training set of 20 ratings per user on average with 10 held-out test ratings per user, factors from initial(); one warm-up call of
each entry, then --steps calls of each.
  topn       Solver.evaluate_topn((K,)): device time from the profile slots recommend/score + recommend/metrics, wall time around
             the call (host relevance tables cached after the warm-up, as in a training loop).
  recommend  Solver.recommend(K) (device: recommend/score + recommend/merge) followed by a vectorised numpy evaluation of the
             copied lists on the host (wall time of both).
  torch      chunked U_chunk @ V.T + a -inf mask of the chunk's training items + torch.topk, then membership of the lists in the
             relevant (user, item) keys by torch.isin and the hit / DCG sums on the device; torch.cuda events after a warm-up, in a
             process of its own, run first.
Prints one JSON line per case and appends it to --out.

    python tools/exp_topn_eval.py [--steps 3] [--shapes ml1m,netflix] [--no-torch] [--out profiles/topn_eval_exp.jsonl]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import primalcr_amd as pcr  # noqa: E402
from primalcr_amd import synth  # noqa: E402

SHAPES = {"ml1m": (6040, 3706, 100), "netflix": (480189, 17770, 100)}


def data(name):
    d1, d2, k = SHAPES[name]
    return synth.generate_fast("netflix", d1=d1, d2=d2, nnz=20 * d1, n_test=10), d1, d2, k


def host_eval(items, tindex, titem, tval, d2, K):
    """The numpy baseline: hits, precision, recall, map and ndcg at K (binary gains), every test rating relevant."""
    d1 = items.shape[0]
    users = np.repeat(np.arange(d1, dtype=np.int64), np.diff(tindex))
    keys = np.unique(users * d2 + titem)
    nrel = np.bincount(keys // d2, minlength=d1)
    q = np.arange(d1, dtype=np.int64)[:, None] * d2 + np.where(items >= 0, items, 0)
    pos = np.minimum(np.searchsorted(keys, q), keys.shape[0] - 1)
    rel = (keys[pos] == q) & (items >= 0)
    counted = nrel > 0
    disc = 1.0 / np.log2(np.arange(K) + 2.0)
    hits = rel.sum(1)
    cum = np.cumsum(rel, 1)
    m = np.minimum(K, nrel)
    idcg = np.concatenate([[0.0], np.cumsum(disc)])[m]
    with np.errstate(invalid="ignore", divide="ignore"):
        ap = (rel * cum / np.arange(1, K + 1)).sum(1) / m
        ndcg = (rel * disc).sum(1) / idcg
        recall = hits / nrel
    n = counted.sum()
    return dict(users=int(n), hits=int(hits[counted].sum()), precision=float(hits[counted].sum() / K / n), recall=float(recall[counted].mean()),
                map=float(ap[counted].mean()), ndcg=float(ndcg[counted].mean()))


def torch_baseline(name, K, prec, steps):
    import torch
    R, d1, d2, k = data(name)
    dev = torch.device("cuda:0")
    tdt = torch.float32 if prec == pcr.PCR_F32 else torch.float64
    U = torch.from_numpy(pcr.initial(d1, k)).to(dev, tdt)
    V = torch.from_numpy(pcr.initial(d2, k)).to(dev, tdt)
    index = np.ascontiguousarray(R.index, np.int64)
    it = torch.from_numpy(np.ascontiguousarray(R.item, np.int64)).to(dev)
    rows = torch.repeat_interleave(torch.arange(d1, device=dev), torch.from_numpy(np.diff(index)).to(dev))
    tindex = np.ascontiguousarray(R.tindex, np.int64)
    tusers = torch.repeat_interleave(torch.arange(d1, device=dev), torch.from_numpy(np.diff(tindex)).to(dev))
    keys = torch.unique(tusers * d2 + torch.from_numpy(np.ascontiguousarray(R.titem, np.int64)).to(dev))
    nrel = torch.bincount(keys // d2, minlength=d1).to(tdt)
    disc = 1.0 / torch.log2(torch.arange(K, device=dev, dtype=tdt) + 2.0)
    idcg = torch.cat([torch.zeros(1, device=dev, dtype=tdt), torch.cumsum(disc, 0)])
    chunk = max(1, min(d1, (2 << 30) // d2))

    def once():
        hits = torch.zeros((), device=dev, dtype=tdt)
        ndcg = torch.zeros((), device=dev, dtype=tdt)
        for u0 in range(0, d1, chunk):
            u1 = min(d1, u0 + chunk)
            S = U[u0:u1] @ V.T
            z0, z1 = int(index[u0]), int(index[u1])
            S[rows[z0:z1] - u0, it[z0:z1]] = -float("inf")
            _, top = torch.topk(S, K, dim=1)
            q = torch.arange(u0, u1, device=dev)[:, None] * d2 + top
            rel = torch.isin(q, keys).to(tdt)
            hits += rel.sum()
            m = torch.clamp(nrel[u0:u1], max=K).long()
            ok = m > 0
            ndcg += ((rel * disc).sum(1)[ok] / idcg[m[ok]]).sum()
        return hits, ndcg

    once()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        once()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--shapes", default="ml1m,netflix")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topn_eval_exp.jsonl"))
    ap.add_argument("--torch-only", action="store_true", help="the torch baselines alone: one JSON object {shape,K,dtype: ms} on stdout")
    a = ap.parse_args()
    cases = [(name, K, prec) for name in a.shapes.split(",") for prec in (pcr.PCR_F32, pcr.PCR_F64) for K in (10, 100)]
    if a.torch_only:
        print(json.dumps({f"{n},{K},{p}": torch_baseline(n, K, p, a.steps) for n, K, p in cases}))
        return
    torch_ms = {}
    if not a.no_torch:             # first, in a process of its own (torch's runtime next to an initialised libprimalcr)
        out = subprocess.run([sys.executable, __file__, "--torch-only", "--shapes", a.shapes, "--steps", str(a.steps)], capture_output=True,
                             text=True, timeout=1200)
        if out.returncode != 0:
            raise RuntimeError(out.stderr[-2000:])
        torch_ms = json.loads(out.stdout.strip().splitlines()[-1])
    for name in a.shapes.split(","):
        R, d1, d2, k = data(name)
        ds = pcr.Dataset.from_ratings(R)
        tindex, titem, tval = ds.csr(1)
        for prec in (pcr.PCR_F32, pcr.PCR_F64):
            s = pcr.Solver(ds, pcr.Parameter(k=k, precision=prec, do_predict=0, verbose=0))
            s.set_factors(pcr.initial(d1, k), pcr.initial(d2, k))
            for K in (10, 100):
                s.evaluate_topn((K,)); s.recommend(K)                          # warm-up (code objects, relevance tables)
                s.profile(True)
                s.profile_reset()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    st = s.evaluate_topn((K,))
                topn_wall = (time.perf_counter() - t0) / a.steps * 1e3
                sc, _ = s.profile_get("recommend/score")
                mt, _ = s.profile_get("recommend/metrics")
                s.profile_reset()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    items, _ = s.recommend(K)
                    host = host_eval(items, tindex, titem, tval, d2, K)
                rec_wall = (time.perf_counter() - t0) / a.steps * 1e3
                rsc, _ = s.profile_get("recommend/score")
                rmg, _ = s.profile_get("recommend/merge")
                s.profile(False)
                topn_dev = (sc + mt) / a.steps                                 # (per call: a call may launch several batches)
                rec_dev = (rsc + rmg) / a.steps
                rec = dict(shape=name, d1=d1, d2=d2, k=k, K=K, dtype="f32" if prec == pcr.PCR_F32 else "f64", users=st[0]["users"],
                           topn_score_ms=round(sc / a.steps, 3), topn_metrics_ms=round(mt / a.steps, 3), topn_device_ms=round(topn_dev, 3),
                           recommend_device_ms=round(rec_dev, 3), device_ratio=round(topn_dev / rec_dev, 3),
                           topn_wall_ms=round(topn_wall, 2), recommend_plus_numpy_wall_ms=round(rec_wall, 2),
                           wall_speedup=round(rec_wall / topn_wall, 2),
                           ndcg=st[0]["ndcg"], numpy_ndcg=host["ndcg"], map=st[0]["map"], numpy_map=host["map"],
                           hits=st[0]["hits"], numpy_hits=host["hits"])
                if torch_ms:
                    rec["torch_ms"] = round(torch_ms[f"{name},{K},{prec}"], 3)
                    rec["speedup_vs_torch"] = round(rec["torch_ms"] / topn_dev, 2)
                print(json.dumps(rec), flush=True)
                with open(a.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")
            s.close()


if __name__ == "__main__":
    main()
