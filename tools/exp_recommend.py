"""Top-K recommendation (pcr_recommend): ms per call, achieved TFLOP/s, the selection's share, and a torch baseline.

For each shape (ml1m 6 040 x 3 706, k = 100; Netflix 480 189 x 17 770, k = 100; a Yahoo!Music share 225 000 x 136 736, k = 200), K = 10
and 100, fp32 and fp64: a solver over a generated training set of 20 ratings per user on average (the exclusion is O(nnz) and
small next to the GEMM at any density), factors from initial(); one warm-up call, then --steps calls timed by the solver's
device events (profile slots recommend/score and recommend/merge).  The selection's share comes from a second solver created
under pcr_tune("recommend_select", "0"): the same kernel with the streaming selection switched off (GEMM and exclusion-free sweep).
Baseline on the same GPU: torch, chunked U_chunk @ V.T + a -inf mask of the chunk's training items + torch.topk, chunks of at most
2 G scores, timed with torch.cuda events after a warm-up (its tie order is torch's, so only its time is compared).
Prints one JSON line per case.

    python tools/exp_recommend.py [--steps 3] [--shapes ml1m,netflix,yahoo] [--no-torch]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import primalcr_amd as pcr  # noqa: E402
from primalcr_amd import synth  # noqa: E402

SHAPES = {"ml1m": (6040, 3706, 100), "netflix": (480189, 17770, 100), "yahoo": (225000, 136736, 200)}
PEAK_F32 = 157.3e12          # f32-input MFMA peak, MI355X
PEAK_F64 = 78.6e12           # f64 MFMA peak, MI355X


def solver_for(ds, d1, d2, k, prec, select):
    with pcr.tuned(recommend_select=select):
        s = pcr.Solver(ds, pcr.Parameter(k=k, precision=prec, do_predict=0, verbose=0))
    s.set_factors(pcr.initial(d1, k), pcr.initial(d2, k))
    return s


def time_solver(s, K, steps):
    s.recommend(K)                                   # warm-up (code object, allocation)
    s.profile(True)
    s.profile_reset()
    for _ in range(steps):
        s.recommend(K)
    sc, n = s.profile_get("recommend/score")
    mg, _ = s.profile_get("recommend/merge")
    s.profile(False)
    return sc / max(n, 1), mg / max(n, 1)


def torch_baseline(index, item, d1, d2, k, K, dtype, steps):
    import torch
    dev = torch.device("cuda:0")
    tdt = torch.float32 if dtype == pcr.PCR_F32 else torch.float64
    U = torch.from_numpy(pcr.initial(d1, k)).to(dev, tdt)
    V = torch.from_numpy(pcr.initial(d2, k)).to(dev, tdt)
    idx = torch.from_numpy(index).to(dev)
    it = torch.from_numpy(item.astype(np.int64)).to(dev)
    rows = torch.repeat_interleave(torch.arange(d1, device=dev), idx[1:] - idx[:-1])
    chunk = max(1, min(d1, (2 << 30) // d2))

    def once():
        for u0 in range(0, d1, chunk):
            u1 = min(d1, u0 + chunk)
            S = U[u0:u1] @ V.T
            z0, z1 = int(index[u0]), int(index[u1])
            S[rows[z0:z1] - u0, it[z0:z1]] = -float("inf")
            torch.topk(S, K, dim=1)

    once()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        once()
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / steps
    del U, V, idx, it, rows
    torch.cuda.empty_cache()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--shapes", default="ml1m,netflix,yahoo")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--torch", default=None, help="shape,K,dtype,steps: the torch baseline alone (ms on stdout)")
    a = ap.parse_args()
    if a.torch:
        name, K, prec, steps = a.torch.split(",")
        d1, d2, k = SHAPES[name]
        R = synth.generate_fast("netflix", d1=d1, d2=d2, nnz=20 * d1)
        print(torch_baseline(np.ascontiguousarray(R.index, np.int64), np.ascontiguousarray(R.item, np.int32), d1, d2, k, int(K), int(prec),
                             int(steps)))
        return
    for name in a.shapes.split(","):
        d1, d2, k = SHAPES[name]
        R = synth.generate_fast("netflix", d1=d1, d2=d2, nnz=20 * d1)
        ds = pcr.Dataset.from_ratings(R)
        index, item = np.ascontiguousarray(R.index, np.int64), np.ascontiguousarray(R.item, np.int32)
        for prec in (pcr.PCR_F32, pcr.PCR_F64):
            fused = solver_for(ds, d1, d2, k, prec, 1)
            bare = solver_for(ds, d1, d2, k, prec, 0)
            for K in (10, 100):
                sc, mg = time_solver(fused, K, a.steps)
                sc0, mg0 = time_solver(bare, K, a.steps)
                flop = 2.0 * d1 * d2 * k
                peak = PEAK_F32 if prec == pcr.PCR_F32 else PEAK_F64
                rec = dict(shape=name, d1=d1, d2=d2, k=k, K=K, dtype="f32" if prec == pcr.PCR_F32 else "f64", nnz=int(index[-1]),
                           score_ms=round(sc, 3), merge_ms=round(mg, 3), total_ms=round(sc + mg, 3),
                           gemm_only_ms=round(sc0, 3), selection_share=round(max(0.0, sc - sc0) / sc, 3) if sc > 0 else None,
                           tflops=round(flop / ((sc + mg) * 1e-3) / 1e12, 2), peak_fraction=round(flop / ((sc + mg) * 1e-3) / peak, 3))
                if not a.no_torch:         # in a fresh process of its own (torch's runtime next to an initialised libprimalcr)
                    out = subprocess.run([sys.executable, __file__, "--torch", f"{name},{K},{prec},{a.steps}"], capture_output=True,
                                         text=True, timeout=600)
                    if out.returncode != 0:
                        raise RuntimeError(out.stderr[-2000:])
                    rec["torch_ms"] = float(out.stdout.strip().splitlines()[-1])
                    rec["speedup_vs_torch"] = round(rec["torch_ms"] / rec["total_ms"], 2)
                print(json.dumps(rec), flush=True)
            fused.close(); bare.close()


if __name__ == "__main__":
    main()
