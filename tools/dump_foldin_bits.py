#!/usr/bin/env python3
"""Dev tool: every output of the eight fold-in entries as raw .npy files, for a byte comparison of two builds.

    python tools/dump_foldin_bits.py --lib A/libprimalcr.so --out dirA       (GPU; once per build)
    python tools/dump_foldin_bits.py --compare dirA dirB                     (anywhere)

Inputs are seeded and NOT dyadic (a changed FMA contraction shows).  Fold-in and item fold-in run on the tests' own length
fixtures (lengths() of tests/test_foldin.py, rater_counts() of tests/test_foldin_items.py: 0, 1 and both form boundaries at
-1 / 0 / +1) at ranks 5 and 16, PrimalCR and PrimalCR++, steps 1 and 5, fp32 and fp64, item fold-in under
itemfold_table_bytes = 4096 as well (several batches); ridge and nnls at rank 8 and above PCR_RIDGE_DIRECT_MAX, lengths on both
sides of PCR_RIDGE_WAVE_MAX and of the rank, weighted and plain, the forced CG form too.  The four solver entries run on a
profiled solver: their slots' names and launch counts go to slots.json."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def compare(a, b):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    if fa != fb:
        sys.exit(f"different file lists: {sorted(set(fa) ^ set(fb))}")
    bad, total = [], 0
    for f in fa:
        x, y = open(os.path.join(a, f), "rb").read(), open(os.path.join(b, f), "rb").read()
        total += len(x)
        if x != y:
            bad.append(f)
    print(f"{len(fa)} files, {total} bytes: " + ("all equal as raw bytes" if not bad else f"{len(bad)} DIFFER: {bad[:20]}"))
    sys.exit(1 if bad else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    a = ap.parse_args()
    if a.compare:
        compare(*a.compare)
    import primalcr_amd as pcr
    if a.lib:
        pcr.use_library(os.path.abspath(a.lib))
    import foldin_ref as fr
    import itemfold_ref as ir
    import ridge_ref as rr
    import test_foldin as tf
    import test_foldin_items as ti
    os.makedirs(a.out, exist_ok=True)
    count = [0]

    def save(name, arrays, stats):
        for i, x in enumerate(arrays):
            np.save(os.path.join(a.out, f"{name}.{i}.npy"), np.ascontiguousarray(x))
        with open(os.path.join(a.out, f"{name}.stats.json"), "w") as f:
            json.dump({k: (v if isinstance(v, int) else float(v).hex()) for k, v in stats.items()}, f, sort_keys=True)
        count[0] += len(arrays)

    PREC = {"f64": pcr.PCR_F64, "f32": pcr.PCR_F32}
    rng = np.random.default_rng(2024)
    lam = 0.7
    # ---- fold-in of users and of items, the _model entries
    for k in (5, 16):
        V = rng.normal(size=(tf.D2, k)) / np.sqrt(k)
        Ui, Vi = rng.normal(size=(ti.D1, k)) / np.sqrt(k), rng.normal(size=(ir.D2, k)) / np.sqrt(k)
        for solver in (2, 1):
            X = tf.users_of(solver)
            U0 = 0.1 * rng.normal(size=(X.d1, k))
            T, items, _ = ti.fixture(solver)
            V0 = 0.1 * rng.normal(size=(len(items), k))
            for steps in (1, 5):
                for pn, dt in PREC.items():
                    for sn, s0 in (("zero", None), ("rand", U0)):
                        U, st, pu = pcr.fold_in(V, fr.csr_args(X), lam, solver_type=solver, U0=s0, steps=steps, dtype=dt, per_user=True)
                        save(f"foldin_k{k}_s{solver}_n{steps}_{pn}_{sn}", (U, pu), st)
                    for tab in (None, 4096):
                        with pcr.tuned(**({} if tab is None else {"itemfold_table_bytes": tab})):
                            R, st, pi = pcr.fold_in_items(Ui, Vi, ti.train_args(T), ir.item_csr(items), lam, solver_type=solver, V0=V0, steps=steps,
                                                          dtype=dt, per_item=True)
                        save(f"itemfold_k{k}_s{solver}_n{steps}_{pn}_t{tab}", (R, pi), st)
    # ---- ridge and nnls, the _model entries
    d2 = 3000
    for k in (8, pcr.PCR_RIDGE_DIRECT_MAX + 4):
        lens = sorted({0, 1, 2, k - 1, k, k + 1, pcr.PCR_RIDGE_WAVE_MAX - 1, pcr.PCR_RIDGE_WAVE_MAX, pcr.PCR_RIDGE_WAVE_MAX + 1, 300, 2049})
        ratings = rr.make_users(d2, lens, 11)
        F = rng.normal(size=(d2, k)) / np.sqrt(k)
        for pn, dt in PREC.items():
            for weighted in (True, False):
                for form in (None, "cg"):
                    with pcr.tuned(**({} if form is None else {"ridge_form": form, "nnls_form": form})):
                        U, st, pu = pcr.fold_in_ridge(F, ratings, 0.05, weighted=weighted, dtype=dt, per_user=True)
                        save(f"ridge_k{k}_{pn}_w{int(weighted)}_{form}", (U, pu), st)
                        U, st, pu = pcr.fold_in_nnls(F, ratings, 0.05, weighted=weighted, dtype=dt, per_user=True)
                        save(f"nnls_k{k}_{pn}_w{int(weighted)}_{form}", (U, pu), st)
    # ---- the solver entries, profiled
    slots = {}
    k = 16
    from primalcr_amd import synth
    T = synth.generate("small", seed=31, d1=ti.D1, d2=400, nnz=ti.D1 * 20)
    ds = pcr.Dataset.from_ratings(T)
    items = [(rng.choice(T.d1, size=c, replace=False), rng.integers(1, 6, size=c).astype(np.float64)) for c in ti.rater_counts()]
    for pn, dt in PREC.items():
        for solver in (2, 1):
            s = pcr.Solver(ds, pcr.Parameter(k=k, precision=dt, solver_type=solver, **{"lambda": lam}))
            s.set_factors(rng.normal(size=(T.d1, k)) / np.sqrt(k), rng.normal(size=(T.d2, k)) / np.sqrt(k))
            s.profile(True)
            X = tf.users_of(solver)
            users = (X.idx, X.item.astype(np.int32) % T.d2, X.val)                # (over the solver's items: duplicates are two ratings)
            U, st, pu = s.fold_in(users, steps=5, per_user=True)
            save(f"solver_foldin_s{solver}_{pn}", (U, pu), st)
            with pcr.tuned(itemfold_table_bytes=4096):
                R, st, pi = s.fold_in_items(ir.item_csr(items), steps=5, per_item=True)
            save(f"solver_itemfold_s{solver}_{pn}", (R, pi), st)
            ratings = rr.make_users(T.d2, [0, 1, 15, 16, 17, 63, 64, 65, 200], 11)
            U, st, pu = s.fold_in_ridge(ratings, per_user=True)
            save(f"solver_ridge_s{solver}_{pn}", (U, pu), st)
            U, st, pu = s.fold_in_nnls(ratings, weighted=False, per_user=True)
            save(f"solver_nnls_s{solver}_{pn}", (U, pu), st)
            slots[f"s{solver}_{pn}"] = {n: s.profile_launches(n) for n in sorted(s.profile_all())}
            s.close()
    with open(os.path.join(a.out, "slots.json"), "w") as f:
        json.dump(slots, f, sort_keys=True, indent=1)
    print(f"{count[0]} arrays written to {a.out}; slots: {slots[next(iter(slots))]}")


if __name__ == "__main__":
    main()
