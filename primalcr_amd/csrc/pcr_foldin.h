// pcr_foldin.h -- k_foldin: fold-in of users the model was not trained on (pcr_fold_in, pcr_fold_in_model of
// include/primalcr.h).  One workgroup runs a user's WHOLE optimisation over u with V fixed -- up to `steps` Newton steps, each
// the gradient, a truncated CG and a line search of update_u_new (pcrpp.cpp:779-815) / update_u (pcr.cpp:523-585) -- in one
// launch.  Part of pcr_fold.hip; the building blocks are those of k_ustep (pcr_prims.h) in its uncached form.
//
// What differs from k_ustep:
//   - nothing is handed over: no Shard<T>, no window cache, no sorted state from a k_prepare, no clusters.  The user's ratings
//     stay in CSR order (item-ascending) for the whole optimisation: the rows of V are gathered in that order by every pass,
//     from L2.  (Staging them in LDS once per user, which that fixed order allows, was built and measured: 2.2 x slower on
//     20-rating users, 1.6 x on 200-rating users -- the image's LDS costs more occupancy than its reads save; NOTES.md
//     "Fold-in".)  The (level, m)-sorted state of a point is the pair (ms, li): sorted scores and the packed (level, CSR
//     position); per-rating values that meet the rows (the SDDMM's b, the sweeps' c) live in CSR order and are read / written
//     through li.
//   - the sorted state and the loss of an ACCEPTED line-search try are the next step's state at u (same scores: the try was
//     evaluated at the point rounded to T), so a step costs no pass of its own for them.  Every sort starts from CSR order, so
//     the state is bit for bit what a fresh evaluation at that u gives.
//   - a failed line search leaves u where it was (status STALLED), where the training loop moves on (quirk q5).
// Results depend on the user's ratings, V and the parameters alone: a user's workgroup form is a function of its length, every
// sum has a fixed order, nothing is exchanged between workgroups and every loop has a static bound (steps, cg_max, 20).
#pragma once
#include <type_traits>

#include "pcr_host.h"
#include "pcr_prims.h"

// The workgroup forms by user length (PCR_FOLDIN_WAVE_MAX, PCR_FOLDIN_LDS_MAX) are part of the contract: include/primalcr.h.

// the new users' ratings on the device: CSR (item-ascending rows), dense level per rating, per user T_u + 1 cumulative level counts
struct FoldinCsr {
    const int64_t* uptr;
    const int32_t* item;
    const uint16_t* lvl;
    const int64_t* runofs;
    const int32_t* runstart;
};

// The LDS vectors of one row's optimisation, k_foldin's and k_itemfold's (pcr_itemfold.h) alike: vecT, red, the seven fp64 vectors
// of ld values and the gather's per-wave partial rows
static inline size_t fold_small_bytes(int ld, int block, size_t elt) {
    return carve_bytes(ld, elt) + carve_bytes(block / PCR_WAVE + 1, 8) + 7 * carve_bytes(ld, 8) + carve_bytes((size_t)(block / PCR_WAVE) * ld, 8);
}
// the per-rating arrays of a user of at most cap ratings and rs_cap - 1 levels (LDS, or one workgroup's slice of the scratch)
static inline size_t foldin_arr_bytes(int cap, int rs_cap, size_t elt, size_t li_bytes) {
    return 2 * carve_bytes(cap, elt) + 2 * carve_bytes(cap, li_bytes) + carve_bytes(cap, 4) + carve_bytes(cap, 2) + carve_bytes((size_t)cap + 1, 8) +
           carve_bytes(rs_cap, 4);
}

template <typename T, int BLOCK, bool BIG>
__global__ __launch_bounds__(BLOCK) void k_foldin(FoldinCsr X, Geo geo, const int32_t* __restrict__ users, int nusers, const T* __restrict__ U0,
                                                  T* __restrict__ Uout, const T* __restrict__ Vm, double* __restrict__ per_user, double lambda,
                                                  double stepsize0, int cg_max, double cg_tol, int steps, int strict, int solver1, int cap, int rs_cap,
                                                  char* scratch, size_t stride) {
    typedef typename std::conditional<BIG, uint64_t, uint32_t>::type LI;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    Carver small(smem);
    T* vecT = small.take<T>(geo.ld);
    double* red = small.take<double>(BLOCK / PCR_WAVE + 1);
    double* uvec = small.take<double>(geo.ld);
    double* gvec = small.take<double>(geo.ld);
    double* delta = small.take<double>(geo.ld);
    double* rr = small.take<double>(geo.ld);
    double* pv = small.take<double>(geo.ld);
    double* Hp = small.take<double>(geo.ld);
    double* unew = small.take<double>(geo.ld);
    double* wbuf = small.take<double>((size_t)(BLOCK / PCR_WAVE) * geo.ld);
    Carver big(BIG ? scratch + (size_t)blockIdx.x * stride : small.p);
    T* ms0 = big.take<T>(cap);              // the sorted state at u: scores ...
    T* key = big.take<T>(cap);              // ... and the working copy: b / c of the sweeps in CSR order, then a tried point's sorted scores
    LI* li0 = big.take<LI>(cap);            // (level, CSR position) at each sorted position of ms0
    LI* li = big.take<LI>(cap);
    int32_t* itm = big.take<int32_t>(cap);  // CSR order
    uint16_t* lvc = big.take<uint16_t>(cap);
    double* Sx = big.take<double>((size_t)cap + 1);
    int* rs = big.take<int>(rs_cap);
    const int tid = threadIdx.x;
    const int ld = geo.ld;

    for (int ui = blockIdx.x; ui < nusers; ui += gridDim.x) {
        const int u = users[ui];
        const int64_t s0 = X.uptr[u];
        const int n = (int)(X.uptr[u + 1] - s0);
        const int nlev = (int)(X.runofs[u + 1] - X.runofs[u]) - 1;
        for (int t = tid; t < ld; t += BLOCK) uvec[t] = (double)U0[(size_t)u * ld + t];
#pragma unroll 4
        for (int p = tid; p < n; p += BLOCK) { itm[p] = X.item[s0 + p]; lvc[p] = X.lvl[s0 + p]; }
        for (int l = tid; l <= nlev; l += BLOCK) rs[l] = X.runstart[X.runofs[u] + l];
        __syncthreads();
        // out[p] = vecT . V[item p], CSR order
        auto sddmm = [&](T* out) { block_sddmm<T, BLOCK, false>(Vm, vecT, itm, n, out, geo, 0); };
        // vec += sum_p c[p] V[item p], CSR order
        auto gather_axpy = [&](const T* c, double* vec) { block_gather_axpy<T, T, BLOCK, false>(Vm, itm, c, n, vec, wbuf, geo, 0, false); };
        const int npad = next_pow2(n);
        // the sorted state of the point in vecT into (key, li); returns its loss (compute_mm_old :728-744, update_infor_ui
        // :684-726, objective_u_new :542-573)
        auto eval_point = [&]() -> double {
            sddmm(key);
            for (int p = tid; p < n; p += BLOCK) li[p] = LiOps<LI>::pack(lvc[p], (unsigned)p);
            __syncthreads();
            bitonic_sort<T, LI, BLOCK, false, !BIG>(key, li, npad, n);
            __syncthreads();
            return block_objective<T, BLOCK>(key, [&](int p) { return (int)LiOps<LI>::lev(li[p]); }, rs, nlev, n, Sx, red, strict);
        };

        int n_steps = 0, n_cg = 0, n_ls = 0, status = 1;          // STEP_CAP unless a step ends the user
        double loss0 = 0.0, gn2 = 0.0, un2 = 0.0;
        if (n > 0) {
            for (int t = tid; t < ld; t += BLOCK) vecT[t] = (T)uvec[t];
            __syncthreads();
            loss0 = eval_point();
            { T* a = ms0; ms0 = key; key = a; LI* b = li0; li0 = li; li = b; }
        }
        for (int step = 0; step < steps; ++step) {
            // ---- gradient, obtain_g_u_new (pcrpp.cpp:493-539)
            if (n > 0) {
                block_excl_scan<BLOCK>([&](int i) { return (double)ms0[i]; }, Sx, n, red);
                for (int p = tid; p < n; p += BLOCK) {
                    const LI x = li0[p];
                    key[LiOps<LI>::idx(x)] = (T)sweep_coeff<T>(ms0, Sx, rs, nlev, (int)LiOps<LI>::lev(x), ms0[p], (double)ms0[p], 1.0, strict);
                }
            }
            for (int t = tid; t < ld; t += BLOCK) gvec[t] = (n == 0) ? 0.0 : uvec[t] * lambda;
            __syncthreads();
            if (n > 0) gather_axpy(key, gvec);
            double a = 0.0, b = 0.0;
            for (int t = tid; t < ld; t += BLOCK) { a += uvec[t] * uvec[t]; b += gvec[t] * gvec[t]; }
            un2 = block_sum<BLOCK>(a, red);
            gn2 = block_sum<BLOCK>(b, red);
            const double prev_obj = lambda / 2.0 * un2 + loss0;
            // pcrpp.cpp:787-790; PrimalCR additionally keeps u when no comparable pair exists (cc == 0, pcr.cpp:552)
            if (n == 0 || gn2 < 0.0001 || (solver1 && nlev <= 1)) { status = 0; break; }
            // ---- CG, solve_delta_u_new (pcrpp.cpp:628-647)
            for (int t = tid; t < ld; t += BLOCK) { delta[t] = 0.0; rr[t] = gvec[t] * -1.0; pv[t] = gvec[t]; }
            const double err = sqrt(gn2) * cg_tol;
            __syncthreads();
            for (int k = 1; k <= cg_max; ++k) {
                for (int t = tid; t < ld; t += BLOCK) { vecT[t] = (T)pv[t]; Hp[t] = pv[t] * lambda; }
                __syncthreads();
                sddmm(key);                                                     // b = V_I p  (:592-594)
                __syncthreads();
                block_excl_scan<BLOCK>([&](int i) { return (double)key[LiOps<LI>::idx(li0[i])]; }, Sx, n, red);
                for (int p = tid; p < n; p += BLOCK) {
                    const LI x = li0[p];
                    const int q = (int)LiOps<LI>::idx(x);
                    key[q] = (T)sweep_coeff<T>(ms0, Sx, rs, nlev, (int)LiOps<LI>::lev(x), ms0[p], (double)key[q], 0.0, strict);
                }
                __syncthreads();
                gather_axpy(key, Hp);
                ++n_cg;
                a = 0.0; b = 0.0;
                for (int t = tid; t < ld; t += BLOCK) { a += pv[t] * Hp[t]; b += rr[t] * pv[t]; }
                const double pHp = block_sum<BLOCK>(a, red);
                const double rp = block_sum<BLOCK>(b, red);
                const double alpha = -1.0 * rp / pHp;
                a = 0.0; b = 0.0;
                for (int t = tid; t < ld; t += BLOCK) {
                    delta[t] = delta[t] + pv[t] * alpha;
                    const double rn = rr[t] + Hp[t] * alpha;
                    rr[t] = rn;
                    a += rn * rn;
                    b += rn * Hp[t];
                }
                const double rr2 = block_sum<BLOCK>(a, red);
                const double rHp = block_sum<BLOCK>(b, red);
                if (sqrt(rr2) < err) break;
                const double beta = rHp / pHp;
                for (int t = tid; t < ld; t += BLOCK) pv[t] = rr[t] * -1.0 + pv[t] * beta;
                __syncthreads();
            }
            __syncthreads();
            // ---- line search (pcrpp.cpp:794-813): fresh scores, fresh sort, objective
            double step_len = stepsize0, loss_new = 0.0;
            bool accepted = false;
            for (int it = 0; it < 20; ++it) {
                double nn = 0.0;
                for (int t = tid; t < ld; t += BLOCK) {
                    const double v = uvec[t] + delta[t] * -step_len;
                    unew[t] = v;
                    vecT[t] = (T)v;
                    nn += (double)(T)v * (double)(T)v;
                }
                nn = block_sum<BLOCK>(nn, red);
                __syncthreads();
                loss_new = eval_point();
                ++n_ls;
                if (lambda / 2.0 * nn + loss_new < prev_obj) { accepted = true; break; }
                step_len /= 2.0;
            }
            if (!accepted) { status = 2; break; }                  // STALLED: u stays where this step found it
            // the accepted point, as the storage type holds it, and its sorted state
            for (int t = tid; t < ld; t += BLOCK) uvec[t] = (double)(T)unew[t];
            loss0 = loss_new;
            { T* c = ms0; ms0 = key; key = c; LI* d = li0; li0 = li; li = d; }
            ++n_steps;
            __syncthreads();
        }
        if (status == 1) {                                         // the step cap: un2 belongs to the point before the last step
            double a = 0.0;
            for (int t = tid; t < ld; t += BLOCK) a += uvec[t] * uvec[t];
            un2 = block_sum<BLOCK>(a, red);
        }
        for (int t = tid; t < ld; t += BLOCK) Uout[(size_t)u * ld + t] = (T)uvec[t];
        if (tid == 0) {
            double* o = per_user + (size_t)u * 6;
            o[0] = (double)n_steps; o[1] = (double)n_cg; o[2] = (double)n_ls;
            o[3] = lambda / 2.0 * un2 + loss0; o[4] = gn2; o[5] = (double)status;
        }
        __syncthreads();
    }
}
