// pcr_itemfold.h -- k_rater_scores, k_itemfold: fold-in of ITEMS the model was not trained on (pcr_fold_in_items,
// pcr_fold_in_items_model of include/primalcr.h).  U and the trained rows of V are fixed; new item j with raters R_j (user i gave
// it r_ij) gets the row v that minimises
//     F_j(v) = lambda/2 |v|^2 + sum_{i in R_j} phi_ij(u_i . v),
//     phi_ij(s) = sum_{k in Omega_i, lev(r_ik) < lev(r_ij)} max(0, 1 - s + m_ik)^2 + sum_{k, lev(r_ik) > lev(r_ij)} max(0, 1 + s - m_ik)^2,
// Omega_i the rater's TRAINING row and m_ik = u_i . v_k as the storage type holds it: F_j is the change of the training objective
// when item j and its ratings are appended to the data.  New items are folded in independently of each other: a pair of two new
// items rated by the same user is NOT modelled.  Part of pcr_fold.hip; the building blocks are those of k_foldin (pcr_prims.h).
//
// The user-side kernel cannot be reused with the roles swapped: the loss compares items WITHIN a user, so the new row couples to
// the whole training row of every rater.  Two kernels:
//   k_rater_scores   the rater table: for each UNIQUE rater of the batch, m = V_I u_i over its training row, rounded to T, in CSR
//                    order in one flat array (the gather-heavy phase: one row of V per training rating).  A rater shared by several
//                    new items is computed once.  The rating's level is the dense rank training uses (pcr_build_levels, uint16).
//   k_itemfold       one workgroup runs an item's WHOLE optimisation in one launch, pcr_fold_in's rules 1-6 with the roles
//                    swapped.  The state at v is s = U_R v in the storage type, then ONE scan of each rater's table segment: a
//                    group of 16 lanes per rater compares 2 * level with the pair's doubled rank (2 * rank of r_ij's level in
//                    the rater's row, the odd value between its neighbours when the row does not hold it) and sums phi, c = phi' and the number
//                    of active pairs (h = 2 * that).  h stays frozen at the gradient point, so a CG iteration is one SDDMM and
//                    one gather-axpy over the rater rows of U and needs no scan.  An accepted line-search try's (loss, c, h) is
//                    the next step's state: the try was evaluated at the point rounded to T, so it is bit for bit what a fresh
//                    evaluation at that v gives.
// Results depend on the item's ratings, its raters' training rows, U, V and the parameters alone: an item's workgroup form is a
// function of its rater count, a rater's of its length; every sum has a fixed order, no atomics, nothing is exchanged between
// workgroups and every loop has a static bound (steps, cg_max, 20).
#pragma once
#include <type_traits>

#include "pcr_host.h"
#include "pcr_foldin.h"      // fold_small_bytes: the small carve is k_foldin's
#include "pcr_prims.h"

// The workgroup forms (PCR_ITEMFOLD_WAVE_MAX, PCR_ITEMFOLD_LDS_MAX, PCR_ITEMFOLD_SCORES_WAVE_MAX) are part of the contract:
// include/primalcr.h.
#define ITEMFOLD_SCAN_UNR 8
#define ITEMFOLD_SCAN_LANES 16

// the batch's unique raters on the device: their training rows (CSR order) and the dense level of every rating
struct RaterTab {
    const int64_t* rptr;      // [raters + 1] offsets into ritem / rlvl / the score table
    const int32_t* ruser;     // [raters] the rater's row of U
    const int32_t* ritem;
    const uint16_t* rlvl;
};
// the new items in launch order (slots, by descending rater count): the (item, rater) pairs of slot t are [sptr[t], sptr[t + 1])
struct ItemfoldCsr {
    const int64_t* sptr;
    const int32_t* orig;      // [slots] the caller's item id: the row of V0 / V_out / per_item
    const int32_t* anypair;   // [slots] some rater's row holds a level different from the new rating's
    const int32_t* puser;     // per pair: the rater's row of U ...
    const int32_t* pq;        // ... and the doubled rank of the new rating among the rater's levels
    const int32_t* ploc;      // per pair of THIS batch (pair - pair0): the rater's position in the batch's RaterTab
    int64_t pair0;
};

// the per-rater arrays of an item of at most cap raters (LDS, or one workgroup's slice of the scratch)
static inline size_t itemfold_arr_bytes(int cap, size_t elt) { return 3 * carve_bytes(cap, elt) + 2 * carve_bytes(cap, 4); }

// tab[rptr[r] + p] = U[ruser[r]] . V[ritem[rptr[r] + p]], one workgroup per rater, longest first
template <typename T, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_rater_scores(RaterTab R, Geo geo, const int32_t* __restrict__ order, int nraters, const T* __restrict__ Um,
                                                        const T* __restrict__ Vm, T* __restrict__ tab) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* vecT = reinterpret_cast<T*>(smem);
    for (int ri = blockIdx.x; ri < nraters; ri += gridDim.x) {
        const int r = order[ri];
        const int64_t a = R.rptr[r];
        const int n = (int)(R.rptr[r + 1] - a);
        __syncthreads();
        for (int t = threadIdx.x; t < geo.ld; t += BLOCK) vecT[t] = Um[row_off(R.ruser[r], geo) + t];
        __syncthreads();
        block_sddmm<T, BLOCK, false>(Vm, vecT, R.ritem + a, n, tab + a, geo, 0);
    }
}

// the sum over the ITEMFOLD_SCAN_LANES (16) lanes of a lane group, to every lane of the group
__device__ __forceinline__ double group_sum16(double v) {
    v += lane_xor<8>(v); v += lane_xor<4>(v);
    v += lane_xor2(v);
    v += lane_xor1(v);
    return v;
}

// One scan of the table segments of the item's raters at the scores sb: per rater i, phi_i (summed into the result), c[i] =
// phi_i'(sb[i]) rounded to T and cnt[i] = its active pairs.  A group of 16 lanes per rater, its lanes strided over the segment with
// ITEMFOLD_SCAN_UNR ratings each in flight: the scan waits on the chain rater -> segment -> ratings, so a wave keeps four raters'
// chains going (a wave per rater: itemfold/newton 8 - 10 % slower on the two measured workloads, NOTES.md "Item fold-in").  A lane adds its
// ratings in ascending order, the group's lanes by the butterfly, a group its raters in order, then the groups and the waves.
// strict: PrimalCR's windows (a pair at the boundary is not active).
template <typename T, int BLOCK>
__device__ __forceinline__ double itemfold_scan(const RaterTab& R, const T* __restrict__ tab, const int32_t* __restrict__ ploc,
                                                const int32_t* __restrict__ pq, int n, const T* sb, T* c, uint32_t* cnt, double* red, int strict) {
    constexpr int GL = ITEMFOLD_SCAN_LANES, NGR = BLOCK / GL;
    const int gl = threadIdx.x & (GL - 1), gid = threadIdx.x / GL;
    double tot = 0.0;
    for (int i0 = 0; i0 < n; i0 += NGR) {                            // (the same trip count for every lane: the sums below are wave-wide code)
        const int i = i0 + gid;
        int64_t a = 0;
        int len = 0, q = 0;
        double s = 0.0;
        if (i < n) {
            const int loc = ploc[i];
            a = R.rptr[loc];
            len = (int)(R.rptr[loc + 1] - a);
            q = pq[i];
            s = (double)sb[i];
        }
        double phi = 0.0, ci = 0.0, act = 0.0;
        for (int z0 = gl; z0 < len; z0 += ITEMFOLD_SCAN_UNR * GL) {
            int lv[ITEMFOLD_SCAN_UNR];
            T mv[ITEMFOLD_SCAN_UNR];
#pragma unroll
            for (int u = 0; u < ITEMFOLD_SCAN_UNR; ++u) {
                const int z = z0 + u * GL;
                lv[u] = q;                                                   // past the end: a tie, no pair
                mv[u] = (T)0;
                if (z < len) { lv[u] = 2 * (int)R.rlvl[a + z]; mv[u] = tab[a + z]; }
            }
#pragma unroll
            for (int u = 0; u < ITEMFOLD_SCAN_UNR; ++u) {
                if (lv[u] == q) continue;
                const double m = (double)mv[u];
                const bool below = lv[u] < q;                                // the new item is to score above this one
                const double d = below ? 1.0 - s + m : 1.0 + s - m;
                if (strict ? d > 0.0 : d >= 0.0) { phi += d * d; ci += below ? d * -2.0 : d * 2.0; act += 1.0; }
            }
        }
        phi = group_sum16(phi); ci = group_sum16(ci); act = group_sum16(act);
        if (i < n && gl == 0) { c[i] = (T)ci; cnt[i] = (uint32_t)act; }
        tot += phi;
    }
    return block_sum<BLOCK>(gl == 0 ? tot : 0.0, red);
}

template <typename T, int BLOCK, bool BIG>
__global__ __launch_bounds__(BLOCK) void k_itemfold(RaterTab R, ItemfoldCsr X, Geo geo, int slot0, int nslots, const T* __restrict__ V0,
                                                    T* __restrict__ Vout, const T* __restrict__ Um, const T* __restrict__ tab,
                                                    double* __restrict__ per_item, double lambda, double stepsize0, int cg_max, double cg_tol,
                                                    int steps, int solver1, int cap, char* scratch, size_t stride) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    Carver small(smem);
    T* vecT = small.take<T>(geo.ld);
    double* red = small.take<double>(BLOCK / PCR_WAVE + 1);
    double* vvec = small.take<double>(geo.ld);
    double* gvec = small.take<double>(geo.ld);
    double* delta = small.take<double>(geo.ld);
    double* rr = small.take<double>(geo.ld);
    double* pv = small.take<double>(geo.ld);
    double* Hp = small.take<double>(geo.ld);
    double* vnew = small.take<double>(geo.ld);
    double* wbuf = small.take<double>((size_t)(BLOCK / PCR_WAVE) * geo.ld);
    Carver big(BIG ? scratch + (size_t)blockIdx.x * stride : small.p);
    T* sb = big.take<T>(cap);                   // scores of the point in vecT, then the CG's coefficients
    T* c0 = big.take<T>(cap);                   // the state at v: c = phi' per rater ...
    T* c1 = big.take<T>(cap);
    uint32_t* n0 = big.take<uint32_t>(cap);     // ... and the active pairs per rater
    uint32_t* n1 = big.take<uint32_t>(cap);
    const int tid = threadIdx.x;
    const int ld = geo.ld;
    const int strict = solver1;

    for (int si = slot0 + blockIdx.x; si < slot0 + nslots; si += gridDim.x) {
        const int j = X.orig[si];
        const int64_t p0 = X.sptr[si];
        const int n = (int)(X.sptr[si + 1] - p0);
        const int32_t* rows = X.puser + p0;
        const int32_t* ploc = X.ploc + (p0 - X.pair0);
        const int32_t* pq = X.pq + p0;
        for (int t = tid; t < ld; t += BLOCK) vvec[t] = (double)V0[(size_t)j * ld + t];
        __syncthreads();
        // out[i] = vecT . U[rater i]
        auto sddmm = [&](T* out) { block_sddmm<T, BLOCK, false>(Um, vecT, rows, n, out, geo, 0); };
        // vec += sum_i c[i] U[rater i]
        auto gather_axpy = [&](const T* c, double* vec) { block_gather_axpy<T, T, BLOCK, false>(Um, rows, c, n, vec, wbuf, geo, 0, false); };
        // the state (c, cnt) of the point in vecT; returns its loss
        auto eval_point = [&](T* c, uint32_t* cnt) -> double {
            sddmm(sb);
            __syncthreads();
            const double loss = itemfold_scan<T, BLOCK>(R, tab, ploc, pq, n, sb, c, cnt, red, strict);
            __syncthreads();
            return loss;
        };

        int n_steps = 0, n_cg = 0, n_ls = 0, status = 1;          // STEP_CAP unless a step ends the item
        double loss0 = 0.0, gn2 = 0.0, vn2 = 0.0, obj_start = 0.0;
        if (n > 0) {
            for (int t = tid; t < ld; t += BLOCK) vecT[t] = (T)vvec[t];
            __syncthreads();
            loss0 = eval_point(c0, n0);
        }
        for (int step = 0; step < steps; ++step) {
            // ---- gradient: lambda v + U_R^T c
            for (int t = tid; t < ld; t += BLOCK) gvec[t] = (n == 0) ? 0.0 : vvec[t] * lambda;
            __syncthreads();
            if (n > 0) gather_axpy(c0, gvec);
            double a = 0.0, b = 0.0;
            for (int t = tid; t < ld; t += BLOCK) { a += vvec[t] * vvec[t]; b += gvec[t] * gvec[t]; }
            vn2 = block_sum<BLOCK>(a, red);
            gn2 = block_sum<BLOCK>(b, red);
            const double prev_obj = lambda / 2.0 * vn2 + loss0;
            if (step == 0) obj_start = prev_obj;
            if (n == 0 || gn2 < 0.0001 || (solver1 && !X.anypair[si])) { status = 0; break; }
            // ---- CG on (lambda I + U_R^T diag(h) U_R) delta = g, h = 2 n0 frozen at v
            for (int t = tid; t < ld; t += BLOCK) { delta[t] = 0.0; rr[t] = gvec[t] * -1.0; pv[t] = gvec[t]; }
            const double err = sqrt(gn2) * cg_tol;
            __syncthreads();
            for (int k = 1; k <= cg_max; ++k) {
                for (int t = tid; t < ld; t += BLOCK) { vecT[t] = (T)pv[t]; Hp[t] = pv[t] * lambda; }
                __syncthreads();
                sddmm(sb);                                                      // b = U_R p
                __syncthreads();
                for (int i = tid; i < n; i += BLOCK) sb[i] = (T)((double)n0[i] * 2.0 * (double)sb[i]);
                __syncthreads();
                gather_axpy(sb, Hp);
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
            // ---- line search: fresh scores and a fresh scan per try
            double step_len = stepsize0, loss_new = 0.0;
            bool accepted = false;
            for (int it = 0; it < 20; ++it) {
                double nn = 0.0;
                for (int t = tid; t < ld; t += BLOCK) {
                    const double x = vvec[t] + delta[t] * -step_len;
                    vnew[t] = x;
                    vecT[t] = (T)x;
                    nn += (double)(T)x * (double)(T)x;
                }
                nn = block_sum<BLOCK>(nn, red);
                __syncthreads();
                loss_new = eval_point(c1, n1);
                ++n_ls;
                if (lambda / 2.0 * nn + loss_new < prev_obj) { accepted = true; break; }
                step_len /= 2.0;
            }
            if (!accepted) { status = 2; break; }                  // STALLED: v stays where this step found it
            // the accepted point, as the storage type holds it, and its state
            for (int t = tid; t < ld; t += BLOCK) vvec[t] = (double)(T)vnew[t];
            loss0 = loss_new;
            { T* x = c0; c0 = c1; c1 = x; uint32_t* y = n0; n0 = n1; n1 = y; }
            ++n_steps;
            __syncthreads();
        }
        if (status == 1) {                                         // the step cap: vn2 belongs to the point before the last step
            double a = 0.0;
            for (int t = tid; t < ld; t += BLOCK) a += vvec[t] * vvec[t];
            vn2 = block_sum<BLOCK>(a, red);
        }
        for (int t = tid; t < ld; t += BLOCK) Vout[(size_t)j * ld + t] = (T)vvec[t];
        if (tid == 0) {
            double* o = per_item + (size_t)j * 8;
            o[0] = (double)n; o[1] = (double)n_steps; o[2] = (double)n_cg; o[3] = (double)n_ls;
            o[4] = obj_start; o[5] = lambda / 2.0 * vn2 + loss0; o[6] = gn2; o[7] = (double)status;
        }
        __syncthreads();
    }
}
