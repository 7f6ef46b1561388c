// pcr_ridge.h -- k_ridge_direct, k_ridge_cg: squared-loss (ridge) fold-in against a fixed factor matrix F (pcr_fold_in_ridge,
// pcr_fold_in_ridge_model of include/primalcr.h).  Part of pcr_fold.hip.
//
// Per user with ratings r on rows I of F (n of them), A = F[I] (n x k), mu = lambda n (weighted) or lambda:
//     minimise |r - A u|^2 + mu |u|^2   <=>   (A^T A + mu I) u = A^T r  (primal, k x k)   <=>   u = A^T a, (A A^T + mu I) a = r  (dual, n x n)
// One user per workgroup -- 64 threads (one wave) up to PCR_RIDGE_WAVE_MAX ratings, 256 beyond -- in one of three forms, chosen by
// (n, k) alone (pcr_ridge_form, pcr_host.cpp):
//   DUAL / PRIMAL  both are a Gram matrix M = Z^T Z + mu I of side m (Z = A^T, m = n / Z = A, m = k), so both share one code path:
//                  chunks of 16 contraction indices (16 columns of the user's rows / 16 ratings) are staged in LDS as fp64, the next
//                  chunk's loads in flight meanwhile, and the lower-triangular 16 x 16 tiles of M are accumulated in registers on
//                  v_mfma_f64_16x16x4_f64 (the primal form adds b = A^T r from the same staged chunk); then pcr_newton.h's scheme:
//                  tiles of M over the dead staging chunk, blocked Cholesky (diagonal tile by one wave in registers, panel by row-
//                  parallel substitution, trailing update on the matrix cores), two triangular solves by one wave; the dual form
//                  ends with u = A^T a.
//   CG             matrix-free conjugate gradient on the primal system from u = 0: Hp = A^T (A p) + mu p in chunks of 256 ratings
//                  (scores by 16-lane groups, then one thread per column), until |res|^2 <= 1e-24 |b|^2, at most
//                  2 min(n, k) + 10 iterations.
// Everything is fp64 from the moment an element of F is read (the T-accumulating block_sddmm / block_gather_axpy of pcr_prims.h
// would cap an fp32 model's CG at fp32 residuals, so the passes here are their fp64 counterparts); the row is rounded to T on store
// and loss = |r - A u^|^2, obj = loss + mu |u^|^2 are taken at the ROUNDED row in one more pass.  Every sum has a fixed order that
// depends on (n, k) alone, nothing is exchanged between workgroups, no atomics, every loop has a static bound.
//
// The confidence-weighted / implicit fold-in (pcr_fold_in_conf, pcr_fold_in_conf_model) runs the same
// stages on RidgeConf's problem below: the CF = true instantiations of every function here (k_ridge_direct_conf,
// k_ridge_cg_conf; the CF = false kernels keep their symbols and code) and, for alpha > 0, the catalogue Gram of
// k_ridge_catgram / k_ridge_catgram_sum at the end of this file.
#pragma once
#include "pcr_host.h"
#include "pcr_prims.h"

#define RIDGE_TP 17                                   // padded row of a 16 x 16 tile in LDS, doubles (pcr_newton.h's layout)
#define RIDGE_TILE (16 * RIDGE_TP)
#define RIDGE_CG_CHUNK 256

typedef double ridge_f64x4 __attribute__((ext_vector_type(4)));
// v_mfma_f64_16x16x4_f64: lane l gives A[l % 16][l / 16] and B[l % 16][l / 16]; accumulator register e of lane l is C[l / 16 + 4 e][l % 16]
__device__ __forceinline__ ridge_f64x4 ridge_mma(double a, double b, ridge_f64x4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
__device__ __forceinline__ double ridge_readlane(double v, int l) {      // l: wave-uniform
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
__device__ __forceinline__ int ridge_tix(int i, int j) { return i * (i + 1) / 2 + j; }                 // lower-triangular tile (i, j), i >= j
__device__ __forceinline__ bool ridge_pos(double x) { return x > 0.0 && x < INFINITY; }                // positive and finite (false for NaN)
__device__ __forceinline__ double ridge_sum16(double v) {                // sum over a 16-lane group, every lane gets it
    v += lane_xor<8>(v); v += lane_xor<4>(v); v += lane_xor2(v); v += lane_xor1(v);
    return v;
}

// the users' ratings on the device: CSR with item-ascending rows
struct RidgeCsr {
    const int64_t* uptr;
    const int32_t* item;
    const double* val;
};
// What the confidence-weighted / implicit forms (CF, pcr_fold_in_conf*) read besides: per rating the weight
// c_p > 0 in X's order, per user W = sum_p c_p + alpha (rows of F - len), and for alpha > 0 the catalogue Gram G = F^T F
// (k_ridge_catgram below): [ldg][ldg] fp64, both triangles, zeros beyond the rank.  Per user the problem is
//     minimise sum_p c_p (r_p - a_p.u)^2 + alpha (u^T G u - sum_p (a_p.u)^2) + mu |u|^2,    mu = lambda W (weighted) or lambda
//     <=>  (alpha G + sum_p (c_p - alpha) a_p a_p^T + mu I) u = sum_p c_p r_p a_p
// and, for alpha == 0, its dual (A A^T + mu C^-1) a = r, u = A^T a.  Inside a user's functions wt points at the user's weights.
struct RidgeConf {
    const double* wt = nullptr;
    const double* W = nullptr;
    const double* G = nullptr;
    int ldg = 0;
    double alpha = 0.0;
};

// sum over the user's ratings of (val - F[item] . uq)^2 (all: the residual; !resid: val is ignored, the scores' squares), uq: LDS,
// fp64.  16-lane groups take the ratings round robin; a group's sum runs in rating order, the groups are added in group order.
// part: LDS, BLOCK / 16 doubles.  Every thread gets the total.  CF: the terms are c_p (val - score)^2 and *dd receives the
// sum of the scores' squares, in the same order.
template <typename T, int BLOCK, bool CF = false>
__device__ __forceinline__ double ridge_loss(const T* __restrict__ F, const int32_t* __restrict__ item, const double* __restrict__ val, int n,
                                             const double* uq, int r, int ld, double* part, RidgeConf cf = RidgeConf(), double* dd = nullptr) {
    constexpr int NG = BLOCK / 16;
    const int g = threadIdx.x & 15, gi = threadIdx.x >> 4;
    double acc = 0.0, acc2 = 0.0;
    for (int base = 0; base < n; base += NG) {
        const int p = base + gi;
        const bool live = p < n;
        double d = 0.0;
        if (live) {
            const T* row = F + (size_t)item[p] * ld;
            for (int t = g; t < r; t += 16) d += (double)row[t] * uq[t];
        }
        d = ridge_sum16(d);
        if (live) {
            const double e = val[p] - d;
            if (CF) { acc += (cf.wt[p] * e) * e; acc2 += d * d; }
            else acc += e * e;
        }
    }
    __syncthreads();
    if (g == 0) part[gi] = acc;
    __syncthreads();
    double tot = 0.0;
#pragma unroll
    for (int q = 0; q < NG; ++q) tot += part[q];
    __syncthreads();
    if (CF) {
        if (g == 0) part[gi] = acc2;
        __syncthreads();
        double t2 = 0.0;
#pragma unroll
        for (int q = 0; q < NG; ++q) t2 += part[q];
        __syncthreads();
        *dd = t2;
    }
    return tot;
}

// the end of a user, every form: the row rounded to T and stored (pad columns zero), loss and obj at the rounded row, the table
// line.  uvec: the solution in LDS (r entries; status != OK: ignored, the row is zeros and loss = |r|^2); uq: LDS scratch of r
// doubles (may be uvec itself).  CF: loss = sum_p c_p (r_p - a_p.u^)^2 + alpha (u^^T G u^ - sum_p (a_p.u^)^2); u^^T G u^ by one
// thread per column of G, the columns added by block_sum.
template <typename T, int BLOCK, bool CF = false>
__device__ __forceinline__ void ridge_finish(const T* __restrict__ F, const int32_t* __restrict__ item, const double* __restrict__ val, int n,
                                             double* uvec, int r, int ld, double mu, int form, int iters, int status, T* __restrict__ urow,
                                             double* __restrict__ o, double* part, double* red, RidgeConf cf = RidgeConf()) {
    const int tid = threadIdx.x;
    const bool zero = status == PCR_RIDGE_SINGULAR;
    double nn = 0.0;
    for (int t = tid; t < ld; t += BLOCK) {
        const T q = (t < r && !zero) ? (T)uvec[t] : (T)0;
        urow[t] = q;
        nn += (double)q * (double)q;
    }
    __syncthreads();
    for (int t = tid; t < r; t += BLOCK) uvec[t] = zero ? 0.0 : (double)(T)uvec[t];
    __syncthreads();
    nn = block_sum<BLOCK>(nn, red);
    double dd = 0.0;
    double loss = ridge_loss<T, BLOCK, CF>(F, item, val, n, uvec, r, ld, part, cf, &dd);
    if (CF && cf.alpha > 0.0) {                                          // (uniform)
        double q = 0.0;
        for (int t = tid; t < r; t += BLOCK) {
            double s = 0.0;
            for (int j = 0; j < r; ++j) s += cf.G[(size_t)j * cf.ldg + t] * uvec[j];
            q += s * uvec[t];
        }
        const double ugu = block_sum<BLOCK>(q, red);
        loss += cf.alpha * (ugu - dd);
    }
    if (tid == 0) {
        o[0] = (double)n; o[1] = (double)form; o[2] = (double)iters; o[3] = loss; o[4] = loss + mu * nn; o[5] = (double)status;
    }
    __syncthreads();
}

// LDS of k_ridge_direct: the m-vectors, the solution / row (max(mp, ld)), the dual form's items and ratings, then ONE region for
// the staging chunk (16 x (mp + 1) doubles) and, after the build, the tiles of M
static inline size_t ridge_direct_bytes(int mp, int ld, int block) {
    const int nt = mp / 16;
    const size_t stage = carve_bytes((size_t)16 * (mp + 1), 8), tiles = carve_bytes((size_t)(nt * (nt + 1) / 2) * RIDGE_TILE, 8);
    return carve_bytes(8, 8) + carve_bytes(block / 16, 8) + carve_bytes(16, 8) + 3 * carve_bytes(mp, 8) + carve_bytes(std::max(mp, ld), 8) +
           carve_bytes(mp, 4) + std::max(stage, tiles);
}

// The three stages of the direct forms as workgroup functions: k_ridge_direct below and k_nnls_direct (pcr_nnls.h) run the same
// ones.  Every thread of the workgroup calls ridge_gram and ridge_chol (both hold barriers); ridge_trisolve is wave 0's.
//
// 1. M's lower-triangular tiles on the matrix cores, 16 contraction indices at a time.  dual != 0: M = A A^T + mu I (m = n; itm:
//    the user's items in LDS); else M = A^T A + mu I (m = r) and the return value is b[tid] = (A^T r)[tid] for tid < mp.  Zc: the
//    staging chunk [16][mp + 1], over which the tiles are written at the end (the caller's barrier makes them visible); rch: 16
//    doubles.  Rows / columns beyond m are zeros with a unit diagonal, which the factorisation passes through unchanged.
//    CF (rch: 32 doubles; cw: the user's weights in LDS, mp of them, ones beyond n): the dual diagonal is mu / c_p; the primal
//    accumulators start from alpha G's tiles (alpha > 0; mp == cf.ldg), the A operand of each staged rating is scaled by
//    c_p - alpha (rch[16..31]) and b takes c_p r_p (rch[0..15]).
template <typename T, int BLOCK, bool CF = false>
__device__ __forceinline__ double ridge_gram(const T* __restrict__ F, const int32_t* __restrict__ uit, const double* __restrict__ uval, int n, int r, int ld,
                                             int m, int mp, int dual, double mu, const int32_t* itm, double* rch, double* Zc,
                                             RidgeConf cf = RidgeConf(), const double* cw = nullptr) {
    constexpr int NW = BLOCK / PCR_WAVE, MAXM = BLOCK == 64 ? 64 : 112, MAXT = MAXM / 16;
    constexpr int MAXP = (MAXT * (MAXT + 1) / 2 + NW - 1) / NW;          // tile pairs per wave: 10 (one wave, 4 x 4 tiles) or 7 (four waves, 7 x 7)
    constexpr int RPP = BLOCK / 16, NREG = 16 * MAXM / BLOCK;            // staging: rows per pass, values per thread (16 or 7)
    double* Tl = Zc;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int mps = mp + 1, nt = mp / 16, npairs = nt * (nt + 1) / 2;
    const int row = lane & 15, kh = lane >> 4;                           // MFMA operand indices of this lane
    const int pp = tid >> 4, t16 = tid & 15;
    const int clen = dual ? r : n;                                   // contraction length: columns (dual) or ratings (primal)
    ridge_f64x4 acc[MAXP];
#pragma unroll
    for (int q = 0; q < MAXP; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[q][e] = 0.0;
    int offA[MAXP], offB[MAXP];                                      // this wave's tile pairs (I >= J) as offsets inside a staged row
#pragma unroll
    for (int q = 0; q < MAXP; ++q) {
        const int pr = wid + q * NW;
        int I = 0, rem = pr < npairs ? pr : 0;                       // pr -> (I, J), J <= I, row-major over the lower triangle
        while (rem > I) { rem -= I + 1; ++I; }
        offA[q] = I * 16 + row; offB[q] = rem * 16 + row;
        if (CF && !dual && cf.alpha > 0.0 && pr < npairs) {              // (uniform) alpha G's tile (I, rem), in the accumulator's layout
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[q][e] = cf.alpha * cf.G[(size_t)(I * 16 + kh + 4 * e) * cf.ldg + rem * 16 + row];
        }
    }
    T xr[NREG];
    double rreg = 0.0, wreg = 0.0;
    // issue(): the next chunk's values into registers; consume(): into the (idle) staging chunk as fp64.
    //   primal: thread (pp, t16) holds ratings c0 + pp + RPP j (j < 16 / RPP) x columns t16 + 16 k  -> Zc[rating][column]
    //   dual:   thread (pp, t16) holds column c0 + t16 of the user's rows pp + RPP j (j < NREG)      -> Zc[column][rating]
    auto issue = [&](int c0) {
#pragma unroll
        for (int j = 0; j < NREG; ++j) xr[j] = (T)0;
        if (dual) {
            const int c = c0 + t16;
#pragma unroll
            for (int j = 0; j < NREG; ++j) {
                const int p = pp + RPP * j;
                if (p < n && c < r) xr[j] = F[(size_t)itm[p] * ld + c];
            }
        } else {
            constexpr int NCK = MAXM / 16;
#pragma unroll
            for (int j = 0; j < 16 / RPP; ++j) {
                const int p = c0 + pp + RPP * j;
                if (p < n) {
                    const T* frow = F + (size_t)uit[p] * ld;
#pragma unroll
                    for (int k = 0; k < NCK; ++k) { const int c = t16 + 16 * k; if (c < r) xr[j * NCK + k] = frow[c]; }
                }
            }
            if (CF) {
                if (tid < 16) {
                    const double c = c0 + tid < n ? cf.wt[c0 + tid] : 0.0;
                    rreg = c0 + tid < n ? c * uval[c0 + tid] : 0.0;
                    wreg = c0 + tid < n ? c - cf.alpha : 0.0;
                }
            } else if (tid < 16) rreg = c0 + tid < n ? uval[c0 + tid] : 0.0;
        }
    };
    auto consume = [&]() {
        if (dual) {
#pragma unroll
            for (int j = 0; j < NREG; ++j) { const int p = pp + RPP * j; if (p < mp) Zc[t16 * mps + p] = (double)xr[j]; }
        } else {
            constexpr int NCK = MAXM / 16;
#pragma unroll
            for (int j = 0; j < 16 / RPP; ++j)
#pragma unroll
                for (int k = 0; k < NCK; ++k) { const int c = t16 + 16 * k; if (c < mp) Zc[(pp + RPP * j) * mps + c] = (double)xr[j * NCK + k]; }
            if (tid < 16) { rch[tid] = rreg; if (CF) rch[16 + tid] = wreg; }
        }
    };
    double bacc = 0.0;                                               // primal: b[tid] = (A^T r)[tid]
    issue(0);
    consume();
    __syncthreads();
    for (int c0 = 0; c0 < clen; c0 += 16) {
        const bool more = c0 + 16 < clen;
        if (more) issue(c0 + 16);
#pragma unroll 1
        for (int s4 = 0; s4 < 4; ++s4) {                             // (not unrolled: one k-step's operands in registers at a time)
            const int pb = (s4 * 4 + kh) * mps;
            if (CF) {
                const double wk = dual ? 1.0 : rch[16 + s4 * 4 + kh];
#pragma unroll
                for (int q = 0; q < MAXP; ++q)
                    if (wid + q * NW < npairs) acc[q] = ridge_mma(Zc[pb + offA[q]] * wk, Zc[pb + offB[q]], acc[q]);
            } else {
#pragma unroll
                for (int q = 0; q < MAXP; ++q)
                    if (wid + q * NW < npairs) acc[q] = ridge_mma(Zc[pb + offA[q]], Zc[pb + offB[q]], acc[q]);      // (wave-uniform)
            }
        }
        if (!dual && tid < mp) {
#pragma unroll
            for (int p = 0; p < 16; ++p) bacc += Zc[p * mps + tid] * rch[p];
        }
        __syncthreads();
        if (more) { consume(); __syncthreads(); }
    }
    // M = Z^T Z + mu I into the tiles (over the staging chunk: the loop above ends in a barrier); beyond m a unit diagonal
#pragma unroll
    for (int q = 0; q < MAXP; ++q) {
        const int pr = wid + q * NW;
        if (pr < npairs) {
            int I = 0, rem = pr;
            while (rem > I) { rem -= I + 1; ++I; }
            double* tile = Tl + (size_t)ridge_tix(I, rem) * RIDGE_TILE;
            const int cl = lane & 15, col = rem * 16 + cl;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int rl = (lane >> 4) + 4 * e, rw = I * 16 + rl;
                double v = acc[q][e] + (rw == col ? ((CF && dual) ? mu / cw[rw] : mu) : 0.0);
                if (rw >= m || col >= m) v = rw == col ? 1.0 : 0.0;
                tile[rl * RIDGE_TP + cl] = v;
            }
        }
    }
    return bacc;
}

// 2. blocked Cholesky of the nt x nt tiles Tl (lower triangle, in place; pcr_newton.h's scheme); dinv: 1 / L[i][i].  The caller
//    has set red[7] = 0 (the "not positive definite" flag) behind a barrier.  Returns true for a pivot that is <= 0 or not finite.
template <int BLOCK>
__device__ __forceinline__ bool ridge_chol(double* Tl, double* dinv, double* red, int nt) {
    constexpr int NW = BLOCK / PCR_WAVE;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int row = lane & 15, kh = lane >> 4;
    for (int k = 0; k < nt; ++k) {
        double* D = Tl + (size_t)ridge_tix(k, k) * RIDGE_TILE;
        if (wid == 0) {                                              // (a) the diagonal tile: lanes 0..15 hold one ROW each in registers
            double a[16];
            const int rr = lane & 15;
#pragma unroll
            for (int c = 0; c < 16; ++c) a[c] = D[rr * RIDGE_TP + c];
            bool pd = true;
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) {
#pragma unroll
                for (int j = 0; j < kk; ++j) a[kk] -= a[j] * ridge_readlane(a[j], kk);
                const double dkk = ridge_readlane(a[kk], kk);
                pd = pd && ridge_pos(dkk);                           // (uniform)
                const double ri = 1.0 / sqrt(dkk);
                a[kk] = rr == kk ? dkk * ri : a[kk] * ri;
                if (lane == 0) dinv[k * 16 + kk] = ri;
            }
            if (!pd) { if (lane == 0) red[7] = 1.0; }
            else if (lane < 16) {
#pragma unroll
                for (int c = 0; c < 16; ++c) D[rr * RIDGE_TP + c] = a[c];
            }
        }
        __syncthreads();
        if (red[7] != 0.0) break;                                    // (uniform: read behind the barrier)
        const int below = nt - k - 1;
        if (tid < below * 16) {                                      // (b) the panel below: X L_kk^T = A, one row per thread (below <= 6, 3 on one wave)
            double* A = Tl + (size_t)ridge_tix(k + 1 + (tid >> 4), k) * RIDGE_TILE + (tid & 15) * RIDGE_TP;
            double x[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) x[c] = A[c];
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                double sacc = x[c];
#pragma unroll
                for (int j = 0; j < c; ++j) sacc -= x[j] * D[c * RIDGE_TP + j];
                x[c] = sacc * dinv[k * 16 + c];
            }
#pragma unroll
            for (int c = 0; c < 16; ++c) A[c] = x[c];
        }
        __syncthreads();
        const int tp = below * (below + 1) / 2;                      // (c) trailing update A_ij -= L_ik L_jk^T on the matrix cores
        for (int pr = wid; pr < tp; pr += NW) {
            int i = 0, rem = pr;
            while (rem > i) { rem -= i + 1; ++i; }
            double* Cm = Tl + (size_t)ridge_tix(k + 1 + i, k + 1 + rem) * RIDGE_TILE;
            const double* Li = Tl + (size_t)ridge_tix(k + 1 + i, k) * RIDGE_TILE;
            const double* Lj = Tl + (size_t)ridge_tix(k + 1 + rem, k) * RIDGE_TILE;
            ridge_f64x4 c4;
#pragma unroll
            for (int e = 0; e < 4; ++e) c4[e] = Cm[((lane >> 4) + 4 * e) * RIDGE_TP + (lane & 15)];
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) c4 = ridge_mma(-Li[row * RIDGE_TP + s4 * 4 + kh], Lj[row * RIDGE_TP + s4 * 4 + kh], c4);
#pragma unroll
            for (int e = 0; e < 4; ++e) Cm[((lane >> 4) + 4 * e) * RIDGE_TP + (lane & 15)] = c4[e];
        }
        __syncthreads();
    }
    return red[7] != 0.0;
}

// 3. the two triangular solves, M x = gv in place, with the factor ridge_chol left: one wave, lane l holds entries l and l + 64
//    (pcr_newton.h)
__device__ __forceinline__ void ridge_trisolve(const double* Tl, const double* dinv, double* gv, int mp, int nt) {
    const int lane = threadIdx.x & 63;
    const int j0 = lane, j1 = lane + 64, t0 = j0 >> 4, t1 = j1 >> 4;
    double y0 = j0 < mp ? gv[j0] : 0.0, y1 = j1 < mp ? gv[j1] : 0.0;
    const double dv0 = j0 < mp ? dinv[j0] : 1.0, dv1 = j1 < mp ? dinv[j1] : 1.0;
    const int tc0 = t0 < nt ? t0 : nt - 1, tc1 = t1 < nt ? t1 : nt - 1;
    for (int ib = 0; ib < nt; ++ib) {                            // L y = g, one tile column of L at a time
        double l0[16], l1[16];
        const double* q0 = Tl + (size_t)ridge_tix(tc0 < ib ? ib : tc0, ib) * RIDGE_TILE + (j0 & 15) * RIDGE_TP;
        const double* q1 = Tl + (size_t)ridge_tix(tc1 < ib ? ib : tc1, ib) * RIDGE_TILE + (j1 & 15) * RIDGE_TP;
#pragma unroll
        for (int ii = 0; ii < 16; ++ii) { l0[ii] = q0[ii]; l1[ii] = q1[ii]; }
        if (ib < 4) {
#pragma unroll
            for (int ii = 0; ii < 16; ++ii) {
                const int i = ib * 16 + ii;
                const double yi = ridge_readlane(y0 * dv0, i);
                y0 = j0 == i ? yi : (j0 > i ? y0 - l0[ii] * yi : y0);
                y1 = j1 < mp ? y1 - l1[ii] * yi : y1;
            }
        } else {
#pragma unroll
            for (int ii = 0; ii < 16; ++ii) {
                const int i = ib * 16 + ii;
                const double yi = ridge_readlane(y1 * dv1, i - 64);
                y1 = j1 == i ? yi : ((j1 > i && j1 < mp) ? y1 - l1[ii] * yi : y1);
            }
        }
    }
    for (int ib = nt - 1; ib >= 0; --ib) {                       // L^T x = y (in place), one tile ROW of L at a time
        double l0[16], l1[16];
        const double* q0 = Tl + (size_t)ridge_tix(ib, tc0 > ib ? ib : tc0) * RIDGE_TILE + (j0 & 15);
        const double* q1 = Tl + (size_t)ridge_tix(ib, tc1 > ib ? ib : tc1) * RIDGE_TILE + (j1 & 15);
#pragma unroll
        for (int ii = 0; ii < 16; ++ii) { l0[ii] = q0[ii * RIDGE_TP]; l1[ii] = q1[ii * RIDGE_TP]; }
        if (ib >= 4) {
#pragma unroll
            for (int ii = 15; ii >= 0; --ii) {
                const int i = ib * 16 + ii;
                const double xi = ridge_readlane(y1 * dv1, i - 64);
                y1 = j1 == i ? xi : ((j1 < i && j1 < mp) ? y1 - l1[ii] * xi : y1);
                y0 -= l0[ii] * xi;                               // (j0 < i for every i >= 64)
            }
        } else {
#pragma unroll
            for (int ii = 15; ii >= 0; --ii) {
                const int i = ib * 16 + ii;
                const double xi = ridge_readlane(y0 * dv0, i);
                y0 = j0 == i ? xi : ((j0 < i && j0 < mp) ? y0 - l0[ii] * xi : y0);
            }
        }
    }
    if (j0 < mp) gv[j0] = y0;
    if (j1 < mp) gv[j1] = y1;
}

// dual != 0: M = A A^T + mu I (m = n); else M = A^T A + mu I (m = r).  mp: the launch's padded side (a multiple of 16, at least
// every user's m; BLOCK = 64: at most 64, BLOCK = 256: at most 112).  A user's results do not depend on mp: rows / columns beyond
// m are zeros with a unit diagonal, which the factorisation passes through unchanged.
// The body of both kernels below.  CF (k_ridge_direct_conf): the weighted / implicit problem of RidgeConf above -- the dual form
// runs at alpha == 0 only (pcr_conf_form), the primal form's mp is cf.ldg.
template <typename T, int BLOCK, bool CF>
__device__ __forceinline__ void ridge_direct_body(char* smem, RidgeCsr X, const int32_t* __restrict__ users, int nusers, const T* __restrict__ F, int r, int ld,
                                                  T* __restrict__ Uout, double* __restrict__ per_user, double lambda, int weighted, int dual, int mp,
                                                  RidgeConf cf) {
    Carver cv(smem);
    double* red = cv.take<double>(8);
    double* part = cv.take<double>(BLOCK / 16);
    double* rch = cv.take<double>(CF ? 32 : 16);                         // the staged chunk's ratings (primal; CF: c r, then c - alpha)
    double* gv = cv.take<double>(mp);                                    // right-hand side, then the solution
    double* dinv = cv.take<double>(mp);                                  // 1 / L[i][i]
    double* rv = cv.take<double>(mp);                                    // dual: the user's ratings
    double* uvec = cv.take<double>(mp > ld ? mp : ld);
    int32_t* itm = cv.take<int32_t>(mp);                                 // dual: the user's items
    double* cw = CF ? cv.take<double>(mp) : nullptr;                     // CF, dual: the user's weights
    double* Zc = reinterpret_cast<double*>(cv.p);                        // staging chunk [16][mp + 1] ...
    double* Tl = Zc;                                                     // ... and the tiles of M over it
    const int tid = threadIdx.x, wid = tid >> 6;
    const int nt = mp / 16;

    for (int ui = blockIdx.x; ui < nusers; ui += gridDim.x) {
        const int u = users[ui];
        const int64_t s0 = X.uptr[u];
        const int n = (int)(X.uptr[u + 1] - s0);
        const int m = dual ? n : r;
        const double mu = weighted ? lambda * (CF ? cf.W[u] : (double)n) : lambda;
        const int32_t* uit = X.item + s0;
        const double* uval = X.val + s0;
        T* urow = Uout + (size_t)u * ld;
        double* o = per_user + (size_t)u * PCR_RIDGE_FIELDS;
        const int form = dual ? PCR_RIDGE_DUAL : PCR_RIDGE_PRIMAL;
        RidgeConf cu = cf;
        if (CF) cu.wt = cf.wt + s0;
        if (n == 0) {                                                    // (uniform) a zero row, loss = obj = 0
            for (int t = tid; t < ld; t += BLOCK) urow[t] = (T)0;
            if (tid == 0) { o[0] = 0.0; o[1] = (double)form; o[2] = 0.0; o[3] = 0.0; o[4] = 0.0; o[5] = (double)PCR_RIDGE_OK; }
            continue;
        }
        if (dual)
            for (int p = tid; p < mp; p += BLOCK) {
                itm[p] = p < n ? uit[p] : 0; rv[p] = p < n ? uval[p] : 0.0;
                if (CF) cw[p] = p < n ? cu.wt[p] : 1.0;
            }
        __syncthreads();
        const double bacc = ridge_gram<T, BLOCK, CF>(F, uit, uval, n, r, ld, m, mp, dual, mu, itm, rch, Zc, cu, cw);
        for (int t = tid; t < mp; t += BLOCK) gv[t] = dual ? rv[t] : (t < m ? bacc : 0.0);      // (primal: mp <= BLOCK, one pass)
        if (tid == 0) red[7] = 0.0;                                      // "not positive definite" flag
        __syncthreads();
        const bool bad = ridge_chol<BLOCK>(Tl, dinv, red, nt);
        if (wid == 0 && !bad) ridge_trisolve(Tl, dinv, gv, mp, nt);
        __syncthreads();
        // ---- 4. the row: the solution itself (primal) or u = A^T a (dual; one thread per column, the ratings in order)
        if (!bad) {
            if (dual) {
                for (int t = tid; t < r; t += BLOCK) {
                    double s = 0.0;
#pragma unroll 4
                    for (int p = 0; p < n; ++p) s += gv[p] * (double)F[(size_t)itm[p] * ld + t];
                    uvec[t] = s;
                }
            } else {
                for (int t = tid; t < r; t += BLOCK) uvec[t] = gv[t];
            }
        }
        __syncthreads();
        ridge_finish<T, BLOCK, CF>(F, uit, uval, n, uvec, r, ld, mu, form, 0, bad ? PCR_RIDGE_SINGULAR : PCR_RIDGE_OK, urow, o, part, red, cu);
    }
}

template <typename T, int BLOCK>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(2))) void k_ridge_direct(RidgeCsr X, const int32_t* __restrict__ users, int nusers, const T* __restrict__ F, int r, int ld,
                                                        T* __restrict__ Uout, double* __restrict__ per_user, double lambda, int weighted, int dual,
                                                        int mp) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    ridge_direct_body<T, BLOCK, false>(smem, X, users, nusers, F, r, ld, Uout, per_user, lambda, weighted, dual, mp, RidgeConf());
}
// The weighted / implicit instantiation (pcr_fold_in_conf*): the same stages on RidgeConf's problem
template <typename T, int BLOCK>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(2))) void k_ridge_direct_conf(RidgeCsr X, const int32_t* __restrict__ users, int nusers, const T* __restrict__ F, int r,
                                                        int ld, T* __restrict__ Uout, double* __restrict__ per_user, double lambda, int weighted,
                                                        int dual, int mp, RidgeConf cf) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    ridge_direct_body<T, BLOCK, true>(smem, X, users, nusers, F, r, ld, Uout, per_user, lambda, weighted, dual, mp, cf);
}
static inline size_t ridge_direct_conf_bytes(int mp, int ld, int block) { return ridge_direct_bytes(mp, ld, block) + carve_bytes(16, 8) + carve_bytes(mp, 8); }

static inline size_t ridge_cg_bytes(int ld) {
    return carve_bytes(8, 8) + carve_bytes(16, 8) + 4 * carve_bytes(ld, 8) + carve_bytes(RIDGE_CG_CHUNK, 8) + carve_bytes(RIDGE_CG_CHUNK, 4);
}

// The CG form's two pieces as functions of a 256-thread workgroup: k_ridge_cg below and k_nnls_cg (pcr_nnls.h) run the same ones.
//
// out[t] (+)= sum over the user's ratings of w_p F[item p][t], w = the ratings (vec NULL) or the scores F[item p] . vec; in chunks of
// RIDGE_CG_CHUNK ratings (scores by 16-lane groups, then one thread per column).  sc, itc: LDS, one chunk each.
// CF: w = c_p r_p (vec NULL) or (c_p - alpha) F[item p] . vec.
template <typename T, bool CF = false>
__device__ __forceinline__ void ridge_cg_apply(const T* __restrict__ F, const int32_t* __restrict__ uit, const double* __restrict__ uval, int n, int r, int ld,
                                               const double* vec, double* out, double* sc, int32_t* itc, RidgeConf cf = RidgeConf()) {
    constexpr int BLOCK = 256, CH = RIDGE_CG_CHUNK;
    const int tid = threadIdx.x, g = tid & 15, gi = tid >> 4;
    for (int c0 = 0; c0 < n; c0 += CH) {
        const int cn = n - c0 < CH ? n - c0 : CH;
        if (tid < cn) { itc[tid] = uit[c0 + tid]; if (!vec) sc[tid] = CF ? cf.wt[c0 + tid] * uval[c0 + tid] : uval[c0 + tid]; }
        __syncthreads();
        if (vec) {
            for (int base = 0; base < cn; base += 16) {
                const int p = base + gi;
                double d = 0.0;
                if (p < cn) {
                    const T* row = F + (size_t)itc[p] * ld;
                    for (int t = g; t < r; t += 16) d += (double)row[t] * vec[t];
                }
                d = ridge_sum16(d);
                if (p < cn && g == 0) sc[p] = CF ? (cf.wt[c0 + p] - cf.alpha) * d : d;
            }
            __syncthreads();
        }
        for (int t = tid; t < r; t += BLOCK) {
            double s = out[t];
#pragma unroll 4
            for (int p = 0; p < cn; ++p) s += sc[p] * (double)F[(size_t)itc[p] * ld + t];
            out[t] = s;
        }
        __syncthreads();
    }
}

// CG on (A^T A + mu I) u = b from u = 0 until |res|^2 <= 1e-24 |b|^2, at most 2 min(n, side) + 10 iterations.  On entry uvec = 0
// and res = b.  pas == NULL: the whole system, side = r.  Else the system restricted to the coordinates with pas[t] != 0 (side =
// npas of them; the caller has zeroed res on the others): the search direction stays zero outside them and Hp is masked to
// them, Hp = mask(A^T (A p) + mu p).  Returns the status (PCR_RIDGE_OK / SINGULAR / CG_CAP); *iters: the iterations.
// CF: Hp = A^T ((c - alpha) o (A p)) + alpha G p + mu p, G p by one thread per column of G; alpha > 0: at most 2 side + 10 iterations.
template <typename T, bool CF = false>
__device__ __forceinline__ int ridge_cg_solve(const T* __restrict__ F, const int32_t* __restrict__ uit, const double* __restrict__ uval, int n, int r, int ld,
                                              double mu, const int32_t* pas, int npas, double* uvec, double* res, double* pv, double* Hp, double* sc,
                                              int32_t* itc, double* red, int* iters_out, RidgeConf cf = RidgeConf()) {
    constexpr int BLOCK = 256;
    const int tid = threadIdx.x;
    double a = 0.0;
    for (int t = tid; t < r; t += BLOCK) { pv[t] = res[t]; a += res[t] * res[t]; }
    double rr = block_sum<BLOCK>(a, red);
    const double stop = 1e-24 * rr;
    const int side = pas ? npas : r;
    const int cap = (CF && cf.alpha > 0.0) ? 2 * side + 10 : 2 * (n < side ? n : side) + 10;
    int iters = 0, status = rr <= stop ? PCR_RIDGE_OK : PCR_RIDGE_CG_CAP;          // (b = 0: u = 0 is the answer)
    __syncthreads();
    for (int it = 0; it < cap && status == PCR_RIDGE_CG_CAP; ++it) {
        if (CF && cf.alpha > 0.0) {                                      // (uniform)
            for (int t = tid; t < r; t += BLOCK) {
                double s = 0.0;
                for (int j = 0; j < r; ++j) s += cf.G[(size_t)j * cf.ldg + t] * pv[j];
                Hp[t] = mu * pv[t] + cf.alpha * s;
            }
        } else {
            for (int t = tid; t < r; t += BLOCK) Hp[t] = mu * pv[t];
        }
        __syncthreads();
        ridge_cg_apply<T, CF>(F, uit, uval, n, r, ld, pv, Hp, sc, itc, cf);
        if (pas)
            for (int t = tid; t < r; t += BLOCK) if (!pas[t]) Hp[t] = 0.0;       // (the thread that wrote Hp[t])
        a = 0.0;
        for (int t = tid; t < r; t += BLOCK) a += pv[t] * Hp[t];
        const double pHp = block_sum<BLOCK>(a, red);
        ++iters;
        if (!ridge_pos(pHp)) { status = PCR_RIDGE_SINGULAR; break; }                // (uniform)
        const double alpha = rr / pHp;
        a = 0.0;
        for (int t = tid; t < r; t += BLOCK) {
            uvec[t] += alpha * pv[t];
            const double rn = res[t] - alpha * Hp[t];
            res[t] = rn;
            a += rn * rn;
        }
        const double rr2 = block_sum<BLOCK>(a, red);
        if (rr2 <= stop) { status = PCR_RIDGE_OK; break; }
        const double beta = rr2 / rr;
        rr = rr2;
        for (int t = tid; t < r; t += BLOCK) pv[t] = res[t] + beta * pv[t];
        __syncthreads();
    }
    __syncthreads();
    *iters_out = iters;
    return status;
}

// Matrix-free CG on (A^T A + mu I) u = A^T r from u = 0; 256 threads per user, any n and k.  The body of both kernels below; CF
// (k_ridge_cg_conf): RidgeConf's system.
template <typename T, bool CF>
__device__ __forceinline__ void ridge_cg_body(char* smem, RidgeCsr X, const int32_t* __restrict__ users, int nusers, const T* __restrict__ F, int r, int ld,
                                              T* __restrict__ Uout, double* __restrict__ per_user, double lambda, int weighted, RidgeConf cf) {
    constexpr int BLOCK = 256, CH = RIDGE_CG_CHUNK;
    Carver cv(smem);
    double* red = cv.take<double>(8);
    double* part = cv.take<double>(16);
    double* uvec = cv.take<double>(ld);
    double* res = cv.take<double>(ld);
    double* pv = cv.take<double>(ld);
    double* Hp = cv.take<double>(ld);
    double* sc = cv.take<double>(CH);
    int32_t* itc = cv.take<int32_t>(CH);
    const int tid = threadIdx.x;

    for (int ui = blockIdx.x; ui < nusers; ui += gridDim.x) {
        const int u = users[ui];
        const int64_t s0 = X.uptr[u];
        const int n = (int)(X.uptr[u + 1] - s0);
        const double mu = weighted ? lambda * (CF ? cf.W[u] : (double)n) : lambda;
        const int32_t* uit = X.item + s0;
        const double* uval = X.val + s0;
        RidgeConf cu = cf;
        if (CF) cu.wt = cf.wt + s0;
        for (int t = tid; t < r; t += BLOCK) { uvec[t] = 0.0; res[t] = 0.0; }
        __syncthreads();
        ridge_cg_apply<T, CF>(F, uit, uval, n, r, ld, nullptr, res, sc, itc, cu);       // b = A^T r: the first residual and direction
        int iters = 0;
        const int status = ridge_cg_solve<T, CF>(F, uit, uval, n, r, ld, mu, nullptr, 0, uvec, res, pv, Hp, sc, itc, red, &iters, cu);
        ridge_finish<T, BLOCK, CF>(F, uit, uval, n, uvec, r, ld, mu, PCR_RIDGE_CG, iters, status, Uout + (size_t)u * ld,
                                   per_user + (size_t)u * PCR_RIDGE_FIELDS, part, red, cu);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_ridge_cg(RidgeCsr X, const int32_t* __restrict__ users, int nusers, const T* __restrict__ F, int r, int ld,
                                                  T* __restrict__ Uout, double* __restrict__ per_user, double lambda, int weighted) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    ridge_cg_body<T, false>(smem, X, users, nusers, F, r, ld, Uout, per_user, lambda, weighted, RidgeConf());
}
template <typename T>
__global__ __launch_bounds__(256) void k_ridge_cg_conf(RidgeCsr X, const int32_t* __restrict__ users, int nusers, const T* __restrict__ F, int r, int ld,
                                                       T* __restrict__ Uout, double* __restrict__ per_user, double lambda, int weighted, RidgeConf cf) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    ridge_cg_body<T, true>(smem, X, users, nusers, F, r, ld, Uout, per_user, lambda, weighted, cf);
}

// ---- the catalogue Gram G = F^T F of the implicit forms (alpha > 0), fp64, once per call, any rank.
// The columns are cut into panels of RIDGE_CAT_PANEL (4 tiles of 16), the rows into nb row blocks -- ridge_catgram_blocks: a
// function of (rows, k) alone, never of the device or the grid.  Workgroup (b, panel pair PI >= PJ) of k_ridge_catgram walks its
// row block in slabs of 16 rows: the slab's two column panels are staged in LDS as fp64 (the next slab's loads in flight
// meanwhile) and the 16 tile pairs (4 x 4; the lower triangle on a diagonal panel pair) are dealt to the four waves, 4 each, on
// v_mfma_f64_16x16x4_f64.  It writes its PARTIAL tiles, in the accumulator's layout; k_ridge_catgram_sum adds the nb partials of
// every entry in block order and writes both triangles of G [ldg][ldg], ldg = roundup(k, 16) (columns beyond the rank are read
// as zeros, so G's pad rows and columns are zeros).  No atomics, no counters: the workgroups meet at the kernel boundary only.
#define RIDGE_CAT_PANEL 64
#define RIDGE_CAT_LDS (2 * RIDGE_CAT_PANEL + 1)
static inline int ridge_catgram_pairs(int64_t k) { const int64_t np = (k + RIDGE_CAT_PANEL - 1) / RIDGE_CAT_PANEL; return (int)(np * (np + 1) / 2); }
static inline int ridge_catgram_blocks(int64_t rows, int64_t k) {        // 1024 rows per block, at most 64 blocks and 256 MB of partials
    const int64_t by_rows = std::min<int64_t>(64, (rows + 1023) / 1024), per_block = (int64_t)ridge_catgram_pairs(k) * 16 * 256 * 8;
    return (int)std::max<int64_t>(1, std::min<int64_t>(by_rows, ((int64_t)256 << 20) / per_block));
}

template <typename T>
__global__ __launch_bounds__(256) void k_ridge_catgram(const T* __restrict__ F, int64_t rows, int r, int ld, int nb, double* __restrict__ part) {
    __shared__ double Z[16 * RIDGE_CAT_LDS];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int row = lane & 15, kh = lane >> 4, pp = tid >> 4, t16 = tid & 15;
    const int nt = (r + 15) / 16;
    int PI = 0, PJ = (int)blockIdx.y;                                    // panel pair, row-major over the lower triangle
    while (PJ > PI) { PJ -= PI + 1; ++PI; }
    const int64_t per = ((rows + nb - 1) / nb + 15) / 16 * 16;           // rows per block, a multiple of the slab
    const int64_t r0 = (int64_t)blockIdx.x * per, r1 = r0 + per < rows ? r0 + per : rows;
    ridge_f64x4 acc[4];
    bool live[4];
    int offA[4], offB[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int t = wid + 4 * q, ti = t >> 2, tj = t & 3, gI = PI * 4 + ti, gJ = PJ * 4 + tj;
        live[q] = gI < nt && gJ < nt && gI >= gJ;                        // (wave-uniform)
        offA[q] = ti * 16 + row; offB[q] = RIDGE_CAT_PANEL + tj * 16 + row;
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[q][e] = 0.0;
    }
    T xr[8];
    auto issue = [&](int64_t p0) {                                       // row p0 + pp, columns t16 + 16 j of panel PI (j < 4) and PJ
        const int64_t p = p0 + pp;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = (j < 4 ? PI : PJ) * RIDGE_CAT_PANEL + t16 + 16 * (j & 3);
            xr[j] = (p < r1 && c < r) ? F[(size_t)p * ld + c] : (T)0;
        }
    };
    auto consume = [&]() {
#pragma unroll
        for (int j = 0; j < 8; ++j) Z[pp * RIDGE_CAT_LDS + 16 * j + t16] = (double)xr[j];
    };
    if (r0 < r1) { issue(r0); consume(); }
    __syncthreads();
    for (int64_t p0 = r0; p0 < r1; p0 += 16) {
        const bool more = p0 + 16 < r1;
        if (more) issue(p0 + 16);
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            const int pb = (s4 * 4 + kh) * RIDGE_CAT_LDS;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (live[q]) acc[q] = ridge_mma(Z[pb + offA[q]], Z[pb + offB[q]], acc[q]);
        }
        __syncthreads();
        if (more) { consume(); __syncthreads(); }
    }
    double* out = part + ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * (16 * 256);
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (live[q]) {
#pragma unroll
            for (int e = 0; e < 4; ++e) out[(wid + 4 * q) * 256 + e * 64 + lane] = acc[q][e];
        }
}

// G's tile t of panel pair blockIdx.x: the nb partials of each entry added in block order; both triangles are written
__global__ __launch_bounds__(256) void k_ridge_catgram_sum(const double* __restrict__ part, int nb, int r, int ldg, double* __restrict__ G) {
    const int tid = threadIdx.x, lane = tid & 63, e = tid >> 6;
    const int nt = (r + 15) / 16, npair = (int)gridDim.x, t = (int)blockIdx.y;
    int PI = 0, PJ = (int)blockIdx.x;
    while (PJ > PI) { PJ -= PI + 1; ++PI; }
    const int gI = PI * 4 + (t >> 2), gJ = PJ * 4 + (t & 3);
    if (gI >= nt || gJ >= nt || gI < gJ) return;                         // (uniform) the tiles k_ridge_catgram left out
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += part[((size_t)b * npair + blockIdx.x) * (16 * 256) + t * 256 + e * 64 + lane];
    const int i = gI * 16 + (lane >> 4) + 4 * e, j = gJ * 16 + (lane & 15);
    G[(size_t)i * ldg + j] = s;
    if (gI != gJ) G[(size_t)j * ldg + i] = s;
}

