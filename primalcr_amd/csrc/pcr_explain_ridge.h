// pcr_explain_ridge.h -- k_explain_ridge: a squared-loss row's scores decomposed over its own rated items (pcr_explain_ridge,
// pcr_explain_ridge_model of include/primalcr.h, "explaining squared-loss recommendations").  Part of
// pcr_fold.hip.  The build and the factorisation are pcr_ridge.h's workgroup functions (k_ridge_direct's and k_nnls_direct's),
// the masking is pcr_nnls.h's, the contributions run through stage 2 of k_explain (pcr_explain.h); the solve for the listed
// items is new.
//
// Per user with ratings r on rows I of F (n of them), A = F[I], mu = lambda n (weighted) or lambda, the free set P (every
// coordinate, or { t : u^_t > 0 } with nonneg), G = A_P^T A_P + mu I, u*_P = G^-1 A_P^T r, and for a listed item j
// z_j = G^-1 (v_j)_P (zero outside P):
//     e_p(j) = r_p (v_{i_p} . z_j),    sum_p e_p(j) = v_j . u*,    score(j) = v_j . u^,    residual(j) = v_j . (u^ - u*)
// One workgroup of 256 threads per user, one form for every (n, k):
//   1  ridge_gram builds G's lower-triangular tiles on v_mfma_f64_16x16x4_f64, the ratings streamed in 16s; nnls_mask_tiles
//      turns the rows and columns outside P into a unit diagonal; ridge_chol factors in place; ridge_trisolve gives u*.  Then
//      loss = |r - A u^|^2 (ridge_loss) and dist2 = |u^ - u*|^2.
//   2  the listed items in tiles of EXPLAIN_TILE: their rows widened to fp64 as the 16 columns of a right-hand side X in LDS, v_j . u^
//      and v_j . (u^ - u*) by four lanes per column, then ridge_solve16: L Y = X and L^T Z = Y by tile rows -- the 16 x 16
//      diagonal solve by one thread per column, the products of the off-diagonal tiles with the solved block on the matrix cores,
//      one tile per wave.
//   3  the user's ratings in chunks of EXPLAIN_CHUNK through block_dots (each row of F gathered once per tile, against the fp64
//      columns, scaled by r_p) and explain_merge (the rank-counting top-E and the support / opposition adders).
//   4  plain stores.
// A user without ratings or with an empty P forms no system (u* = 0, no contributor); a pivot that is <= 0 or not finite gives
// status SINGULAR with the same outputs.  Everything after an element of F or U is read is fp64.  Every sum has a fixed order that
// depends on (n, k, L) alone, every loop a static bound, nothing is exchanged between workgroups, no atomics.
#pragma once
#include "pcr_explain.h"
#include "pcr_nnls.h"
#include "pcr_ridge.h"

// a right-hand-side column in LDS: mp values and 2 of padding -- even, so that a column starts on 16 bytes, and 2 (mp + 2) = 4
// mod 32 dwords, so that the 16 columns an MFMA operand reads at one row offset sit on 16 different bank pairs
#define EXPLAIN_RIDGE_PAD 2

// LDS of k_explain_ridge: the small vectors, the two top-E images, the right-hand-side tile, one chunk's contributions (rows =
// min(longest user, EXPLAIN_CHUNK)), then ONE region for ridge_gram's staging chunk and the tiles of G.  Rank 112, 256 rows:
// 60 928 B of tiles + 14 592 B + 32 768 B + 6 144 B + 4 KB = 116 KB, one workgroup per CU.
static inline size_t explain_ridge_bytes(int mp, int block, int rows) {
    const int nt = mp / 16;
    const size_t stage = carve_bytes((size_t)16 * (mp + 1), 8), tiles = carve_bytes((size_t)(nt * (nt + 1) / 2) * RIDGE_TILE, 8);
    return carve_bytes(8, 8) + carve_bytes(block / 16, 8) + carve_bytes(16, 8) + carve_bytes(4, 8) + 4 * carve_bytes(mp, 8) +
           2 * carve_bytes(EXPLAIN_TILE, 8) + 2 * carve_bytes(EXPLAIN_TILE * 16, 8) + 2 * carve_bytes(EXPLAIN_TILE * 16, 4) +
           carve_bytes((size_t)EXPLAIN_TILE * (mp + EXPLAIN_RIDGE_PAD), 8) + carve_bytes((size_t)rows * EXPLAIN_TILE, 8) + std::max(stage, tiles);
}

// X := (L L^T)^-1 X for the EXPLAIN_TILE columns staged as xt[column * ldx + coordinate], with the factor ridge_chol left in Tl
// and dinv.  Forward by tile rows ib = 0 ..: the diagonal solve L_bb Y_b = X_b by one thread per column (the column's 16 values
// in registers), then X_i -= L_ib Y_b for every tile row below, one tile per wave on v_mfma_f64_16x16x4_f64; backward the same
// from the last tile row with the transposed tiles.  Every thread of the workgroup calls it; ends with a barrier.
template <int BLOCK>
__device__ __forceinline__ void ridge_solve16(const double* Tl, const double* dinv, double* xt, int ldx, int nt) {
    constexpr int NW = BLOCK / PCR_WAVE;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int row = lane & 15, kh = lane >> 4;                      // MFMA operand indices; the accumulator holds X[kh + 4 e][column row]
    for (int ib = 0; ib < nt; ++ib) {
        const double* D = Tl + (size_t)ridge_tix(ib, ib) * RIDGE_TILE;
        if (tid < EXPLAIN_TILE) {
            double* xc = xt + tid * ldx + ib * 16;
            double x[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) x[c] = xc[c];
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                double sacc = x[c];
#pragma unroll
                for (int j = 0; j < c; ++j) sacc -= x[j] * D[c * RIDGE_TP + j];
                x[c] = sacc * dinv[ib * 16 + c];
            }
#pragma unroll
            for (int c = 0; c < 16; ++c) xc[c] = x[c];
        }
        __syncthreads();
        for (int i = ib + 1 + wid; i < nt; i += NW) {
            const double* Li = Tl + (size_t)ridge_tix(i, ib) * RIDGE_TILE;
            double* xi = xt + row * ldx + i * 16 + kh;
            ridge_f64x4 c4;
#pragma unroll
            for (int e = 0; e < 4; ++e) c4[e] = xi[4 * e];
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) c4 = ridge_mma(-Li[row * RIDGE_TP + s4 * 4 + kh], xt[row * ldx + ib * 16 + s4 * 4 + kh], c4);
#pragma unroll
            for (int e = 0; e < 4; ++e) xi[4 * e] = c4[e];
        }
        __syncthreads();
    }
    for (int ib = nt - 1; ib >= 0; --ib) {
        const double* D = Tl + (size_t)ridge_tix(ib, ib) * RIDGE_TILE;
        if (tid < EXPLAIN_TILE) {
            double* xc = xt + tid * ldx + ib * 16;
            double x[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) x[c] = xc[c];
#pragma unroll
            for (int c = 15; c >= 0; --c) {
                double sacc = x[c];
#pragma unroll
                for (int j = c + 1; j < 16; ++j) sacc -= x[j] * D[j * RIDGE_TP + c];
                x[c] = sacc * dinv[ib * 16 + c];
            }
#pragma unroll
            for (int c = 0; c < 16; ++c) xc[c] = x[c];
        }
        __syncthreads();
        for (int i = wid; i < ib; i += NW) {
            const double* Lt = Tl + (size_t)ridge_tix(ib, i) * RIDGE_TILE;      // rows of tile row ib, columns of tile row i: read transposed
            double* xi = xt + row * ldx + i * 16 + kh;
            ridge_f64x4 c4;
#pragma unroll
            for (int e = 0; e < 4; ++e) c4[e] = xi[4 * e];
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) c4 = ridge_mma(-Lt[(s4 * 4 + kh) * RIDGE_TP + row], xt[row * ldx + ib * 16 + s4 * 4 + kh], c4);
#pragma unroll
            for (int e = 0; e < 4; ++e) xi[4 * e] = c4[e];
        }
        __syncthreads();
    }
}

// users: the launch's users (positions in the call); Um: their rows of U (row urow[u], NULL: row u; Um NULL: the minimiser itself
// is explained); mp: the rank padded to 16 (at most PCR_RIDGE_DIRECT_MAX); erows: rows of the contribution chunk
template <typename T, int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_explain_ridge(RidgeCsr X, Geo geo, const int32_t* __restrict__ users, int nusers, const T* __restrict__ F,
                                                         const T* __restrict__ Um, const int32_t* __restrict__ urow, double lambda, int weighted,
                                                         int nonneg, int mp, const int32_t* __restrict__ lists, int L, int E,
                                                         int32_t* __restrict__ expl_item, double* __restrict__ expl_contrib,
                                                         double* __restrict__ per_pair, double* __restrict__ per_user, int erows) {
    static_assert(BLOCK == 256, "ridge_gram's four-wave form covers every rank up to PCR_RIDGE_DIRECT_MAX");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    Carver cv(smem);
    double* red = cv.take<double>(8);
    double* part = cv.take<double>(BLOCK / 16);
    double* rch = cv.take<double>(16);                                   // the staged chunk's ratings
    unsigned long long* pm = cv.take<unsigned long long>(4);             // P: bits of coordinates 0..63, 64..127
    double* gv = cv.take<double>(mp);                                    // b masked to P, then u*
    double* dinv = cv.take<double>(mp);                                  // 1 / L[i][i]
    double* uh = cv.take<double>(mp);                                    // u^
    double* dv = cv.take<double>(mp);                                    // u^ - u*
    double* tile_u = cv.take<double>(EXPLAIN_TILE);                      // v_j . u^
    double* tile_d = cv.take<double>(EXPLAIN_TILE);                      // v_j . (u^ - u*)
    double* topv0 = cv.take<double>(EXPLAIN_TILE * 16);                  // running top-E per tile position, two images
    double* topv1 = cv.take<double>(EXPLAIN_TILE * 16);
    int32_t* topp0 = cv.take<int32_t>(EXPLAIN_TILE * 16);
    int32_t* topp1 = cv.take<int32_t>(EXPLAIN_TILE * 16);
    const int ldx = mp + EXPLAIN_RIDGE_PAD;
    double* xt = cv.take<double>((size_t)EXPLAIN_TILE * ldx);            // the listed items' columns: v_j, then z_j
    double* ebuf = cv.take<double>((size_t)erows * EXPLAIN_TILE);
    double* Tl = reinterpret_cast<double*>(cv.p);                        // ridge_gram's staging chunk, then the tiles of G over it
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int r = geo.r, ld = geo.ld, nt = mp / 16;

    for (int ui = blockIdx.x; ui < nusers; ui += gridDim.x) {
        const int u = users[ui];
        const int64_t s0 = X.uptr[u];
        const int n = (int)(X.uptr[u + 1] - s0);
        const double mu = weighted ? lambda * (double)n : lambda;
        const int32_t* uit = X.item + s0;
        const double* uval = X.val + s0;
        const T* urowp = Um ? Um + (size_t)(urow ? urow[u] : u) * ld : nullptr;
        // ---- u^ and the free set
        for (int t = tid; t < mp; t += BLOCK) uh[t] = (urowp && t < r) ? (double)urowp[t] : 0.0;
        if (wid == 0) {
            const int j0 = lane, j1 = lane + 64;
            const bool f0 = j0 < r && (!nonneg || (double)urowp[j0] > 0.0), f1 = j1 < r && (!nonneg || (double)urowp[j1] > 0.0);     // (nonneg: Um is given)
            const unsigned long long m0 = __ballot(f0), m1 = __ballot(f1);
            if (lane == 0) { pm[0] = m0; pm[1] = m1; }
        }
        __syncthreads();
        const unsigned long long p0 = pm[0], p1 = pm[1];
        auto in_p = [&](int j) { return (((j < 64 ? p0 : p1) >> (j & 63)) & 1ull) != 0ull; };
        const int np = __popcll(p0) + __popcll(p1);
        // ---- 1. G = A_P^T A_P + mu I, its factor and u*; without a system, or with a bad pivot, u* = 0
        bool solved = n > 0 && np > 0, bad = false;                      // (uniform)
        if (solved) {
            const double bacc = ridge_gram<T, BLOCK>(F, uit, uval, n, r, ld, r, mp, 0, mu, nullptr, rch, Tl);
            __syncthreads();
            if (nonneg) nnls_mask_tiles<BLOCK>(Tl, Tl, nt, p0, p1);
            for (int t = tid; t < mp; t += BLOCK) gv[t] = in_p(t) ? bacc : 0.0;               // (mp <= BLOCK: one pass)
            if (tid == 0) red[7] = 0.0;                                  // "not positive definite" flag
            __syncthreads();
            bad = ridge_chol<BLOCK>(Tl, dinv, red, nt);
            if (wid == 0 && !bad) {
                ridge_trisolve(Tl, dinv, gv, mp, nt);
                if (lane < mp && !in_p(lane)) gv[lane] = 0.0;
                if (lane + 64 < mp && !in_p(lane + 64)) gv[lane + 64] = 0.0;
            }
            __syncthreads();
            solved = !bad;
        }
        double d2 = 0.0;
        for (int t = tid; t < mp; t += BLOCK) {
            const double us = solved ? gv[t] : 0.0;
            if (!urowp) uh[t] = us;
            const double d = urowp ? uh[t] - us : 0.0;
            dv[t] = d;
            d2 += d * d;
        }
        __syncthreads();
        const double dist2 = block_sum<BLOCK>(d2, red);
        const double loss = ridge_loss<T, BLOCK>(F, uit, uval, n, uh, r, ld, part);
        if (tid == 0 && per_user) {
            double* o = per_user + (size_t)u * PCR_EXPLAIN_RIDGE_USER_FIELDS;
            o[0] = (double)n; o[1] = (double)np; o[2] = loss; o[3] = dist2; o[4] = (double)(bad ? PCR_RIDGE_SINGULAR : PCR_RIDGE_OK);
        }
        // ---- the listed items: non-padding entries first
        const int32_t* lst = lists + (size_t)u * L;
        int Lu = 0;
        for (int l = tid; l < L; l += BLOCK) Lu += lst[l] >= 0 ? 1 : 0;
        Lu = (int)block_sum<BLOCK>((double)Lu, red);
        const int nc = solved ? n : 0;                                   // the ratings that contribute
        for (int l0 = 0; l0 < Lu; l0 += EXPLAIN_TILE) {
            const int tl = min(EXPLAIN_TILE, Lu - l0);
            __syncthreads();
            // ---- 2. the tile's rows of F as fp64 columns (zero beyond the rank and beyond the tile), their two dots, the solve
            for (int x = tid; x < EXPLAIN_TILE * mp; x += BLOCK) {
                const int jj = x / mp, c = x - jj * mp;
                xt[jj * ldx + c] = (jj < tl && c < r) ? (double)F[(size_t)lst[l0 + jj] * ld + c] : 0.0;
            }
            __syncthreads();
            if (tid < 64) {                                              // four lanes per tile position
                const int jj = tid >> 2, q = tid & 3;
                double a = 0.0, b = 0.0;
                for (int t = q; t < r; t += 4) { const double v = xt[jj * ldx + t]; a += v * uh[t]; b += v * dv[t]; }
                a += lane_xor2(a); b += lane_xor2(b);
                a += lane_xor1(a); b += lane_xor1(b);
                if (q == 0) { tile_u[jj] = a; tile_d[jj] = b; }
            }
            __syncthreads();
            if (nc > 0) {
                if (nonneg) {
                    for (int x = tid; x < EXPLAIN_TILE * mp; x += BLOCK) {
                        const int jj = x / mp, c = x - jj * mp;
                        if (!in_p(c)) xt[jj * ldx + c] = 0.0;
                    }
                    __syncthreads();
                }
                ridge_solve16<BLOCK>(Tl, dinv, xt, ldx, nt);
            }
            // ---- 3. e_p(j) = r_p (v_{i_p} . z_j), a chunk of ratings at a time
            double sup = 0.0, opp = 0.0;                                 // of tile position tid (tid < tl)
            ExplainTop top = {topv0, topv1, topp0, topp1, 0};
            for (int c0 = 0; c0 < nc; c0 += EXPLAIN_CHUNK) {
                const int c1 = min(nc, c0 + EXPLAIN_CHUNK);
                __syncthreads();
                block_dots<T, BLOCK>(F, uit, [&](int p) { return uval[p]; }, c0, c1, xt, ldx, ebuf, geo);
                __syncthreads();
                explain_merge<BLOCK>(ebuf, c0, c1 - c0, tl, E, top, sup, opp);
            }
            __syncthreads();
            // ---- 4. stores
            explain_store_top<BLOCK>(top, uit, tl, E, expl_item + ((size_t)u * L + l0) * E, expl_contrib + ((size_t)u * L + l0) * E);
            if (tid < tl && per_pair) {
                double* o = per_pair + ((size_t)u * L + l0 + tid) * PCR_EXPLAIN_PAIR_FIELDS;
                o[0] = tile_u[tid]; o[1] = sup; o[2] = opp; o[3] = urowp ? tile_d[tid] : 0.0;
            }
        }
        explain_store_padding<BLOCK>(Lu, L, E, expl_item + (size_t)u * L * E, expl_contrib + (size_t)u * L * E,
                                     per_pair ? per_pair + (size_t)u * L * PCR_EXPLAIN_PAIR_FIELDS : nullptr);
        __syncthreads();
    }
}
