// pcr_nnls.h -- k_nnls_direct, k_nnls_cg: non-negative fold-in against a fixed factor matrix F (pcr_fold_in_nnls,
// pcr_fold_in_nnls_model of include/primalcr.h).  Part of pcr_fold.hip.
//
// Per user with ratings r on rows I of F (n of them), A = F[I], mu = lambda n (weighted) or lambda, G = A^T A + mu I, b = A^T r:
//     minimise |r - A u|^2 + mu |u|^2  subject to u >= 0
// by block principal pivoting (the Kim-Park rule, spelled out in include/primalcr.h): the passive set P starts as every
// coordinate, each pivot solves G_PP u_P = b_P exactly, takes y = G u - b on the complement Z, and exchanges the violators
// V = { j in P : u_j < 0 } + { j in Z : y_j < 0 } -- all of them while |V| keeps shrinking (and three more times), else the largest
// one.  One user per workgroup, in one of two forms chosen by the rank alone (pcr_nnls_form, pcr_host.cpp):
//   DIRECT  G's lower-triangular tiles are built ONCE by pcr_ridge.h's ridge_gram (the primal build of k_ridge_direct) and stay in
//           LDS as a master copy that is never factored; every pivot copies them into a working set with the rows and columns of
//           Z replaced by a unit diagonal (what the build already does beyond the rank), runs ridge_chol and ridge_trisolve on b
//           masked to P, and reads y off the master (entry (i, j) with i < j from the transposed tile).  The rule runs on wave 0:
//           P is one bit per coordinate (lane l holds coordinates l and l + 64), |V| and max V come from two ballots.
//   CG      the solve on P is pcr_ridge.h's ridge_cg_solve with the search direction masked to P; one more pass of
//           ridge_cg_apply gives y.  P is one LDS word per coordinate, |V| and max V are workgroup reductions.
// fp64 from the moment an element of F is read; the row is rounded to T on store (rounding keeps >= 0) and loss / obj are taken at
// the rounded row by ridge_finish.  No atomics, nothing is exchanged between workgroups, every loop has a static bound; a user's
// bits depend on its ratings, F and the parameters alone.
#pragma once
#include "pcr_ridge.h"

// the end of a user, both forms: ridge_finish (the row, loss and obj at the rounded row) into an LDS line, then the table line of
// PCR_NNLS_FIELDS with the count of coordinates at 0.  uvec: the row in LDS (>= 0; status SINGULAR: ignored); ot: LDS, 8 doubles.
template <typename T, int BLOCK>
__device__ __forceinline__ void nnls_finish(const T* __restrict__ F, const int32_t* __restrict__ item, const double* __restrict__ val, int n, double* uvec,
                                            int r, int ld, double mu, int form, int pivots, int status, T* __restrict__ urow, double* __restrict__ o,
                                            double* ot, double* part, double* red) {
    ridge_finish<T, BLOCK>(F, item, val, n, uvec, r, ld, mu, form, pivots, status, urow, ot, part, red);      // (PCR_NNLS_SINGULAR == PCR_RIDGE_SINGULAR)
    double z = 0.0;
    for (int t = threadIdx.x; t < r; t += BLOCK) z += uvec[t] == 0.0 ? 1.0 : 0.0;          // (ridge_finish left the rounded row in uvec)
    z = block_sum<BLOCK>(z, red);
    if (threadIdx.x == 0) {
        o[0] = ot[0]; o[1] = ot[1]; o[2] = ot[2]; o[3] = z; o[4] = ot[3]; o[5] = ot[4]; o[6] = ot[5];
    }
    __syncthreads();
}

// a user without ratings: a zero row, status OK, 0 pivots
template <typename T, int BLOCK>
__device__ __forceinline__ void nnls_empty(int r, int ld, int form, T* __restrict__ urow, double* __restrict__ o) {
    for (int t = threadIdx.x; t < ld; t += BLOCK) urow[t] = (T)0;
    if (threadIdx.x == 0) { o[0] = 0.0; o[1] = (double)form; o[2] = 0.0; o[3] = (double)r; o[4] = 0.0; o[5] = 0.0; o[6] = (double)PCR_NNLS_OK; }
}

// the rule's step on the count nv > 0 and the largest member of V: true = exchange all of V, false = the largest alone
__device__ __forceinline__ bool nnls_rule(int nv, int& alpha, int& beta) {
    if (nv < beta) { beta = nv; alpha = 3; return true; }
    if (alpha > 0) { alpha -= 1; return true; }
    return false;
}

// dst = the nt x nt lower-triangular tiles src with the rows and columns outside P (bit j & 63 of p0 / p1 for coordinate j < 64 /
// >= 64) replaced by a unit diagonal -- what ridge_gram already leaves beyond the rank, and what ridge_chol passes through
// unchanged.  dst may be src.  k_nnls_direct's pivots and k_explain_ridge's free set (pcr_explain_ridge.h) run this one.
template <int BLOCK>
__device__ __forceinline__ void nnls_mask_tiles(const double* src, double* dst, int nt, unsigned long long p0, unsigned long long p1) {
    constexpr int NW = BLOCK / PCR_WAVE;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, npairs = nt * (nt + 1) / 2;
    auto in_p = [&](int j) { return (((j < 64 ? p0 : p1) >> (j & 63)) & 1ull) != 0ull; };
    for (int pr = wid; pr < npairs; pr += NW) {
        int I = 0, rem = pr;
        while (rem > I) { rem -= I + 1; ++I; }
        const double* s = src + (size_t)ridge_tix(I, rem) * RIDGE_TILE;
        double* d = dst + (size_t)ridge_tix(I, rem) * RIDGE_TILE;
        const int cl = lane & 15, col = rem * 16 + cl;
        const bool pc = in_p(col);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int rl = (lane >> 4) + 4 * e, rw = I * 16 + rl;
            d[rl * RIDGE_TP + cl] = (pc && in_p(rw)) ? s[rl * RIDGE_TP + cl] : (rw == col ? 1.0 : 0.0);
        }
    }
}

// LDS of k_nnls_direct: the small vectors, then the master tiles of G (the staging chunk of the build lies under them, as in
// k_ridge_direct) and the working tiles of a pivot.  7 x 7 tiles: 2 x 60 928 B + 5 KB = 124 KB, one workgroup per CU.
static inline size_t nnls_direct_bytes(int mp, int ld, int block) {
    const int nt = mp / 16;
    const size_t stage = carve_bytes((size_t)16 * (mp + 1), 8), tiles = carve_bytes((size_t)(nt * (nt + 1) / 2) * RIDGE_TILE, 8);
    return carve_bytes(8, 8) + carve_bytes(block / 16, 8) + carve_bytes(16, 8) + carve_bytes(8, 8) + carve_bytes(4, 8) + 4 * carve_bytes(mp, 8) +
           carve_bytes(std::max(mp, ld), 8) + std::max(stage, tiles) + tiles;
}

// mp: the rank padded to 16 (BLOCK = 64: at most 64, BLOCK = 256: at most 112)
template <typename T, int BLOCK>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(2))) void k_nnls_direct(RidgeCsr X, const int32_t* __restrict__ users, int nusers, const T* __restrict__ F, int r, int ld,
                                                       T* __restrict__ Uout, double* __restrict__ per_user, double lambda, int weighted, int mp) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    Carver cv(smem);
    double* red = cv.take<double>(8);
    double* part = cv.take<double>(BLOCK / 16);
    double* rch = cv.take<double>(16);                                   // the staged chunk's ratings
    double* ot = cv.take<double>(8);                                    // ridge_finish's table line
    unsigned long long* pm = cv.take<unsigned long long>(4);             // P: bits of coordinates 0..63, 64..127; [2] != 0: V was empty
    double* gv = cv.take<double>(mp);                                    // b masked to P, then the pivot's solution
    double* dinv = cv.take<double>(mp);                                  // 1 / L[i][i]
    double* bv = cv.take<double>(mp);                                    // b = A^T r
    double* yv = cv.take<double>(mp);                                    // y = G u - b
    double* uvec = cv.take<double>(mp > ld ? mp : ld);
    const int nt = mp / 16, npairs = nt * (nt + 1) / 2;
    const size_t stage = ((size_t)16 * (mp + 1) * 8 + 15) & ~(size_t)15, tiles = ((size_t)npairs * RIDGE_TILE * 8 + 15) & ~(size_t)15;
    double* Gm = reinterpret_cast<double*>(cv.p);                        // the staging chunk, then the master tiles of G over it
    double* Tw = reinterpret_cast<double*>(cv.p + (stage > tiles ? stage : tiles));      // a pivot's working tiles
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;

    for (int ui = blockIdx.x; ui < nusers; ui += gridDim.x) {
        const int u = users[ui];
        const int64_t s0 = X.uptr[u];
        const int n = (int)(X.uptr[u + 1] - s0);
        const double mu = weighted ? lambda * (double)n : lambda;
        const int32_t* uit = X.item + s0;
        const double* uval = X.val + s0;
        T* urow = Uout + (size_t)u * ld;
        double* o = per_user + (size_t)u * PCR_NNLS_FIELDS;
        if (n == 0) { nnls_empty<T, BLOCK>(r, ld, PCR_NNLS_DIRECT, urow, o); continue; }       // (uniform)
        __syncthreads();
        // ---- G's tiles (the master copy) and b, once
        const double bacc = ridge_gram<T, BLOCK>(F, uit, uval, n, r, ld, r, mp, 0, mu, nullptr, rch, Gm);
        for (int t = tid; t < mp; t += BLOCK) bv[t] = t < r ? bacc : 0.0;                      // (mp <= BLOCK: one pass)
        if (tid == 0) {
            pm[0] = r >= 64 ? ~0ull : (1ull << r) - 1ull;
            pm[1] = r > 64 ? (1ull << (r - 64)) - 1ull : 0ull;
        }
        __syncthreads();
        int pivots = 0, status = PCR_NNLS_CAP, alpha = 3, beta = r + 1;                         // (alpha, beta: wave 0's)
        unsigned long long p0 = 0ull, p1 = 0ull;                                                // P of the latest solve
        for (int pv = 0; pv < PCR_NNLS_PIVOT_CAP; ++pv) {
            p0 = pm[0]; p1 = pm[1];
            auto in_p = [&](int j) { return (((j < 64 ? p0 : p1) >> (j & 63)) & 1ull) != 0ull; };
            // ---- the working tiles: the master with Z's rows and columns as a unit diagonal; b masked to P
            nnls_mask_tiles<BLOCK>(Gm, Tw, nt, p0, p1);
            for (int t = tid; t < mp; t += BLOCK) gv[t] = in_p(t) ? bv[t] : 0.0;
            if (tid == 0) red[7] = 0.0;                                  // "not positive definite" flag
            __syncthreads();
            // ---- u_P = G_PP^-1 b_P, u_Z = 0
            if (ridge_chol<BLOCK>(Tw, dinv, red, nt)) { status = PCR_NNLS_SINGULAR; break; }   // (uniform)
            if (wid == 0) {
                ridge_trisolve(Tw, dinv, gv, mp, nt);
                if (lane < mp && !in_p(lane)) gv[lane] = 0.0;
                if (lane + 64 < mp && !in_p(lane + 64)) gv[lane + 64] = 0.0;
            }
            __syncthreads();
            ++pivots;
            // ---- y = G u - b on Z, one thread per coordinate, the columns in order
            for (int t = tid; t < mp; t += BLOCK) {
                double s = 0.0;
                if (t < r && !in_p(t)) {
                    const int I = t >> 4, tr = t & 15;
                    for (int J = 0; J < nt; ++J) {
                        const double* tile = J <= I ? Gm + (size_t)ridge_tix(I, J) * RIDGE_TILE + tr * RIDGE_TP : Gm + (size_t)ridge_tix(J, I) * RIDGE_TILE + tr;
                        const int st = J <= I ? 1 : RIDGE_TP;
#pragma unroll
                        for (int c = 0; c < 16; ++c) s += tile[c * st] * gv[J * 16 + c];
                    }
                    s -= bv[t];
                }
                yv[t] = s;
            }
            __syncthreads();
            // ---- the rule, on wave 0
            if (wid == 0) {
                const int j0 = lane, j1 = lane + 64;
                const bool v0 = j0 < r && (in_p(j0) ? gv[j0] < 0.0 : yv[j0] < 0.0);
                const bool v1 = j1 < r && (in_p(j1) ? gv[j1] < 0.0 : yv[j1] < 0.0);
                unsigned long long m0 = __ballot(v0), m1 = __ballot(v1);
                const int nv = __popcll(m0) + __popcll(m1);
                if (nv > 0 && !nnls_rule(nv, alpha, beta)) {             // the largest violator alone
                    if (m1 != 0ull) { m1 = 1ull << (63 - __clzll((long long)m1)); m0 = 0ull; }
                    else m0 = 1ull << (63 - __clzll((long long)m0));
                }
                if (lane == 0) { pm[0] = p0 ^ m0; pm[1] = p1 ^ m1; pm[2] = nv == 0 ? 1ull : 0ull; }
            }
            __syncthreads();
            if (pm[2] != 0ull) { status = PCR_NNLS_OK; break; }          // (uniform: read behind the barrier)
        }
        // ---- the row: the latest solve on its P, a negative entry (PCR_NNLS_CAP alone has any) as 0
        if (status != PCR_NNLS_SINGULAR)
            for (int t = tid; t < r; t += BLOCK) uvec[t] = gv[t] > 0.0 ? gv[t] : 0.0;
        __syncthreads();
        nnls_finish<T, BLOCK>(F, uit, uval, n, uvec, r, ld, mu, PCR_NNLS_DIRECT, pivots, status, urow, o, ot, part, red);
    }
}

static inline size_t nnls_cg_bytes(int ld) {
    return carve_bytes(8, 8) + carve_bytes(16, 8) + carve_bytes(8, 8) + carve_bytes(8, 4) + 5 * carve_bytes(ld, 8) + carve_bytes(ld, 4) +
           carve_bytes(RIDGE_CG_CHUNK, 8) + carve_bytes(RIDGE_CG_CHUNK, 4);
}

// 256 threads per user, any n and k
template <typename T>
__global__ __launch_bounds__(256) void k_nnls_cg(RidgeCsr X, const int32_t* __restrict__ users, int nusers, const T* __restrict__ F, int r, int ld,
                                                 T* __restrict__ Uout, double* __restrict__ per_user, double lambda, int weighted) {
    constexpr int BLOCK = 256, CH = RIDGE_CG_CHUNK;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    Carver cv(smem);
    double* red = cv.take<double>(8);
    double* part = cv.take<double>(16);
    double* ot = cv.take<double>(8);
    int* ired = cv.take<int>(8);                                         // the waves' largest violators
    double* uvec = cv.take<double>(ld);
    double* res = cv.take<double>(ld);
    double* pv = cv.take<double>(ld);
    double* Hp = cv.take<double>(ld);                                    // the CG's H p, then G u and y
    double* bv = cv.take<double>(ld);                                    // b = A^T r
    int32_t* pas = cv.take<int32_t>(ld);                                 // P: 1 = passive
    double* sc = cv.take<double>(CH);
    int32_t* itc = cv.take<int32_t>(CH);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;

    for (int ui = blockIdx.x; ui < nusers; ui += gridDim.x) {
        const int u = users[ui];
        const int64_t s0 = X.uptr[u];
        const int n = (int)(X.uptr[u + 1] - s0);
        const double mu = weighted ? lambda * (double)n : lambda;
        const int32_t* uit = X.item + s0;
        const double* uval = X.val + s0;
        T* urow = Uout + (size_t)u * ld;
        double* o = per_user + (size_t)u * PCR_NNLS_FIELDS;
        if (n == 0) { nnls_empty<T, BLOCK>(r, ld, PCR_NNLS_CG, urow, o); continue; }           // (uniform)
        for (int t = tid; t < r; t += BLOCK) { bv[t] = 0.0; pas[t] = 1; uvec[t] = 0.0; }
        __syncthreads();
        ridge_cg_apply<T>(F, uit, uval, n, r, ld, nullptr, bv, sc, itc);                       // b = A^T r
        int pivots = 0, status = PCR_NNLS_CAP, alpha = 3, beta = r + 1;                         // (uniform: every thread runs the rule)
        for (int pvt = 0; pvt < PCR_NNLS_PIVOT_CAP; ++pvt) {
            // ---- u_P = G_PP^-1 b_P by the masked CG from u = 0, u_Z = 0
            double c = 0.0;
            for (int t = tid; t < r; t += BLOCK) { uvec[t] = 0.0; res[t] = pas[t] ? bv[t] : 0.0; c += pas[t] ? 1.0 : 0.0; }
            const int npas = (int)block_sum<BLOCK>(c, red);
            __syncthreads();
            int iters = 0;
            const int cs = ridge_cg_solve<T>(F, uit, uval, n, r, ld, mu, pas, npas, uvec, res, pv, Hp, sc, itc, red, &iters);
            ++pivots;
            if (cs == PCR_RIDGE_SINGULAR) { status = PCR_NNLS_SINGULAR; break; }               // (uniform)
            if (cs == PCR_RIDGE_CG_CAP) break;                                                  // the user's status is PCR_NNLS_CAP
            // ---- y = G u - b: one more pass
            for (int t = tid; t < r; t += BLOCK) Hp[t] = mu * uvec[t];
            __syncthreads();
            ridge_cg_apply<T>(F, uit, uval, n, r, ld, uvec, Hp, sc, itc);
            // ---- the rule: |V| and max V over the workgroup
            auto viol = [&](int t) { return pas[t] ? uvec[t] < 0.0 : Hp[t] - bv[t] < 0.0; };
            double cnt = 0.0;
            int top = -1;
            for (int t = tid; t < r; t += BLOCK) if (viol(t)) { cnt += 1.0; top = t; }
            const int nv = (int)block_sum<BLOCK>(cnt, red);
            if (nv == 0) { status = PCR_NNLS_OK; break; }                                       // (uniform)
            top = max(top, lane_xor_i<32>(top)); top = max(top, lane_xor_i<16>(top)); top = max(top, lane_xor_i<8>(top));
            top = max(top, lane_xor_i<4>(top)); top = max(top, lane_xor_i<2>(top)); top = max(top, lane_xor_i<1>(top));
            if (lane == 0) ired[wid] = top;                              // (last read before the barrier that ends a pivot)
            __syncthreads();
            top = max(max(ired[0], ired[1]), max(ired[2], ired[3]));
            const bool all = nnls_rule(nv, alpha, beta);
            for (int t = tid; t < r; t += BLOCK) if (all ? viol(t) : t == top) pas[t] ^= 1;     // (a thread reads and writes its own t alone)
            __syncthreads();
        }
        // ---- the row: the latest solve (zero outside its P), a negative entry (PCR_NNLS_CAP alone has any) as 0
        __syncthreads();
        for (int t = tid; t < r; t += BLOCK) uvec[t] = uvec[t] > 0.0 ? uvec[t] : 0.0;
        __syncthreads();
        nnls_finish<T, BLOCK>(F, uit, uval, n, uvec, r, ld, mu, PCR_NNLS_CG, pivots, status, urow, o, ot, part, red);
    }
}
