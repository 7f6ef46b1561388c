// pcr_explain.h -- k_explain: a user's scores decomposed over its own rated items (pcr_explain, pcr_explain_model of
// include/primalcr.h, "explaining recommendations").  Part of pcr_fold.hip; the state evaluation is k_foldin's (pcr_foldin.h,
// steps 1-2 of a fold-in step), the rest is new.
//
// A row u of U trained on the ratings I has the gradient g = lambda_u u + sum_{p in I} c_p v_{i_p}, c_p the sweep coefficients of
// obtain_g_u_new (pcrpp.cpp:493-539).  So for ANY item j
//     v_j . u = sum_p e_p(j) + rho(j),    e_p(j) = -(c_p / lambda_u) (v_{i_p} . v_j),    rho(j) = (v_j . g) / lambda_u
// exactly: one signed contribution per rated item and a residual that vanishes at a stationary row.
//
// One workgroup per user, three forms by the user's length as k_foldin's.  Per user:
//   1  m = V_I u in T (block_sddmm: the bits k_foldin has), the (level, m) sort, the loss (block_objective), the fp64 prefix sums
//      and the sweep into c[] (fp64, CSR order, NOT rounded to T); g in fp64 by block_gradient -- its own fixed order.
//   2  the listed items in tiles of EXPLAIN_TILE: their rows of V staged in LDS with v_j . u and v_j . g; the user's ratings in
//      chunks of EXPLAIN_CHUNK: block_dots gathers every row ONCE per tile from L2 and dots it against the staged rows in fp64
//      into ebuf[chunk position][tile position]; the chunk is merged into the running top-E of every tile position by rank
//      counting under the strict total order (e descending, position ascending) -- ranks are distinct, so every slot has one
//      writer: no atomics, and the result does not depend on arrival order; support / opposition are added by one thread per
//      tile position in ascending row position.
//   3  plain stores.  e_p(j) is never materialised beyond one chunk x one tile.
// Every loop has a static bound, nothing is exchanged between workgroups, no atomics.
// Stage 2's pieces -- block_dots, explain_merge, explain_store_top, explain_store_padding -- are workgroup functions:
// k_explain_ridge (pcr_explain_ridge.h) runs the same ones on its fp64 columns.
#pragma once
#include <type_traits>

#include "pcr_foldin.h"
#include "pcr_host.h"
#include "pcr_prims.h"

#define EXPLAIN_TILE 16
#define EXPLAIN_CHUNK 256
static_assert(EXPLAIN_TILE == 16 && PCR_EXPLAIN_MAX_E <= 16, "block_dots reduces two sets of 8 tile positions; a top-E row has 16 slots");

// The LDS of one user's explanation besides the per-rating arrays: u in T, red, u and g in fp64, block_gradient's partial rows, the
// tile (rows of V, v.u, v.g), one chunk's contributions (rows = min(longest user, EXPLAIN_CHUNK)) and the two top-E images
static inline size_t explain_small_bytes(int ld, int block, size_t elt, int rows) {
    return carve_bytes(ld, elt) + carve_bytes(block / PCR_WAVE + 1, 8) + 2 * carve_bytes(ld, 8) + carve_bytes((size_t)block * (16 / elt), 8) +
           carve_bytes((size_t)EXPLAIN_TILE * ld, elt) + 2 * carve_bytes(EXPLAIN_TILE, 8) +
           carve_bytes((size_t)rows * EXPLAIN_TILE, 8) + 2 * carve_bytes(EXPLAIN_TILE * 16, 8) + 2 * carve_bytes(EXPLAIN_TILE * 16, 4);
}
// the per-rating arrays of a user of at most cap ratings and rs_cap - 1 levels (LDS, or one workgroup's slice of the scratch)
static inline size_t explain_arr_bytes(int cap, int rs_cap, size_t elt, size_t li_bytes) {
    return carve_bytes(cap, elt) + carve_bytes(cap, li_bytes) + carve_bytes(cap, 4) + carve_bytes(cap, 2) + carve_bytes((size_t)cap + 1, 8) +
           carve_bytes(cap, 8) + carve_bytes(rs_cap, 4);
}

// gvec[0, ld) = lam * uvec + sum_{p < n} c[p] M[rows[p]] in fp64.  A thread owns one 16-byte chunk of the row and one of nsl
// slices of the ratings (p = s, s + nsl, ...: ascending inside a slice); the slices are then added in ascending s.  The order
// is a function of n, ld and BLOCK alone.  wbuf: LDS, BLOCK * VEC doubles.  Ends with a barrier.
template <typename T, int BLOCK>
__device__ __forceinline__ void block_gradient(const T* __restrict__ M, const int32_t* rows, const double* c, int n, double lam,
                                               const double* uvec, double* gvec, double* wbuf, const Geo& geo) {
    typedef typename VecOf<T>::type V;
    constexpr int VEC = VecOf<T>::N;
    const int tid = threadIdx.x;
    const int nsl = geo.nchunk >= BLOCK ? 1 : BLOCK / geo.nchunk;
    const int cpp = nsl == 1 ? BLOCK : geo.nchunk;                 // chunks per pass
    const int s = tid / cpp, cl = tid - s * cpp;
    for (int c0 = 0; c0 < geo.nchunk; c0 += cpp) {
        const int ch = c0 + cl;
        if (s < nsl && ch < geo.nchunk) {
            double acc[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[e] = 0.0;
#pragma unroll 4
            for (int p = s; p < n; p += nsl) {
                const V rv = *reinterpret_cast<const V*>(M + row_off(rows[p], geo) + ch * VEC);
                const double cp = c[p];
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc[e] += cp * (double)velem(rv, e);
            }
#pragma unroll
            for (int e = 0; e < VEC; ++e) wbuf[(s * cpp + cl) * VEC + e] = acc[e];
        }
        __syncthreads();
        const int cols = min(cpp, geo.nchunk - c0) * VEC;
        for (int t = tid; t < cols; t += BLOCK) {
            double sum = 0.0;
            for (int q = 0; q < nsl; ++q) sum += wbuf[q * cpp * VEC + t];
            gvec[c0 * VEC + t] = lam * uvec[c0 * VEC + t] + sum;
        }
        __syncthreads();
    }
}

// ebuf[(p - p0) * EXPLAIN_TILE + jj] = scale(p) * (M[rows[p]] . tile[jj]) in fp64 for p in [p0, p1), jj < EXPLAIN_TILE (k_explain:
// scale(p) = -(c[p] / lam); k_explain_ridge: the rating r_p).  G lanes per row as block_sddmm: a lane loads ITS 16-byte chunk of
// the row once (global_load_dwordx4) and meets the same columns of the 16 staged rows (ds_read_b128: the G lanes of a group read
// consecutive slots, the other groups of the wave the same addresses -- a broadcast, no bank conflict); a wide row's next chunk is
// in flight meanwhile.  The 16 partial dots are summed over the group by two group_reduce8 (G >= 8) or butterflies.  tile: LDS,
// EXPLAIN_TILE rows of tld values of TT -- the storage type T (rows of the factor as they are) or double (k_explain_ridge's solved
// columns; tld even); at least geo.ld of them per row are read.  rows and what scale reads may be LDS or global.
template <typename TT, int VEC>
__device__ __forceinline__ void tile_chunk(const TT* p, double (&out)[VEC]) {
    typedef TT nat __attribute__((ext_vector_type(16 / sizeof(TT))));
    constexpr int PER = 16 / sizeof(TT);
#pragma unroll
    for (int h = 0; h < VEC / PER; ++h) {
        const nat v = *((const PCR_LDS nat*)p + h);
#pragma unroll
        for (int e = 0; e < PER; ++e) out[h * PER + e] = (double)v[e];
    }
}
template <typename T, int BLOCK, typename TT, class Scale>
__device__ __forceinline__ void block_dots(const T* __restrict__ M, const int32_t* rows, Scale scale_of, int p0, int p1, const TT* tile, int tld,
                                           double* ebuf, const Geo& geo) {
    typedef typename VecOf<T>::type V;
    constexpr int VEC = VecOf<T>::N;
    const int G = geo.G, g = threadIdx.x & (G - 1), grp = threadIdx.x / G, ngrp = BLOCK / G;
    const int npass = (geo.nchunk + G - 1) / G;
    const int rho = 4 * (g & 1) + (g & 2) + ((g >> 2) & 1);
    for (int row = p0 + grp; row < p1; row += ngrp) {
        double pa[8], pb[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) { pa[q] = 0.0; pb[q] = 0.0; }
        const T* src = M + row_off(rows[row], geo);
        V cur = {};
        if (g < geo.nchunk) cur = *reinterpret_cast<const V*>(src + g * VEC);
        for (int k = 0; k < npass; ++k) {
            const int ch = g + k * G;
            const bool act = ch < geo.nchunk;
            V nxt = cur;
            if (k + 1 < npass && ch + G < geo.nchunk) nxt = *reinterpret_cast<const V*>(src + (ch + G) * VEC);
            if (act) {
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    double ta[VEC], tb[VEC];
                    tile_chunk<TT, VEC>(tile + q * tld + ch * VEC, ta);
                    tile_chunk<TT, VEC>(tile + (q + 8) * tld + ch * VEC, tb);
#pragma unroll
                    for (int e = 0; e < VEC; ++e) {
                        pa[q] += (double)velem(cur, e) * ta[e];
                        pb[q] += (double)velem(cur, e) * tb[e];
                    }
                }
            }
            cur = nxt;
        }
        const double scale = scale_of(row);
        double* out = ebuf + (size_t)(row - p0) * EXPLAIN_TILE;
        if (G >= 8) {                                             // whole lane groups are active here
            const double ta = group_reduce8<double>(pa, g, G), tb = group_reduce8<double>(pb, g, G);
            if (g < 8) { out[rho] = scale * ta; out[8 + rho] = scale * tb; }
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                double a = pa[q], b = pb[q];
                if (G > 2) { a += lane_xor2(a); b += lane_xor2(b); }
                if (G > 1) { a += lane_xor1(a); b += lane_xor1(b); }
                if (g == 0) { out[q] = scale * a; out[8 + q] = scale * b; }
            }
        }
    }
}

// (e, position) a precedes b in a contributor list: e descending, equal e by ascending position
__device__ __forceinline__ bool explain_before(double ea, int pa, double eb, int pb) { return ea > eb || (ea == eb && pa < pb); }

// The running top-E of the EXPLAIN_TILE tile positions: two images of 16 slots per position (values, row positions), the
// current one first, and the entries it holds
struct ExplainTop {
    double *tv, *tvn;
    int32_t *tp, *tpn;
    int have;
};
// One chunk of contributions ebuf[cn][EXPLAIN_TILE] (row positions p0 ...) into the running top-E of tile positions < tl, and
// into the support / opposition of tile position threadIdx.x (< tl).  Rank counting: the chunk's entries and the running ones
// are the candidates of every tile position; ranks under explain_before are distinct, so every slot of the other image has one
// writer.  The caller's barrier stands before (ebuf complete) and after (the images swapped).
template <int BLOCK>
__device__ __forceinline__ void explain_merge(const double* ebuf, int p0, int cn, int tl, int E, ExplainTop& top, double& sup, double& opp) {
    const int tid = threadIdx.x, have = top.have;
    const double* tv = top.tv;
    const int32_t* tp = top.tp;
    for (int x = tid; x < (cn + have) * EXPLAIN_TILE; x += BLOCK) {
        const int cand = x / EXPLAIN_TILE, jj = x - cand * EXPLAIN_TILE;
        if (jj >= tl) continue;
        const bool fresh = cand < cn;
        const double e = fresh ? ebuf[cand * EXPLAIN_TILE + jj] : tv[jj * 16 + cand - cn];
        const int pos = fresh ? p0 + cand : tp[jj * 16 + cand - cn];
        int rank = 0;
        for (int q = 0; q < have && rank < E; ++q) rank += explain_before(tv[jj * 16 + q], tp[jj * 16 + q], e, pos) ? 1 : 0;
        for (int q = 0; q < cn && rank < E; ++q) rank += explain_before(ebuf[q * EXPLAIN_TILE + jj], p0 + q, e, pos) ? 1 : 0;
        if (rank < E) { top.tvn[jj * 16 + rank] = e; top.tpn[jj * 16 + rank] = pos; }
    }
    if (tid < tl) {
        for (int q = 0; q < cn; ++q) {
            const double e = ebuf[q * EXPLAIN_TILE + tid];
            if (e > 0.0) sup += e; else if (e < 0.0) opp += e;
        }
    }
    top.have = min(E, have + cn);
    { double* a = top.tv; top.tv = top.tvn; top.tvn = a; int32_t* b = top.tp; top.tp = top.tpn; top.tpn = b; }
}
// the finished top-E of tile positions < tl to out_item / out_contrib [tl][E] (itm: the row's items, LDS or global); (-1, 0.0)
// beyond the entries held
template <int BLOCK>
__device__ __forceinline__ void explain_store_top(const ExplainTop& top, const int32_t* itm, int tl, int E, int32_t* __restrict__ out_item,
                                                  double* __restrict__ out_contrib) {
    for (int x = threadIdx.x; x < tl * E; x += BLOCK) {
        const int jj = x / E, r = x - jj * E;
        const bool ok = r < top.have;
        out_item[x] = ok ? itm[top.tp[jj * 16 + r]] : -1;
        out_contrib[x] = ok ? top.tv[jj * 16 + r] : 0.0;
    }
}
// list positions [Lu, L) of a user are padding: (-1, 0.0) contributors and NaN in the per_pair fields (base: the user's first)
template <int BLOCK>
__device__ __forceinline__ void explain_store_padding(int Lu, int L, int E, int32_t* __restrict__ item_base, double* __restrict__ contrib_base,
                                                      double* __restrict__ pair_base) {
    for (int x = threadIdx.x; x < (L - Lu) * E; x += BLOCK) {
        item_base[(size_t)Lu * E + x] = -1; contrib_base[(size_t)Lu * E + x] = 0.0;
    }
    if (pair_base)
        for (int x = threadIdx.x; x < (L - Lu) * PCR_EXPLAIN_PAIR_FIELDS; x += BLOCK) pair_base[(size_t)Lu * PCR_EXPLAIN_PAIR_FIELDS + x] = __builtin_nan("");
}

template <typename T, int BLOCK, bool BIG>
__global__ __launch_bounds__(BLOCK) void k_explain(FoldinCsr X, Geo geo, const int32_t* __restrict__ users, int nusers, const T* __restrict__ Um,
                                                   const int32_t* __restrict__ urow, const T* __restrict__ Vm, const double* __restrict__ lam_u,
                                                   const int32_t* __restrict__ lists, int L, int E, int32_t* __restrict__ expl_item,
                                                   double* __restrict__ expl_contrib, double* __restrict__ per_pair,
                                                   double* __restrict__ per_user, int strict, int cap, int rs_cap, int erows, char* scratch,
                                                   size_t stride) {
    typedef typename std::conditional<BIG, uint64_t, uint32_t>::type LI;
    typedef typename VecOf<T>::type V;
    constexpr int VEC = VecOf<T>::N;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    Carver small(smem);
    T* vecT = small.take<T>(geo.ld);
    double* red = small.take<double>(BLOCK / PCR_WAVE + 1);
    double* uvec = small.take<double>(geo.ld);
    double* gvec = small.take<double>(geo.ld);
    double* wbuf = small.take<double>((size_t)BLOCK * VEC);
    T* tile = small.take<T>((size_t)EXPLAIN_TILE * geo.ld);
    double* tile_u = small.take<double>(EXPLAIN_TILE);           // v_j . u
    double* tile_g = small.take<double>(EXPLAIN_TILE);           // v_j . g
    double* ebuf = small.take<double>((size_t)erows * EXPLAIN_TILE);
    double* topv0 = small.take<double>(EXPLAIN_TILE * 16);       // running top-E per tile position, two images
    double* topv1 = small.take<double>(EXPLAIN_TILE * 16);
    int32_t* topp0 = small.take<int32_t>(EXPLAIN_TILE * 16);
    int32_t* topp1 = small.take<int32_t>(EXPLAIN_TILE * 16);
    Carver big(BIG ? scratch + (size_t)blockIdx.x * stride : small.p);
    T* key = big.take<T>(cap);              // the sorted scores
    LI* li = big.take<LI>(cap);             // (level, CSR position) at each sorted position
    int32_t* itm = big.take<int32_t>(cap);  // CSR order
    uint16_t* lvc = big.take<uint16_t>(cap);
    double* Sx = big.take<double>((size_t)cap + 1);
    double* cc = big.take<double>(cap);     // the sweep coefficients, CSR order, fp64
    int* rs = big.take<int>(rs_cap);
    const int tid = threadIdx.x;
    const int ld = geo.ld;

    for (int ui = blockIdx.x; ui < nusers; ui += gridDim.x) {
        const int u = users[ui];
        const int64_t s0 = X.uptr[u];
        const int n = (int)(X.uptr[u + 1] - s0);
        const int nlev = (int)(X.runofs[u + 1] - X.runofs[u]) - 1;
        const double lam = lam_u[u];
        const T* urowp = Um + (size_t)(urow ? urow[u] : u) * ld;
        for (int t = tid; t < ld; t += BLOCK) { const T x = urowp[t]; vecT[t] = x; uvec[t] = (double)x; }
#pragma unroll 4
        for (int p = tid; p < n; p += BLOCK) { itm[p] = X.item[s0 + p]; lvc[p] = X.lvl[s0 + p]; }
        for (int l = tid; l <= nlev; l += BLOCK) rs[l] = X.runstart[X.runofs[u] + l];
        __syncthreads();
        // ---- the state at u, as k_foldin's eval_point and gradient sweep; c stays fp64
        double loss = 0.0;
        if (n > 0) {
            block_sddmm<T, BLOCK, false>(Vm, vecT, itm, n, key, geo, 0);
            for (int p = tid; p < n; p += BLOCK) li[p] = LiOps<LI>::pack(lvc[p], (unsigned)p);
            __syncthreads();
            bitonic_sort<T, LI, BLOCK, false, !BIG>(key, li, next_pow2(n), n);
            __syncthreads();
            loss = block_objective<T, BLOCK>(key, [&](int p) { return (int)LiOps<LI>::lev(li[p]); }, rs, nlev, n, Sx, red, strict);
            block_excl_scan<BLOCK>([&](int i) { return (double)key[i]; }, Sx, n, red);
            for (int p = tid; p < n; p += BLOCK) {
                const LI x = li[p];
                cc[LiOps<LI>::idx(x)] = sweep_coeff<T>(key, Sx, rs, nlev, (int)LiOps<LI>::lev(x), key[p], (double)key[p], 1.0, strict);
            }
            __syncthreads();
        }
        block_gradient<T, BLOCK>(Vm, itm, cc, n, lam, uvec, gvec, wbuf, geo);
        double gg = 0.0;
        for (int t = tid; t < ld; t += BLOCK) gg += gvec[t] * gvec[t];
        const double gn2 = block_sum<BLOCK>(gg, red);
        if (tid == 0 && per_user) {
            double* o = per_user + (size_t)u * PCR_EXPLAIN_USER_FIELDS;
            o[0] = (double)n; o[1] = loss; o[2] = gn2;
        }
        // ---- the listed items: non-padding entries first
        const int32_t* lst = lists + (size_t)u * L;
        int Lu = 0;
        for (int l = tid; l < L; l += BLOCK) Lu += lst[l] >= 0 ? 1 : 0;
        Lu = (int)block_sum<BLOCK>((double)Lu, red);
        for (int l0 = 0; l0 < Lu; l0 += EXPLAIN_TILE) {
            const int tl = min(EXPLAIN_TILE, Lu - l0);
            __syncthreads();
            for (int x = tid; x < EXPLAIN_TILE * geo.nchunk; x += BLOCK) {
                const int jj = x / geo.nchunk, ch = x - jj * geo.nchunk;
                V v = {};
                if (jj < tl) v = *reinterpret_cast<const V*>(Vm + row_off(lst[l0 + jj], geo) + ch * VEC);
                *reinterpret_cast<V*>(tile + jj * ld + ch * VEC) = v;
            }
            __syncthreads();
            if (tid < 64) {                                        // v_j . u and v_j . g: four lanes per tile position
                const int jj = tid >> 2, q = tid & 3;
                double a = 0.0, b = 0.0;
                for (int t = q; t < ld; t += 4) { const double v = (double)tile[jj * ld + t]; a += v * uvec[t]; b += v * gvec[t]; }
                a += lane_xor2(a); b += lane_xor2(b);
                a += lane_xor1(a); b += lane_xor1(b);
                if (q == 0) { tile_u[jj] = a; tile_g[jj] = b; }
            }
            double sup = 0.0, opp = 0.0;                            // of tile position tid (tid < tl)
            ExplainTop top = {topv0, topv1, topp0, topp1, 0};
            for (int p0 = 0; p0 < n; p0 += EXPLAIN_CHUNK) {
                const int p1 = min(n, p0 + EXPLAIN_CHUNK);
                __syncthreads();
                block_dots<T, BLOCK>(Vm, itm, [&](int p) { return -(cc[p] / lam); }, p0, p1, tile, ld, ebuf, geo);
                __syncthreads();
                explain_merge<BLOCK>(ebuf, p0, p1 - p0, tl, E, top, sup, opp);
            }
            __syncthreads();
            explain_store_top<BLOCK>(top, itm, tl, E, expl_item + ((size_t)u * L + l0) * E, expl_contrib + ((size_t)u * L + l0) * E);
            if (tid < tl && per_pair) {
                double* o = per_pair + ((size_t)u * L + l0 + tid) * PCR_EXPLAIN_PAIR_FIELDS;
                o[0] = tile_u[tid]; o[1] = sup; o[2] = opp; o[3] = tile_g[tid] / lam;
            }
        }
        // ---- padding positions
        explain_store_padding<BLOCK>(Lu, L, E, expl_item + (size_t)u * L * E, expl_contrib + (size_t)u * L * E,
                                     per_pair ? per_pair + (size_t)u * L * PCR_EXPLAIN_PAIR_FIELDS : nullptr);
        __syncthreads();
    }
}
