// pcr_topk.h -- top-K recommendation (pcr_recommend / pcr_recommend_model): for every requested user the K items of highest
// score U[u] . V[j], without the items the user rated in training, in the order of include/primalcr.h (descending score, equal
// scores by ascending item id).  DESIGN.md section 3.10 has the layout, the selection and the roofline.
//
// k_rec_score: a wave owns 16 users and sweeps the items [jb, je) of its split 64 at a time.  The scores of a step are four
//   16 x 16 tiles on the matrix cores (v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64) with the items as the A operand's rows
//   and the users as the B operand's columns, so every lane keeps ONE user (lane & 15) through the whole sweep: its threshold,
//   its exclusion cursor and its list length live in registers.  Each lane group g = lane >> 4 loads 16 bytes of a row per
//   k-step (k = c + KV g + e, e < KV) for both operands, so the k order of every score is fixed by the code alone.
//   Selection: a score that beats the user's threshold -- the K-th entry of its list, or nothing while the list is short --
//   goes into the user's candidate buffer in LDS (64 slots); when fewer than 16 slots are free the wave merges the buffer into
//   the user's list (global scratch, staged through LDS) by rank counting and raises the threshold.  After the first few
//   steps almost every score fails the threshold: one compare per score.
//   Exclusion: training rows are item-ascending (duplicates allowed); each lane walks a cursor through its user's row and
//   builds the 64-bit mask of the step's rated items -- O(nnz) in all.  With an allow set (pcr_recommend_filtered, DESIGN.md
//   section 3.17) the complement of the step's word of the packed set is ORed into that mask: one wave-uniform 8-byte load per step.
// k_rec_merge: one wave per user merges the partial lists of the item splits by rank counting (binary searches into the other
//   lists), converts the scores to double and pads with (-1, -inf).
// k_rec_cand: top-K over a candidate list per user (pcr_recommend_filtered with cand_ptr), one wave per user, below k_rec_merge;
//   its TOPN instantiation keeps the list in LDS and scores it (pcr_evaluate_topn_filtered with cand_ptr; section 3.21).
// k_rec_merge_topn: the same merge for the full-catalogue top-N evaluation (pcr_evaluate_topn): the list
//   stays in LDS and is scored against the user's relevant test items; k_topn_sum1 / k_topn_fin reduce the per-user metrics.
// k_rank_relscore / k_rank_sort / k_rank_count / k_rank_finish: the exact full-catalogue rank metrics (pcr_evaluate_ranks, DESIGN.md
//   section 3.12): the same sweep with a counting tail in place of the selecting one, at the end of this file.
// k_cand_count: that counting tail over a candidate row per user (pcr_evaluate_ranks_filtered with cand_ptr; section 3.21), one
//   wave per user, below k_rank_count.
// k_rec_merge_div / k_rec_merge_mmr: the same merge with the beyond-accuracy metrics (section 3.13) or the greedy MMR re-ranking
//   (pcr_recommend_diverse, section 3.14) fused into its tail, further down in this file.
// k_list_metrics: the two metric tails over a list that is already in device memory (pcr_evaluate_lists_model, and the theta sweep
//   pcr_evaluate_rerank, which runs it on k_rec_merge_mmr's output; section 3.15), below k_rec_merge_div.
// k_rec_merge_cap: the same merge with the group cap ("at most q items of one group", pcr_recommend_capped, section 3.23) fused
//   into its tail, at the end of this file.
// No atomic decides a result: the LDS slot counter only decides where a candidate sits in the buffer, and the merges rank by
// the total order (score, id), so every list is the same whatever the order of arrival.
#pragma once
#include "primalcr.h"
#include "pcr_prims.h"

namespace rec {
constexpr int WAVES = 4;      // waves per workgroup: the four sweep the same items, so three of them read V's rows from L1
constexpr int UW = 16;        // users per wave (the columns of the MFMA tile)
constexpr int NQ = 4;         // 16-item MFMA tiles per step
constexpr int TILE = 16 * NQ; // items per step
constexpr int CAP = 64;       // candidate slots per user; a merge is due when fewer than 16 are free
constexpr int RANK_STAGE = 32;            // k_rank_count: relevant rows up to this length are staged (and counted) in LDS
constexpr int RANK_LD = RANK_STAGE + 1;   // their LDS row stride (scores, ids, histogram): odd, see rank_wave_lds
constexpr int CAND_STAGE = PCR_CAND_RANK_STAGE;   // k_cand_count: relevant rows up to this length are staged (and counted) in LDS
}  // namespace rec

template <typename T> struct RecMma;
template <> struct RecMma<float> {
    typedef float acc_t __attribute__((ext_vector_type(4)));
    typedef float vec_t __attribute__((ext_vector_type(4)));
    static constexpr int KV = 4;   // k values per 16-byte load
    static __device__ __forceinline__ acc_t mma(float a, float b, acc_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
    // accumulator register j of lane l holds C[row][l & 15]
    static __device__ __forceinline__ int crow(int j, int l) { return 4 * (l >> 4) + j; }
};
template <> struct RecMma<double> {
    typedef double acc_t __attribute__((ext_vector_type(4)));
    typedef double vec_t __attribute__((ext_vector_type(2)));
    static constexpr int KV = 2;
    static __device__ __forceinline__ acc_t mma(double a, double b, acc_t c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int crow(int j, int l) { return (l >> 4) + 4 * j; }
};

// the order of a list: a before b
template <typename T>
__device__ __forceinline__ bool rec_better(T sa, int ia, T sb, int ib) { return sa > sb || (sa == sb && ia < ib); }

// LDS of one wave of k_rec_score: candidate scores [UW * CAP], staged list scores [K], candidate ids, staged ids, fill counters
template <typename T>
__host__ __device__ inline size_t rec_wave_lds(int K) {
    const size_t b = (size_t)(rec::UW * rec::CAP + K) * (sizeof(T) + sizeof(int)) + rec::UW * sizeof(int);
    return (b + 15) & ~(size_t)15;
}

// The scores of one step: acc[q] = the 16 x 16 tile of the rows row_of(q) of V (the A operand; row_of is asked by lane m = lane & 15
// for its row of tile q, -1: none, a zero row) against the wave's 16 user columns (the B operand: lane m + 16 g holds its user's
// row Ur, inactive columns are zero).  Lane group g loads 16 bytes of a row per k-step for both operands, so the k order of a
// score is fixed by this code alone and depends on its (row of U, row of V) only: every caller that scores a pair through here
// gets the same bits (k_rec_score, k_rank_count and k_rank_relscore rely on that).
template <typename T, class RowOf>
__device__ __forceinline__ void rec_score_tile(const T* __restrict__ Ur, bool active, const T* __restrict__ V, int r, int ld, int g,
                                               RowOf&& row_of, typename RecMma<T>::acc_t (&acc)[rec::NQ]) {
    typedef RecMma<T> M;
    typedef typename M::acc_t acc_t;
    typedef typename M::vec_t vec_t;
    constexpr int KV = M::KV;
#pragma unroll
    for (int q = 0; q < rec::NQ; ++q) acc[q] = acc_t{};
    for (int c = 0; c < ld; c += 4 * KV) {          // wave-uniform trip count: the MFMAs run with every lane
        const int c0 = c + g * KV;
        vec_t b = vec_t{};
        if (active && c0 < ld) b = *(const vec_t*)(Ur + c0);
#pragma unroll
        for (int e = 0; e < KV; ++e) if (c0 + e >= r) b[e] = (T)0;
#pragma unroll
        for (int q = 0; q < rec::NQ; ++q) {
            const int jr = row_of(q);
            vec_t a = vec_t{};
            if (jr >= 0 && c0 < ld) a = *(const vec_t*)(V + (size_t)(unsigned)jr * (unsigned)ld + c0);
#pragma unroll
            for (int e = 0; e < KV; ++e) if (c0 + e >= r) a[e] = (T)0;
#pragma unroll
            for (int e = 0; e < KV; ++e) acc[q] = M::mma(a[e], b[e], acc[q]);
        }
    }
}

// partial lists: [split][n][K] scores and ids, [split][n] lengths
template <typename T>
__global__ __launch_bounds__(256) void k_rec_score(const T* __restrict__ U, const T* __restrict__ V, int r, int ld, int d2,
                                                   const int32_t* __restrict__ users, int64_t n,
                                                   const int64_t* __restrict__ xptr, const int32_t* __restrict__ xitem,
                                                   int K, int per_split, T* __restrict__ lst_s, int32_t* __restrict__ lst_i,
                                                   int32_t* __restrict__ lst_n, int select,
                                                   const unsigned long long* __restrict__ allow) {
    typedef RecMma<T> M;
    typedef typename M::acc_t acc_t;
    extern __shared__ __align__(16) char rec_lds[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    char* wl = rec_lds + (size_t)w * rec_wave_lds<T>(K);
    T* bs = (T*)wl;
    T* ss = bs + rec::UW * rec::CAP;
    int* bi = (int*)(ss + K);
    int* si = bi + rec::UW * rec::CAP;
    int* fill = si + K;

    const int m = lane & 15, g = lane >> 4;
    const int64_t idx = ((int64_t)blockIdx.x * rec::WAVES + w) * rec::UW + m;
    const bool active = idx < n;
    const int u = active ? users[idx] : 0;
    const int jb = (int)blockIdx.y * per_split;
    const int je = min(d2, jb + per_split);
    const size_t lofs = active ? ((size_t)blockIdx.y * (size_t)n + (size_t)idx) * (size_t)K : 0;
    int64_t cur = 0, cend = 0;
    if (xptr && active) {
        cur = xptr[u]; cend = xptr[u + 1];
        int64_t hi = cend;
        while (cur < hi) { const int64_t mid = (cur + hi) >> 1; if (xitem[mid] < jb) cur = mid + 1; else hi = mid; }
    }
    if (lane < rec::UW) fill[lane] = 0;
    int len = 0;
    T ts = -INFINITY;
    int ti = INT_MAX;
    wave_sync();

    // merge user column mm's candidate buffer into its list; every lane of the wave takes part
    auto merge = [&](int mm) {
        const int B = fill[mm];
        const int L = __shfl(len, mm);
        const size_t lo = (size_t)__shfl((long long)lofs, mm);
        T* gs = lst_s + lo;
        int32_t* gi = lst_i + lo;
        const T* cs = bs + mm * rec::CAP;
        const int* ci = bi + mm * rec::CAP;
        for (int p = lane; p < L; p += 64) { ss[p] = gs[p]; si[p] = gi[p]; }
        wave_sync();
        bool has = false;
        T hs = -INFINITY;
        int hi_ = INT_MAX;
        if (lane < B) {
            const T s = cs[lane];
            const int j = ci[lane];
            int rk = 0;
            for (int e = 0; e < B; ++e) rk += rec_better(cs[e], ci[e], s, j) ? 1 : 0;
            int a = 0, b = L;
            while (a < b) { const int mid = (a + b) >> 1; if (rec_better(ss[mid], si[mid], s, j)) a = mid + 1; else b = mid; }
            rk += a;
            if (rk < K) { gs[rk] = s; gi[rk] = j; }
            if (rk == K - 1) { has = true; hs = s; hi_ = j; }
        }
        for (int p = lane; p < L; p += 64) {
            const T s = ss[p];
            const int j = si[p];
            int rk = p;
            for (int e = 0; e < B; ++e) rk += rec_better(cs[e], ci[e], s, j) ? 1 : 0;
            if (rk < K) { gs[rk] = s; gi[rk] = j; }
            if (rk == K - 1) { has = true; hs = s; hi_ = j; }
        }
        const int nl = min(K, L + B);
        const unsigned long long hb = __ballot(has);
        if (hb) {
            const int src = __ffsll((long long)hb) - 1;
            hs = __shfl(hs, src);
            hi_ = __shfl(hi_, src);
        }
        if (m == mm) {
            len = nl;
            if (nl == K) { ts = hs; ti = hi_; }
        }
        __threadfence_block();             // the next merge of this user reads the list back
        wave_sync();
        if (lane == 0) fill[mm] = 0;
        wave_sync();
    };

    const T* Ur = U + (size_t)(unsigned)u * (unsigned)ld;
    for (int j0 = jb; j0 < je; j0 += rec::TILE) {
        acc_t acc[rec::NQ];
        rec_score_tile<T>(Ur, active, V, r, ld, g, [&](int q) { const int jr = j0 + 16 * q + m; return jr < je ? jr : -1; }, acc);
        if (!select) {                                 // (tools/exp_recommend.py: the GEMM alone; the NaN test keeps it alive)
            T t = (T)0;
#pragma unroll
            for (int q = 0; q < rec::NQ; ++q) t += acc[q][0] + acc[q][1] + acc[q][2] + acc[q][3];
            if (t != t && active && g == 0) lst_n[(size_t)blockIdx.y * (size_t)n + (size_t)idx] = -1;
            continue;
        }
        unsigned long long xm = 0;                     // this step's rated items of the lane's user
        while (cur < cend) {
            const int it = xitem[cur];
            if (it >= j0 + rec::TILE) break;
            xm |= 1ull << (it - j0);
            ++cur;
        }
        if (allow) xm |= ~allow[j0 >> 6];              // (j0 is a multiple of 64: the step is one word of the packed allow set)
#pragma unroll
        for (int q = 0; q < rec::NQ; ++q) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int jl = 16 * q + M::crow(j, lane);
                const int item = j0 + jl;
                const T s = acc[q][j];
                if (active && item < je && !((xm >> jl) & 1ull) && rec_better(s, item, ts, ti)) {
                    const int p = atomicAdd(&fill[m], 1);
                    bs[m * rec::CAP + p] = s;
                    bi[m * rec::CAP + p] = item;
                }
            }
            wave_sync();
            unsigned long long due = __ballot(lane < rec::UW && fill[lane] > rec::CAP - 16);
            while (due) {
                const int mm = __ffsll((long long)due) - 1;
                due &= due - 1;
                merge(mm);
            }
        }
    }
    unsigned long long due = __ballot(lane < rec::UW && fill[lane] > 0);
    while (due) {
        const int mm = __ffsll((long long)due) - 1;
        due &= due - 1;
        merge(mm);
    }
    if (active && g == 0) lst_n[(size_t)blockIdx.y * (size_t)n + (size_t)idx] = len;
}

// the rank of every entry of the nsplit partial lists of user idx in the merged list, by rank counting (binary searches into
// the other lists); emit(rank, id, score) for ranks < K.  Returns the total length of the partial lists.
template <typename T, class Emit>
__device__ __forceinline__ int rec_merge_ranks(const T* __restrict__ lst_s, const int32_t* __restrict__ lst_i,
                                               const int32_t* __restrict__ lst_n, int nsplit, int64_t n, int K, int64_t idx, int lane,
                                               Emit&& emit) {
    int tot = 0;
    for (int sp = 0; sp < nsplit; ++sp) {
        const size_t o = ((size_t)sp * (size_t)n + (size_t)idx) * (size_t)K;
        const int L = lst_n[(size_t)sp * (size_t)n + (size_t)idx];
        tot += L;
        for (int p = lane; p < L; p += 64) {
            const T s = lst_s[o + p];
            const int j = lst_i[o + p];
            int rk = p;
            for (int sq = 0; sq < nsplit; ++sq) {
                if (sq == sp) continue;
                const size_t o2 = ((size_t)sq * (size_t)n + (size_t)idx) * (size_t)K;
                int a = 0, b = lst_n[(size_t)sq * (size_t)n + (size_t)idx];
                while (a < b) { const int mid = (a + b) >> 1; if (rec_better(lst_s[o2 + mid], lst_i[o2 + mid], s, j)) a = mid + 1; else b = mid; }
                rk += a;
            }
            if (rk < K) emit(rk, j, s);
        }
    }
    return tot;
}

// one wave per user: the nsplit partial lists -> items[idx * K ...], scores (double), padded with (-1, -inf)
template <typename T>
__global__ __launch_bounds__(256) void k_rec_merge(const T* __restrict__ lst_s, const int32_t* __restrict__ lst_i,
                                                   const int32_t* __restrict__ lst_n, int nsplit, int64_t n, int K,
                                                   int32_t* __restrict__ out_i, double* __restrict__ out_s) {
    const int lane = threadIdx.x & 63;
    const int64_t idx = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (idx >= n) return;
    const int tot = rec_merge_ranks(lst_s, lst_i, lst_n, nsplit, n, K, idx, lane, [&](int rk, int j, T s) {
        out_i[(size_t)idx * K + rk] = j; out_s[(size_t)idx * K + rk] = (double)s;
    });
    for (int p = min(tot, K) + lane; p < K; p += 64) { out_i[(size_t)idx * K + p] = -1; out_s[(size_t)idx * K + p] = -INFINITY; }
}

// Top-N evaluation (pcr_evaluate_topn): the relevance tables of the batch's users (offset to the batch), built on the host.
struct TopnArgs {
    const int64_t* rptr;   // [n + 1] relevant CSR: distinct items, item-ascending
    const int32_t* ritem;
    const double* rgain;   // graded gain of each relevant item
    const double* idcg;    // [n][ncut][2] ideal DCG, binary then graded
    const double* disc;    // [K] d(i) = 1 / log2(i + 2)
    double* out;           // [n][ncut][6] hits, precision, recall, ap, ndcg, ndcg_graded
    int ncut;
    int cut[PCR_TOPN_MAX_CUTOFFS];
};

// One step of a candidate-row kernel (k_rec_cand, k_cand_count), the whole wave: candidates ci[t0 .. t0 + 64) of a row of nc ids
// are scored against the one user row Ur through rec_score_tile -- all 16 columns of the tile are this user and column 0 is
// read, as k_rank_relscore does, so a score has the bits k_rec_score gives the pair -- and handed to the lanes through the wave's
// 64-entry LDS stage stg: lane `lane` gets candidate t0 + lane, its id (-1 past the row's end) and its score s.  Returns whether
// the candidate is eligible: its bit of the packed allow set is on (allow NULL: every item) and a binary search does not find it
// in the user's item-ascending training row xitem[xb, xe) (an empty range: no exclusion).  The caller orders the wave
// (wave_sync) before the next step overwrites stg.  Both kernels score and filter through here, so they cannot drift apart.
template <typename T>
__device__ __forceinline__ bool cand_step(const T* __restrict__ Ur, const T* __restrict__ V, int r, int ld, const int32_t* __restrict__ ci,
                                          int64_t nc, int64_t t0, int lane, T* stg, const unsigned long long* __restrict__ allow,
                                          const int32_t* __restrict__ xitem, int64_t xb, int64_t xe, int& id, T& s) {
    typedef RecMma<T> M;
    typedef typename M::acc_t acc_t;
    const int m = lane & 15, g = lane >> 4;
    const int64_t t = t0 + lane;
    id = t < nc ? (int)ci[t] : -1;
    int jr[rec::NQ];
#pragma unroll
    for (int q = 0; q < rec::NQ; ++q) jr[q] = __shfl(id, 16 * q + m);
    acc_t acc[rec::NQ];
    rec_score_tile<T>(Ur, true, V, r, ld, g, [&](int q) { return jr[q]; }, acc);
    if (m == 0) {
#pragma unroll
        for (int q = 0; q < rec::NQ; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j) stg[16 * q + M::crow(j, lane)] = acc[q][j];
    }
    wave_sync();
    s = stg[lane];
    bool ok = id >= 0;
    if (ok && allow) ok = ((allow[id >> 6] >> (id & 63)) & 1ull) != 0;
    if (ok && xe > xb) {
        int64_t a = xb, b = xe;
        while (a < b) { const int64_t mid = (a + b) >> 1; if (xitem[mid] < id) a = mid + 1; else b = mid; }
        ok = !(a < xe && xitem[a] == id);
    }
    return ok;
}

// LDS of one wave of k_rec_cand: the user's list scores [K], the survivor buffer's scores [CAP], the step's scores [TILE], the
// list ids [K], the buffer ids [CAP]
template <typename T>
__host__ __device__ inline size_t cand_wave_lds(int K) {
    const size_t b = (size_t)(K + rec::CAP + rec::TILE) * sizeof(T) + (size_t)(K + rec::CAP) * sizeof(int);
    return (b + 15) & ~(size_t)15;
}

// Top-K over candidate lists (pcr_recommend_filtered with cand_ptr), one wave per user, four users per
// workgroup: row idx of the candidate CSR (cptr[n + 1] absolute, citem based at cptr[0]; ids in any order, none twice in a row)
// belongs to users[idx].  Each step (cand_step, shared with k_cand_count) scores 64 candidates through rec_score_tile -- all 16 columns of the tile are this one user
// and column 0 is read, as k_rank_relscore does, so a score has the bits k_rec_score gives the same (user, item) -- and hands
// candidate t0 + lane to lane `lane` through LDS.  A candidate is eligible when its bit of the packed allow set is on (allow
// NULL: every item) and a binary search does not find it in the user's item-ascending training row (xptr NULL: no exclusion).
// Selection is the sweep's: an eligible score that beats the threshold (the K-th list entry, in registers; nothing while the
// list is short) goes to the 64-slot buffer at the position of its lane among the step's survivors (a prefix count of the
// ballot: no atomic); when a step's survivors would not fit, and at the end, the buffer merges into the list by rank counting
// under rec_better.  The list stays in the wave's LDS for the whole call and is merged in place: a list entry moves up by the
// number of buffer entries before it, never down, so the wave shifts the list 64 entries at a time from its end (each chunk
// is read before it is written, and a chunk writes at or above its own positions only), then drops the buffer entries into
// their ranks.  The ids of a row are distinct, so the order is strict and a list is the same whatever the order of the row.
// The tail converts to double and pads with (-1, -inf).  Every loop is bounded by K, by 64 or by the row's length.
// TOPN (pcr_evaluate_topn_filtered): the finished list is not written out; it is padded with -1 where it
// stands, in the wave's LDS, and scored by rec_topn_tail against ta's relevance tables (offset to the batch, as k_rec_merge_topn's):
// the selection above is the same code, so the list scored is the list the plain instantiation returns.
__device__ __forceinline__ void rec_topn_tail(int32_t* sl, int K, int64_t idx, int lane, const TopnArgs& ta);   // (below)
template <typename T, bool TOPN>
__global__ __launch_bounds__(256) void k_rec_cand(const T* __restrict__ U, const T* __restrict__ V, int r, int ld,
                                                  const int32_t* __restrict__ users, int64_t n, const int64_t* __restrict__ cptr,
                                                  const int32_t* __restrict__ citem, const unsigned long long* __restrict__ allow,
                                                  const int64_t* __restrict__ xptr, const int32_t* __restrict__ xitem, int K,
                                                  int32_t* __restrict__ out_i, double* __restrict__ out_s, TopnArgs ta) {
    extern __shared__ __align__(16) char rec_lds[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t idx = (int64_t)blockIdx.x * 4 + w;
    if (idx >= n) return;                               // (the whole wave)
    char* wl = rec_lds + (size_t)w * cand_wave_lds<T>(K);
    T* ls = (T*)wl;
    T* bs = ls + K;
    T* stg = bs + rec::CAP;
    int* li = (int*)(stg + rec::TILE);
    int* bi = li + K;

    const int u = users[idx];
    const int64_t nc = cptr[idx + 1] - cptr[idx];
    const int32_t* ci = citem + (cptr[idx] - cptr[0]);
    int64_t xb = 0, xe = 0;
    if (xptr) { xb = xptr[u]; xe = xptr[u + 1]; }
    const T* Ur = U + (size_t)(unsigned)u * (unsigned)ld;
    int len = 0, fill = 0;                              // (wave-uniform)
    T ts = -INFINITY;
    int ti = INT_MAX;

    auto merge = [&]() {
        const int B = fill, L = len;
        T s = (T)0;
        int j = 0, rk = K;
        if (lane < B) {                                // a buffer entry: its rank among the buffer and the list as it stands
            s = bs[lane]; j = bi[lane];
            rk = 0;
            for (int e = 0; e < B; ++e) rk += rec_better(bs[e], bi[e], s, j) ? 1 : 0;
            int a = 0, b = L;
            while (a < b) { const int mid = (a + b) >> 1; if (rec_better(ls[mid], li[mid], s, j)) a = mid + 1; else b = mid; }
            rk += a;
        }
        for (int c = (L - 1) & ~63; L > 0 && c >= 0; c -= 64) {
            const int p = c + lane;
            T es = (T)0;
            int ej = 0, erk = K;
            if (p < L) {
                es = ls[p]; ej = li[p];
                erk = p;
                for (int e = 0; e < B; ++e) erk += rec_better(bs[e], bi[e], es, ej) ? 1 : 0;
            }
            wave_sync();
            if (erk < K) { ls[erk] = es; li[erk] = ej; }
            wave_sync();
        }
        if (rk < K) { ls[rk] = s; li[rk] = j; }
        wave_sync();
        len = min(K, L + B);
        fill = 0;
        if (len == K) { ts = ls[K - 1]; ti = li[K - 1]; }
    };

    for (int64_t t0 = 0; t0 < nc; t0 += rec::TILE) {
        int id;
        T s;
        bool ok = cand_step<T>(Ur, V, r, ld, ci, nc, t0, lane, stg, allow, xitem, xb, xe, id, s);
        ok = ok && rec_better(s, id, ts, ti);
        const unsigned long long pm = __ballot(ok);
        const int c = __popcll(pm);
        if (fill + c > rec::CAP) merge();              // (wave-uniform)
        if (ok) {
            const int p = fill + __popcll(pm & ((1ull << lane) - 1ull));
            bs[p] = s; bi[p] = id;
        }
        fill += c;
        wave_sync();
    }
    if (fill > 0) merge();
    wave_sync();
    if (TOPN) {
        for (int p = len + lane; p < K; p += 64) li[p] = -1;
        wave_sync();
        rec_topn_tail(li, K, idx, lane, ta);
        return;
    }
    for (int p = lane; p < K; p += 64) {
        const bool have = p < len;
        out_i[(size_t)idx * K + p] = have ? li[p] : -1;
        out_s[(size_t)idx * K + p] = have ? (double)ls[p] : -INFINITY;
    }
}

// k_rec_merge with the metrics fused into its tail, one wave per user: the merged list goes to the wave's LDS row (K ids; 4 K
// ints of dynamic LDS per workgroup) and is never written out.  Lanes own contiguous position ranges; each list entry is
// looked up in the user's relevant row by binary search (its slot replaces the id in LDS, -1 if not relevant); a wave
// exclusive scan of the lanes' hit counts gives every hit its hits_{<=i}; the per-cutoff sums are reduced by wave_sum's fixed
// butterfly.
// (the tail is rec_topn_tail, shared with k_list_metrics)
__device__ __forceinline__ void rec_topn_tail(int32_t* sl, int K, int64_t idx, int lane, const TopnArgs& ta) {
    const int64_t rb = ta.rptr[idx], nr = ta.rptr[idx + 1] - rb;
    const int32_t* ri = ta.ritem + rb;
    const int P = (K + 63) >> 6, p0 = min(K, lane * P), p1 = min(K, p0 + P);
    int h = 0;
    for (int i = p0; i < p1; ++i) {              // the list entry -> its slot in the relevant row, or -1
        const int j = sl[i];
        int f = -1;
        if (j >= 0) {
            int64_t a = 0, b = nr;
            while (a < b) { const int64_t mid = (a + b) >> 1; if (ri[mid] < j) a = mid + 1; else b = mid; }
            if (a < nr && ri[a] == j) f = (int)a;
        }
        sl[i] = f;
        h += f >= 0 ? 1 : 0;
    }
    int ex = h;                                   // inclusive scan of the lanes' hit counts (integers: exact), then exclusive
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(ex, d); if (lane >= d) ex += t; }
    ex -= h;
    int hits[PCR_TOPN_MAX_CUTOFFS];
    double ap[PCR_TOPN_MAX_CUTOFFS], dcg[PCR_TOPN_MAX_CUTOFFS], gdcg[PCR_TOPN_MAX_CUTOFFS];
#pragma unroll
    for (int c = 0; c < PCR_TOPN_MAX_CUTOFFS; ++c) { hits[c] = 0; ap[c] = 0.0; dcg[c] = 0.0; gdcg[c] = 0.0; }
    int cum = ex;
    for (int i = p0; i < p1; ++i) {
        const int f = sl[i];
        if (f < 0) continue;
        ++cum;
        const double pr = (double)cum / (double)(i + 1), d = ta.disc[i], gd = ta.rgain[rb + f] * d;
#pragma unroll
        for (int c = 0; c < PCR_TOPN_MAX_CUTOFFS; ++c)
            if (c < ta.ncut && i < ta.cut[c]) { hits[c] += 1; ap[c] += pr; dcg[c] += d; gdcg[c] += gd; }
    }
    // lane l < 6 ncut writes field l % 6 of cutoff l / 6: one coalesced row per user
    double v = 0.0;
    const int myc = lane / 6, myf = lane - 6 * myc;
#pragma unroll
    for (int c = 0; c < PCR_TOPN_MAX_CUTOFFS; ++c) {
        if (c >= ta.ncut) break;                  // (wave-uniform)
        const double H = wave_sum((double)hits[c]);   // (an exact integer)
        const double A = wave_sum(ap[c]), D = wave_sum(dcg[c]), G = wave_sum(gdcg[c]);
        const double* id = ta.idcg + ((size_t)idx * ta.ncut + c) * 2;
        const double c_ = (double)ta.cut[c], m = (double)(ta.cut[c] < nr ? (int64_t)ta.cut[c] : nr);
        if (myc == c) {
            v = myf == 0 ? H : myf == 1 ? H / c_ : myf == 2 ? H / (double)nr : myf == 3 ? A / m : myf == 4 ? D / id[0]
              : (id[1] > 0.0 ? G / id[1] : (double)NAN);
        }
    }
    if (lane < 6 * ta.ncut) ta.out[(size_t)idx * 6 * ta.ncut + lane] = v;
}
template <typename T>
__global__ __launch_bounds__(256) void k_rec_merge_topn(const T* __restrict__ lst_s, const int32_t* __restrict__ lst_i,
                                                        const int32_t* __restrict__ lst_n, int nsplit, int64_t n, int K, TopnArgs ta) {
    extern __shared__ int32_t rec_lst[];
    const int lane = threadIdx.x & 63;
    const int64_t idx = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (idx >= n) return;
    int32_t* sl = rec_lst + (size_t)(threadIdx.x >> 6) * (size_t)K;
    const int tot = rec_merge_ranks(lst_s, lst_i, lst_n, nsplit, n, K, idx, lane, [&](int rk, int j, T) { sl[rk] = j; });
    for (int p = min(tot, K) + lane; p < K; p += 64) sl[p] = -1;
    wave_sync();
    rec_topn_tail(sl, K, idx, lane, ta);
}

// Top-N evaluation's sums over users (fixed order, as k_sum4_stage1 / k_fin4): block x of cutoff y = blockIdx.y sums rows
// [x per_block, ...) of the per-user table into part[y][x][8] = hits, precision, recall, users with a hit, ap, ndcg,
// ndcg_graded (defined ones), users with ndcg_graded defined.
__global__ __launch_bounds__(PCR_EW_BLOCK) void k_topn_sum1(const double* __restrict__ in, int64_t n, int ncut, int per_block,
                                                            double* __restrict__ part) {
    __shared__ double red[PCR_EW_BLOCK / PCR_WAVE + 1];
    const int c = blockIdx.y;
    const int64_t lo = (int64_t)blockIdx.x * per_block;
    const int64_t hi = (lo + per_block < n) ? lo + per_block : n;
    double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t i = lo + threadIdx.x; i < hi; i += PCR_EW_BLOCK) {
        const double* r = in + ((size_t)i * ncut + c) * 6;
        a[0] += r[0]; a[1] += r[1]; a[2] += r[2]; a[3] += r[0] > 0.0 ? 1.0 : 0.0; a[4] += r[3]; a[5] += r[4];
        if (r[5] == r[5]) { a[6] += r[5]; a[7] += 1.0; }
    }
#pragma unroll
    for (int f = 0; f < 8; ++f) {
        const double s = block_sum<PCR_EW_BLOCK>(a[f], red);
        if (threadIdx.x == 0) part[((size_t)c * gridDim.x + blockIdx.x) * 8 + f] = s;
    }
}
// one block per cutoff: out[c][8] = the sums of part[c][0..nblk)[8]; out[8 ncut] = n (the counted users of this shard)
__global__ __launch_bounds__(PCR_EW_BLOCK) void k_topn_fin(const double* __restrict__ part, int nblk, int64_t n, double* __restrict__ out) {
    __shared__ double red[PCR_EW_BLOCK / PCR_WAVE + 1];
    const int c = blockIdx.x;
#pragma unroll
    for (int f = 0; f < 8; ++f) {
        double x = 0.0;
        for (int i = threadIdx.x; i < nblk; i += PCR_EW_BLOCK) x += part[((size_t)c * nblk + i) * 8 + f];
        x = block_sum<PCR_EW_BLOCK>(x, red);
        if (threadIdx.x == 0) out[c * 8 + f] = x;
    }
    if (c == 0 && threadIdx.x == 0) out[gridDim.x * 8] = (double)n;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Exact full-catalogue rank metrics (pcr_evaluate_ranks, include/primalcr.h).  Per counted user a
// histogram over |R_u| + 1 buckets: bucket b counts the eligible non-relevant items that have exactly b relevant items before
// them.  The relevance tables are TopnArgs' (rptr / ritem: distinct items, item-ascending).

// One wave per counted user: the scores of its relevant items, us[rptr[idx] + t] for ritem[rptr[idx] + t], 64 per step through
// rec_score_tile -- the same chain as the sweep's, so that the sweep recognises a relevant item by its (score, id).  All 16
// columns of the tile are this one user; column 0 is read.
template <typename T>
__global__ __launch_bounds__(256) void k_rank_relscore(const T* __restrict__ U, const T* __restrict__ V, int r, int ld,
                                                       const int32_t* __restrict__ users, int64_t n, const int64_t* __restrict__ rptr,
                                                       const int32_t* __restrict__ ritem, T* __restrict__ us) {
    typedef RecMma<T> M;
    typedef typename M::acc_t acc_t;
    const int lane = threadIdx.x & 63;
    const int64_t idx = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (idx >= n) return;                               // (the whole wave)
    const int m = lane & 15, g = lane >> 4;
    const int64_t rb = rptr[idx], nr = rptr[idx + 1] - rb;
    const T* Ur = U + (size_t)(unsigned)users[idx] * (unsigned)ld;
    for (int64_t t0 = 0; t0 < nr; t0 += rec::TILE) {
        acc_t acc[rec::NQ];
        rec_score_tile<T>(Ur, true, V, r, ld, g, [&](int q) { const int64_t t = t0 + 16 * q + m; return t < nr ? (int)ritem[rb + t] : -1; }, acc);
#pragma unroll
        for (int q = 0; q < rec::NQ; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t t = t0 + 16 * q + M::crow(j, lane);
                if (m == 0 && t < nr) us[rb + t] = acc[q][j];
            }
    }
}

// One wave per counted user: its relevant row in the order of a list (rec_better) by rank counting, as the merges do: rs / ri
// the sorted scores and ids, rslot[t] = the position in the item-ascending row of the t-th entry.  The ids of a row are
// distinct, so the order is strict and every rank is taken once.
template <typename T>
__global__ __launch_bounds__(256) void k_rank_sort(int64_t n, const int64_t* __restrict__ rptr, const int32_t* __restrict__ ritem,
                                                   const T* __restrict__ us, T* __restrict__ rs, int32_t* __restrict__ ri,
                                                   int32_t* __restrict__ rslot) {
    const int lane = threadIdx.x & 63;
    const int64_t idx = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (idx >= n) return;
    const int64_t rb = rptr[idx];
    const int nr = (int)(rptr[idx + 1] - rb);
    for (int p = lane; p < nr; p += 64) {
        const T s = us[rb + p];
        const int j = ritem[rb + p];
        int rk = 0;
        for (int e = 0; e < nr; ++e) rk += rec_better(us[rb + e], ritem[rb + e], s, j) ? 1 : 0;
        rs[rb + rk] = s; ri[rb + rk] = j; rslot[rb + rk] = p;
    }
}

// LDS of one wave of k_rank_count: per user column a staged relevant row (RANK_LD scores, RANK_LD ids) and its histogram
// (RANK_LD counters).  The odd stride puts entry t of the 16 users of a wave into 16 different banks (32 in fp64, two per
// entry), so neither the probes of a binary search that run in step nor the adds to equal buckets share a bank.
template <typename T>
__host__ __device__ inline size_t rank_wave_lds() {
    const size_t b = (size_t)rec::UW * rec::RANK_LD * (sizeof(T) + 2 * sizeof(int));
    return (b + 15) & ~(size_t)15;
}

// b = the number of entries of the sorted row (s[t], id[t]), t < nr, that come before (sc, item); -1 when the item meets itself
template <typename T, class S, class I>
__device__ __forceinline__ int rank_bucket(const S s, const I id, int nr, T sc, int item) {
    int a = 0, b = nr;
    while (a < b) { const int mid = (a + b) >> 1; if (rec_better(s[mid], id[mid], sc, item)) a = mid + 1; else b = mid; }
    return (a < nr && s[a] == sc && id[a] == item) ? -1 : a;
}

// The counting sweep: k_rec_score's layout (a wave owns 16 users, a lane keeps one user, 64 items per step, the same exclusion
// cursor and item splits on blockIdx.y) with this tail: every eligible score is placed into the user's sorted relevant row.
// The best and the worst relevant (score, id) sit in registers: an item before the best goes to bucket 0 and one after the
// worst to bucket nr without a search, in per-lane register counters (most of the catalogue).  The others are searched: rows
// of at most RANK_STAGE entries in LDS with an LDS integer add, longer ones in global memory (rs / ri, L2-resident) with a
// global integer add.  An item that compares equal to a row entry (same score, same id) is a relevant item meeting itself and
// is not counted.  Integer adds commute: the histogram is the same whatever the order of arrival.
// hist: [split][hsplit] counters, zeroed by the caller; user idx's nr + 1 buckets start at (rptr[idx] - rptr[0]) + idx.
// allow (pcr_evaluate_ranks_filtered; NULL: every item): the packed allow set, ORed complemented into the
// step's exclusion mask exactly as k_rec_score does.
template <typename T>
__global__ __launch_bounds__(256) void k_rank_count(const T* __restrict__ U, const T* __restrict__ V, int r, int ld, int d2,
                                                    const int32_t* __restrict__ users, int64_t n,
                                                    const int64_t* __restrict__ xptr, const int32_t* __restrict__ xitem, int per_split,
                                                    const int64_t* __restrict__ rptr, const T* __restrict__ rs, const int32_t* __restrict__ ri,
                                                    int32_t* __restrict__ hist, int64_t hsplit,
                                                    const unsigned long long* __restrict__ allow) {
    typedef RecMma<T> M;
    typedef typename M::acc_t acc_t;
    extern __shared__ __align__(16) char rec_lds[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int m = lane & 15, g = lane >> 4;
    char* wl = rec_lds + (size_t)w * rank_wave_lds<T>();
    T* ls = (T*)wl + m * rec::RANK_LD;
    int* li = (int*)((T*)wl + rec::UW * rec::RANK_LD) + m * rec::RANK_LD;
    int* lh = li + rec::UW * rec::RANK_LD;

    const int64_t idx = ((int64_t)blockIdx.x * rec::WAVES + w) * rec::UW + m;
    const bool active = idx < n;
    const int u = active ? users[idx] : 0;
    const int jb = (int)blockIdx.y * per_split;
    const int je = min(d2, jb + per_split);
    int64_t cur = 0, cend = 0;
    if (xptr && active) {
        cur = xptr[u]; cend = xptr[u + 1];
        int64_t hi = cend;
        while (cur < hi) { const int64_t mid = (cur + hi) >> 1; if (xitem[mid] < jb) cur = mid + 1; else hi = mid; }
    }
    int nr = 0;
    const T* gs = rs;
    const int32_t* gi = ri;
    int32_t* gh = hist;
    T best_s = (T)0, worst_s = (T)0;
    int best_i = 0, worst_i = 0;
    if (active) {                                      // (a counted user: nr >= 1)
        const int64_t rb = rptr[idx];
        nr = (int)(rptr[idx + 1] - rb);
        gs += rb; gi += rb;
        gh += (size_t)blockIdx.y * (size_t)hsplit + (size_t)(rb - rptr[0]) + (size_t)idx;
        best_s = gs[0]; best_i = gi[0]; worst_s = gs[nr - 1]; worst_i = gi[nr - 1];
    }
    const bool staged = active && nr <= rec::RANK_STAGE;
    if (staged) {
        for (int t = g; t < nr; t += 4) { ls[t] = gs[t]; li[t] = gi[t]; }
        for (int t = g; t <= nr; t += 4) lh[t] = 0;
    }
    wave_sync();
    int c_lo = 0, c_hi = 0;

    const T* Ur = U + (size_t)(unsigned)u * (unsigned)ld;
    for (int j0 = jb; j0 < je; j0 += rec::TILE) {
        acc_t acc[rec::NQ];
        rec_score_tile<T>(Ur, active, V, r, ld, g, [&](int q) { const int jr = j0 + 16 * q + m; return jr < je ? jr : -1; }, acc);
        unsigned long long xm = 0;                     // this step's rated items of the lane's user
        while (cur < cend) {
            const int it = xitem[cur];
            if (it >= j0 + rec::TILE) break;
            xm |= 1ull << (it - j0);
            ++cur;
        }
        if (allow) xm |= ~allow[j0 >> 6];              // (as k_rec_score: the step is one word of the packed allow set)
#pragma unroll
        for (int q = 0; q < rec::NQ; ++q) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int jl = 16 * q + M::crow(j, lane);
                const int item = j0 + jl;
                const T s = acc[q][j];
                if (!(active && item < je && !((xm >> jl) & 1ull))) continue;
                if (rec_better(s, item, best_s, best_i)) ++c_lo;
                else if (rec_better(worst_s, worst_i, s, item)) ++c_hi;
                else if (staged) {
                    const int b = rank_bucket<T>(ls, li, nr, s, item);
                    if (b >= 0) atomicAdd(&lh[b], 1);
                } else {
                    const int b = rank_bucket<T>(gs, gi, nr, s, item);
                    if (b >= 0) atomicAdd(&gh[b], 1);
                }
            }
        }
    }
    // the four lanes of a user add up their end buckets; lane group 0 holds the sums
    c_lo += __shfl_xor(c_lo, 16); c_lo += __shfl_xor(c_lo, 32);
    c_hi += __shfl_xor(c_hi, 16); c_hi += __shfl_xor(c_hi, 32);
    wave_sync();
    if (staged) {
        for (int t = g; t <= nr; t += 4) gh[t] = lh[t] + (t == 0 ? c_lo : 0) + (t == nr ? c_hi : 0);
    } else if (active && g == 0) {
        atomicAdd(&gh[0], c_lo);
        atomicAdd(&gh[nr], c_hi);
    }
}

// The counting tail over candidate rows (pcr_evaluate_ranks_filtered with cand_ptr), one wave per counted
// user, four users per workgroup: row idx of the candidate CSR (cptr / citem as k_rec_cand's) belongs to users[idx].  A step scores
// 64 candidates and hands candidate t0 + lane to lane `lane` through cand_step, the step k_rec_cand takes -- the bits k_rec_score,
// k_rank_count and k_rank_relscore give the pair.  An eligible candidate (its allow bit on, allow NULL: every
// item; not found in the item-ascending training row, xptr NULL: no exclusion) is placed into the user's sorted relevant row by
// rank_bucket and counted by an integer add: rows of at most CAND_STAGE entries are staged in the wave's LDS with their
// histogram, longer ones are searched in global memory (rs / ri, L2-resident) with a global add.  A candidate that meets itself
// in the relevant row is not counted.  One split: hist holds the batch's buckets once, zeroed by the caller, user idx's nr + 1
// starting at (rptr[idx] - rptr[0]) + idx, and k_rank_finish runs on it with nsplit = 1.  Every loop is bounded by the row's
// length, by 64 or by nr.
template <typename T>
__global__ __launch_bounds__(256) void k_cand_count(const T* __restrict__ U, const T* __restrict__ V, int r, int ld,
                                                    const int32_t* __restrict__ users, int64_t n, const int64_t* __restrict__ cptr,
                                                    const int32_t* __restrict__ citem, const unsigned long long* __restrict__ allow,
                                                    const int64_t* __restrict__ xptr, const int32_t* __restrict__ xitem,
                                                    const int64_t* __restrict__ rptr, const T* __restrict__ rs, const int32_t* __restrict__ ri,
                                                    int32_t* __restrict__ hist) {
    __shared__ T stg_[4][rec::TILE];
    __shared__ T ls_[4][rec::CAND_STAGE];
    __shared__ int li_[4][rec::CAND_STAGE];
    __shared__ int lh_[4][rec::CAND_STAGE + 1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t idx = (int64_t)blockIdx.x * 4 + w;
    if (idx >= n) return;                               // (the whole wave)
    T* stg = stg_[w];
    T* ls = ls_[w];
    int* li = li_[w];
    int* lh = lh_[w];

    const int u = users[idx];
    const int64_t nc = cptr[idx + 1] - cptr[idx];
    const int32_t* ci = citem + (cptr[idx] - cptr[0]);
    int64_t xb = 0, xe = 0;
    if (xptr) { xb = xptr[u]; xe = xptr[u + 1]; }
    const int64_t rb = rptr[idx];
    const int nr = (int)(rptr[idx + 1] - rb);           // (a counted user: nr >= 1)
    const T* gs = rs + rb;
    const int32_t* gi = ri + rb;
    int32_t* gh = hist + (size_t)(rb - rptr[0]) + (size_t)idx;
    const bool staged = nr <= rec::CAND_STAGE;          // (wave-uniform)
    if (staged) {
        for (int t = lane; t < nr; t += 64) { ls[t] = gs[t]; li[t] = gi[t]; }
        for (int t = lane; t <= nr; t += 64) lh[t] = 0;
    }
    wave_sync();

    const T* Ur = U + (size_t)(unsigned)u * (unsigned)ld;
    for (int64_t t0 = 0; t0 < nc; t0 += rec::TILE) {
        int id;
        T s;
        const bool ok = cand_step<T>(Ur, V, r, ld, ci, nc, t0, lane, stg, allow, xitem, xb, xe, id, s);
        if (ok) {
            if (staged) {
                const int b = rank_bucket<T>(ls, li, nr, s, id);
                if (b >= 0) atomicAdd(&lh[b], 1);
            } else {
                const int b = rank_bucket<T>(gs, gi, nr, s, id);
                if (b >= 0) atomicAdd(&gh[b], 1);
            }
        }
        wave_sync();                                   // (the next step overwrites stg)
    }
    if (staged) for (int t = lane; t <= nr; t += 64) gh[t] = lh[t];
}

// One wave per counted user: the splits' histograms summed and scanned.  With cum(t) = sum_{b <= t} hist[b], the t-th entry of
// the sorted relevant row has rank 1 + t + cum(t) (t relevant and cum(t) non-relevant items before it), |N_u| = cum(nr) and
// the (relevant, non-relevant) pairs in the right order number sum_t (|N_u| - cum(t)).  Writes rrank[rptr[idx] + rslot] (the
// ranks in the item-ascending order of the relevance table) and the user's row met[idx][6] = |R_u|, rr, mean_rank, mpr,
// first_rank, auc -- the column order k_topn_sum1 reduces (columns 0, 1, 2, 4 summed, column 0 > 0 counted, column 5 summed
// and counted where it is not NaN).  Every quotient is one fp64 division of two exact integers.
__global__ __launch_bounds__(256) void k_rank_finish(const int32_t* __restrict__ hist, int64_t hsplit, int nsplit, int64_t n,
                                                     const int64_t* __restrict__ rptr, const int32_t* __restrict__ rslot,
                                                     int64_t* __restrict__ rrank, double* __restrict__ met) {
    const int lane = threadIdx.x & 63;
    const int64_t idx = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (idx >= n) return;
    const int64_t rb = rptr[idx], nr = rptr[idx + 1] - rb;
    const int32_t* h = hist + (size_t)(rb - rptr[0]) + (size_t)idx;
    long long carry = 0, first = 0;
    double sum_rank = 0.0, sum_cum = 0.0;               // (integers below 2^53: exact in any order)
    for (int64_t t0 = 0; t0 <= nr; t0 += 64) {
        const int64_t t = t0 + lane;
        long long c = 0;
        if (t <= nr) for (int sp = 0; sp < nsplit; ++sp) c += h[(size_t)sp * (size_t)hsplit + (size_t)t];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const long long x = __shfl_up(c, d); if (lane >= d) c += x; }
        c += carry;
        if (t < nr) {
            const long long rank = 1 + t + c;
            rrank[rb + rslot[rb + t]] = rank;
            sum_rank += (double)rank; sum_cum += (double)c;
            if (t == 0) first = rank;
        }
        carry = __shfl(c, 63);
    }
    first = __shfl(first, 0);
    sum_rank = wave_sum(sum_rank); sum_cum = wave_sum(sum_cum);
    const double R = (double)nr, N = (double)carry;
    const double pairs = R * N, span = R * (N + R - 1.0);
    double v = R;
    if (lane == 1) v = 1.0 / (double)first;
    else if (lane == 2) v = sum_rank / R;
    else if (lane == 3) v = span > 0.0 ? (sum_rank - R) / span : 0.0;
    else if (lane == 4) v = (double)first;
    else if (lane == 5) v = pairs > 0.0 ? (pairs - sum_cum) / pairs : (double)NAN;
    if (lane < 6) met[(size_t)idx * 6 + lane] = v;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Beyond-accuracy metrics (pcr_evaluate_diversity, include/primalcr.h): item exposure, novelty and
// intra-list diversity of the merged lists.  The tables are per item: inv[j] = 1 / |V[j]| (0 for a zero row), q[j] = |v^_j|^2
// (k_div_prepare), info[j] the self-information (built on the host).
namespace rec {
constexpr int DIV_ROWS = 8;   // rows of V in flight per wave in k_rec_merge_div's walk (the gathers are latency-bound, as k_ustep's)
constexpr int DIV_CH = 2;     // components per lane and pass: a pass covers 64 DIV_CH components of the rows
}  // namespace rec

struct DivArgs {
    const double* inv;            // [d2]
    const double* q;              // [d2]
    const double* info;           // [d2]
    unsigned long long* expo;     // [ncut][d2]: row c counts the list positions in [cut[c - 1], cut[c]); made cumulative by k_div_expo_finish
    double* out;                  // [n][ncut][6]: len, novelty (0 when len = 0), 0, 0, 0, ild -- the columns k_topn_sum1 reduces
    int64_t d2;
    int ncut;
    int cut[PCR_TOPN_MAX_CUTOFFS];
};

// one wave per item: the fixed-order sum of squares of its row (lane-strided partial sums, wave_sum's butterfly), then the same
// sum over the normalised components
template <typename T>
__global__ __launch_bounds__(256) void k_div_prepare(const T* __restrict__ V, int r, int ld, int64_t d2, double* __restrict__ inv,
                                                     double* __restrict__ q) {
    const int lane = threadIdx.x & 63;
    const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= d2) return;
    const T* row = V + (size_t)j * (size_t)ld;
    double s = 0.0;
    for (int c = lane; c < r; c += 64) { const double x = (double)row[c]; s += x * x; }
    s = wave_sum(s);
    const double iv = s > 0.0 ? 1.0 / sqrt(s) : 0.0;
    double t = 0.0;
    for (int c = lane; c < r; c += 64) { const double x = (double)row[c] * iv; t += x * x; }
    t = wave_sum(t);
    if (lane == 0) { inv[j] = iv; q[j] = t; }
}

// popularity: cnt[item[z]] += 1 over the training ratings (64-bit integer adds, as the exposure: no count an int64 nnz can
// reach wraps), then the counts as doubles for the all-reduce
__global__ __launch_bounds__(256) void k_div_pop(const int32_t* __restrict__ item, int64_t nnz, unsigned long long* __restrict__ cnt) {
    for (int64_t z = (int64_t)blockIdx.x * 256 + threadIdx.x; z < nnz; z += (int64_t)gridDim.x * 256) atomicAdd(&cnt[item[z]], 1ull);
}
__global__ __launch_bounds__(256) void k_div_pop_f64(const unsigned long long* __restrict__ cnt, int64_t d2, double* __restrict__ pop) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < d2) pop[j] = (double)cnt[j];
}

// exposure rows per cutoff band -> cumulative over the cutoffs, as doubles (exact below 2^53)
__global__ __launch_bounds__(256) void k_div_expo_finish(const unsigned long long* __restrict__ expo, int64_t d2, int ncut,
                                                         double* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= d2) return;
    unsigned long long c = 0;
    for (int k = 0; k < ncut; ++k) { c += expo[(size_t)k * d2 + j]; out[(size_t)k * d2 + j] = (double)c; }
}

// k_rec_merge with the beyond-accuracy metrics fused into its tail, one wave per user: the merged list goes to the wave's LDS
// row as in k_rec_merge_topn and is never written out.  Then
//   exposure   every list position p does one integer add into the row of the first cutoff that contains p;
//   novelty    lanes own the positions p = lane, lane + 64, ...: info[] and q[] lookups, per-cutoff sums by wave_sum;
//   ILD        sum_{a<b} v^_a . v^_b = (|sum_a v^_a|^2 - sum_a q_a) / 2: the wave walks the list in position order, gathers each
//              listed row of V coalesced (lane = component, DIV_CH components per lane), scales it by inv[id] in fp64 and adds
//              it to a running vector sum in registers; at every cutoff boundary wave_sum of the squared components.  DIV_ROWS
//              rows are loaded before the first is used.  Ranks wider than 64 DIV_CH re-walk the list per component chunk (the
//              squared norm is a sum over components).  Lane c keeps cutoff c's |S|^2.
// Every value of a user depends on its list and on V alone.
// (the tail is rec_div_tail, shared with k_list_metrics: the list is sl[0, L), no padding inside, L <= the last cutoff)
template <typename T>
__device__ __forceinline__ void rec_div_tail(const int32_t* sl, int L, int64_t idx, int lane, const T* __restrict__ V, int r, int ld,
                                             const DivArgs& da) {
    double nov[PCR_TOPN_MAX_CUTOFFS], qs[PCR_TOPN_MAX_CUTOFFS];
#pragma unroll
    for (int c = 0; c < PCR_TOPN_MAX_CUTOFFS; ++c) { nov[c] = 0.0; qs[c] = 0.0; }
    for (int p = lane; p < L; p += 64) {
        const int j = sl[p];
        const double nv = da.info[j], qq = da.q[j];
        int c0 = 0;                                                  // the first cutoff that contains p (p < L <= the last cutoff)
#pragma unroll
        for (int c = 0; c < PCR_TOPN_MAX_CUTOFFS; ++c)
            if (c < da.ncut) { if (p < da.cut[c]) { nov[c] += nv; qs[c] += qq; } else c0 = c + 1; }
        atomicAdd(&da.expo[(size_t)c0 * (size_t)da.d2 + (size_t)j], 1ull);
    }
    double myn = 0.0;                                                // lane c: |sum_{a < len(c)} v^_a|^2
    for (int cb = 0; cb < r; cb += 64 * rec::DIV_CH) {
        double S[rec::DIV_CH];
#pragma unroll
        for (int t = 0; t < rec::DIV_CH; ++t) S[t] = 0.0;
        for (int i0 = 0; i0 < L; i0 += rec::DIV_ROWS) {
            T x[rec::DIV_ROWS][rec::DIV_CH];
            double iv[rec::DIV_ROWS];
#pragma unroll
            for (int e = 0; e < rec::DIV_ROWS; ++e) {
                const int j = __builtin_amdgcn_readfirstlane(i0 + e < L ? sl[i0 + e] : -1);
                iv[e] = j >= 0 ? da.inv[j] : 0.0;
#pragma unroll
                for (int t = 0; t < rec::DIV_CH; ++t) {
                    const int c = cb + 64 * t + lane;
                    x[e][t] = (j >= 0 && c < r) ? V[(size_t)(unsigned)j * (unsigned)ld + c] : (T)0;
                }
            }
#pragma unroll
            for (int e = 0; e < rec::DIV_ROWS; ++e) {
                const int cnt = i0 + e + 1;                          // entries summed after this one
                if (cnt > L) break;                                  // (wave-uniform)
#pragma unroll
                for (int t = 0; t < rec::DIV_CH; ++t) S[t] += (double)x[e][t] * iv[e];
                unsigned hit = 0;                                    // the cutoffs whose list ends here
#pragma unroll
                for (int c = 0; c < PCR_TOPN_MAX_CUTOFFS; ++c) if (c < da.ncut && cnt == min(da.cut[c], L)) hit |= 1u << c;
                if (hit) {
                    double ss = 0.0;
#pragma unroll
                    for (int t = 0; t < rec::DIV_CH; ++t) ss += S[t] * S[t];
                    ss = wave_sum(ss);
                    if (lane < PCR_TOPN_MAX_CUTOFFS && ((hit >> lane) & 1u)) myn += ss;
                }
            }
        }
    }
    double mynov = 0.0, myq = 0.0;
    int mycut = 0;
#pragma unroll
    for (int c = 0; c < PCR_TOPN_MAX_CUTOFFS; ++c) {
        if (c >= da.ncut) break;                                     // (wave-uniform)
        const double N = wave_sum(nov[c]), Q = wave_sum(qs[c]);
        if (lane == c) { mynov = N; myq = Q; mycut = da.cut[c]; }
    }
    const int len = min(mycut, L);
    const double dl = (double)len, pairs = 0.5 * dl * (dl - 1.0);
    const double ild = len >= 2 ? 1.0 - (0.5 * (myn - myq)) / pairs : (double)NAN;
    const double novelty = len >= 1 ? mynov / dl : 0.0;
    // lane l < 6 ncut writes field l % 6 of cutoff l / 6: one coalesced row per user
    const int myc = lane / 6, myf = lane - 6 * myc;
    const double f0 = __shfl(dl, myc), f1 = __shfl(novelty, myc), f5 = __shfl(ild, myc);
    if (lane < 6 * da.ncut) da.out[(size_t)idx * 6 * da.ncut + lane] = myf == 0 ? f0 : myf == 1 ? f1 : myf == 5 ? f5 : 0.0;
}
template <typename T>
__global__ __launch_bounds__(256) void k_rec_merge_div(const T* __restrict__ lst_s, const int32_t* __restrict__ lst_i,
                                                       const int32_t* __restrict__ lst_n, int nsplit, int64_t n, int K,
                                                       const T* __restrict__ V, int r, int ld, DivArgs da) {
    extern __shared__ int32_t rec_lst[];
    const int lane = threadIdx.x & 63;
    const int64_t idx = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (idx >= n) return;
    int32_t* sl = rec_lst + (size_t)(threadIdx.x >> 6) * (size_t)K;
    const int tot = rec_merge_ranks(lst_s, lst_i, lst_n, nsplit, n, K, idx, lane, [&](int rk, int j, T) { sl[rk] = j; });
    const int L = __builtin_amdgcn_readfirstlane(min(tot, K));      // the list is sl[0, L): no padding inside
    wave_sync();
    rec_div_tail<T>(sl, L, idx, lane, V, r, ld, da);
}

// Both tails over a list that is already in device memory (pcr_evaluate_lists_model, pcr_evaluate_rerank; DESIGN.md section
// 3.15), one wave per list, four lists per workgroup: lists[m][L] in list order, the non-padding entries first and -1 padding
// only after them (checked on the host, or written so by k_rec_merge_mmr).  The wave stages its list in LDS (4 L ints of dynamic
// LDS per workgroup) and runs rec_div_tail over its first min(len, last cutoff) entries -- positions past the last cutoff
// belong to no metric -- and then, when ta.rptr is given, rec_topn_tail over all L positions (the tail replaces the ids in LDS,
// so it comes second).  A user with an empty relevant row gets the row that adds nothing to k_topn_sum1's sums: zeros, with
// ndcg_graded NaN; the host counts it out.  The arithmetic is that of k_rec_merge_topn / k_rec_merge_div on the same list, bit
// for bit.
template <typename T>
__global__ __launch_bounds__(256) void k_list_metrics(const int32_t* __restrict__ lists, int64_t m, int L, const T* __restrict__ V, int r,
                                                      int ld, TopnArgs ta, DivArgs da) {
    extern __shared__ int32_t rec_lst[];
    const int lane = threadIdx.x & 63;
    const int64_t idx = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (idx >= m) return;
    int32_t* sl = rec_lst + (size_t)(threadIdx.x >> 6) * (size_t)L;
    const int32_t* gl = lists + (size_t)idx * (size_t)L;
    int len = 0;
    for (int p0 = 0; p0 < L; p0 += 64) {                            // (wave-uniform trip count)
        const int p = p0 + lane;
        const int j = p < L ? gl[p] : -1;
        if (p < L) sl[p] = j;
        len += __popcll(__ballot(j >= 0));
    }
    len = __builtin_amdgcn_readfirstlane(min(len, da.cut[da.ncut - 1]));
    wave_sync();
    rec_div_tail<T>(sl, len, idx, lane, V, r, ld, da);
    if (!ta.rptr) return;                                            // (wave-uniform)
    if (ta.rptr[idx + 1] == ta.rptr[idx]) {
        if (lane < 6 * ta.ncut) ta.out[(size_t)idx * 6 * ta.ncut + lane] = (lane % 6) == 5 ? (double)NAN : 0.0;
        return;
    }
    wave_sync();
    rec_topn_tail(sl, L, idx, lane, ta);
}

// ------------------------------------------------------------------------------------------------------------------------------
// MMR diversity re-ranking (pcr_recommend_diverse, include/primalcr.h): greedy selection of topk entries
// from the merged pool of K = pool entries, m_i = (1 - theta) (s_i - smin) - theta R max_{a in S} cos(j_i, j_a), in fp64.
namespace rec {
constexpr int MMR_ROWS = DIV_ROWS;   // streaming form: rows of V in flight per wave (one transposing butterfly reduces them together)
constexpr int MMR_PT = 4;            // LDS form: candidates a lane scores against one read of the winner's row
}  // namespace rec

struct MmrArgs {
    const double* inv;    // [d2] 1 / |V[j]| (k_div_prepare)
    int32_t* out_i;       // [n][topk]
    double* out_s;        // [n][topk]
    int topk;
    double theta;
};

// LDS form: the row stride of the staged image in elements -- an odd number of 16-byte slots, so that by the bank rule the 16
// lanes of a ds_read_b128 group, one row each, fall on 16 different slots of the 64-bank row (not confirmed by a counter run)
template <typename T>
__host__ __device__ inline int mmr_row_stride(int ld) {
    const int per = 16 / (int)sizeof(T);
    return ((ld / per) | 1) * per;
}
// LDS of one wave of k_rec_merge_mmr: the image [K][stride] (LDS form) or the winner's row [ld] doubles (streaming form), then
// c[K] doubles, the pool's scores [K] and ids [K]
template <typename T>
__host__ __device__ inline size_t mmr_wave_lds(int K, int ld, int form) {
    const size_t b = (form ? (size_t)K * mmr_row_stride<T>(ld) * sizeof(T) : (size_t)ld * sizeof(double)) +
                     (size_t)K * (sizeof(double) + sizeof(T) + sizeof(int));
    return (b + 15) & ~(size_t)15;
}

// one step of the arg-max butterfly: the larger m, equal m to the smaller position (INT_MAX: no entry)
template <int OFF>
__device__ __forceinline__ void mmr_best(double& bm, int& bp) {
    const double om = lane_xor<OFF>(bm);
    const int op = lane_xor_i<OFF>(bp);
    if (op != INT_MAX && (bp == INT_MAX || om > bm || (om == bm && op < bp))) { bm = om; bp = op; }
}

// k_rec_merge with the greedy re-ranking fused into its tail, one wave per user (blockDim.x / 64 users per workgroup): the
// merged pool goes to the wave's LDS (ids, scores) with c_i next to it.  The pool is in list order, so smin and the maximum are
// its two ends.  Each round: every lane forms m_i of its positions p = lane, lane + 64, ... (ascending, strict compare: the
// smaller position keeps a tie), a fixed xor butterfly picks the winner, lane 0 writes it out and marks it (id -> -1 - id), then
// c_i = max(c_i, cos(j_i, j_w)) for the entries left, cos = (sum_c V[j_i][c] V[j_w][c]) (inv[j_i] inv[j_w]) with every product
// and sum in fp64.  theta R = 0 needs no cosine at all.
//   FORM 0 (streaming)  lane = component: the winner's row sits in LDS as doubles; MMR_ROWS candidate rows are gathered coalesced
//          from global memory before the first is used, their partial dot products are reduced together by a transposing
//          butterfly (8 -> 4 -> 2 -> 1 values per lane over xor 32, 16, 8, then xor 4, 2, 1) and lanes 0, 8, ..., 56 update one
//          candidate each.
//   FORM 1 (LDS)        lane = candidate: the pool's rows are staged once into the image (padding components zeroed); a lane
//          walks its candidates' rows 16 bytes at a time against a broadcast read of the winner's row, MMR_PT candidates per read.
// Both forms add the products of a pair in an order fixed by the code; a row depends on its pool and V alone.
template <typename T, int FORM>
__global__ __launch_bounds__(256) void k_rec_merge_mmr(const T* __restrict__ lst_s, const int32_t* __restrict__ lst_i,
                                                       const int32_t* __restrict__ lst_n, int nsplit, int64_t n, int K,
                                                       const T* __restrict__ V, int r, int ld, MmrArgs ma) {
    typedef typename RecMma<T>::vec_t vec_t;
    constexpr int PER = RecMma<T>::KV;                               // elements per 16 bytes
    extern __shared__ __align__(16) char rec_lds[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t idx = (int64_t)blockIdx.x * (blockDim.x >> 6) + w;
    if (idx >= n) return;
    const int rs = mmr_row_stride<T>(ld);
    char* wl = rec_lds + (size_t)w * mmr_wave_lds<T>(K, ld, FORM);
    T* img = (T*)wl;
    double* wr = (double*)wl;
    double* cc = (double*)(wl + (FORM ? (size_t)K * rs * sizeof(T) : (size_t)ld * sizeof(double)));
    T* ss = (T*)(cc + K);
    int* si = (int*)(ss + K);
    const int tot = rec_merge_ranks(lst_s, lst_i, lst_n, nsplit, n, K, idx, lane, [&](int rk, int j, T s) { si[rk] = j; ss[rk] = s; });
    const int L = __builtin_amdgcn_readfirstlane(min(tot, K));      // the pool is [0, L): no padding inside
    const int rounds = min(ma.topk, L);
    int32_t* oi = ma.out_i + (size_t)idx * ma.topk;
    double* os = ma.out_s + (size_t)idx * ma.topk;
    for (int p = rounds + lane; p < ma.topk; p += 64) { oi[p] = -1; os[p] = -INFINITY; }
    if (L == 0) return;
    wave_sync();
    for (int p = lane; p < L; p += 64) cc[p] = -INFINITY;
    if (FORM) {
        const int nv = ld / PER;
#pragma unroll 4
        for (int e = lane; e < L * nv; e += 64) {
            const int p = e / nv, v = e - p * nv;
            vec_t x = *(const vec_t*)(V + (size_t)(unsigned)si[p] * (unsigned)ld + v * PER);
#pragma unroll
            for (int q = 0; q < PER; ++q) if (v * PER + q >= r) x[q] = (T)0;
            *(vec_t*)(img + (size_t)p * rs + v * PER) = x;
        }
    }
    const double smin = (double)ss[L - 1];
    double R = (double)ss[0] - smin;
    if (R == 0.0) R = 1.0;
    const double a = 1.0 - ma.theta, b = ma.theta * R;
    wave_sync();
    for (int t = 0; t < rounds; ++t) {
        const bool usec = t > 0 && b != 0.0;                         // (c_i = 0 while S is empty)
        double bm = -INFINITY;
        int bp = INT_MAX;
        for (int p = lane; p < L; p += 64) {
            if (si[p] < 0) continue;
            double m = a * ((double)ss[p] - smin);
            if (usec) m -= b * cc[p];
            if (!(m == m)) m = -INFINITY;                            // (a total order whatever the factors hold)
            if (bp == INT_MAX || m > bm) { bm = m; bp = p; }
        }
        mmr_best<32>(bm, bp); mmr_best<16>(bm, bp); mmr_best<8>(bm, bp); mmr_best<4>(bm, bp); mmr_best<2>(bm, bp); mmr_best<1>(bm, bp);
        const int wp = __builtin_amdgcn_readfirstlane(bp);
        if (wp < 0 || wp >= L) break;                                // (cannot happen: rounds <= L entries are left)
        const int jw = __builtin_amdgcn_readfirstlane(si[wp]);
        wave_sync();
        if (lane == 0) { oi[t] = jw; os[t] = (double)ss[wp]; si[wp] = -1 - jw; }
        wave_sync();
        if (t + 1 == rounds || b == 0.0) continue;                   // (wave-uniform)
        const double invw = ma.inv[jw];
        if (FORM) {
            const int nv = ld / PER;
            const T* wrow = img + (size_t)wp * rs;
            for (int p0 = 0; p0 < L; p0 += 64 * rec::MMR_PT) {
                double acc[rec::MMR_PT];
                const T* row[rec::MMR_PT];
                int id[rec::MMR_PT];
#pragma unroll
                for (int e = 0; e < rec::MMR_PT; ++e) {
                    const int p = p0 + 64 * e + lane;
                    id[e] = p < L ? si[p] : -1;
                    row[e] = img + (size_t)(id[e] >= 0 ? p : wp) * rs;
                    acc[e] = 0.0;
                }
                for (int v = 0; v < nv; ++v) {
                    const vec_t xw = *(const vec_t*)(wrow + v * PER);
#pragma unroll
                    for (int e = 0; e < rec::MMR_PT; ++e) {
                        if (p0 + 64 * e >= L) break;                 // (wave-uniform)
                        const vec_t x = *(const vec_t*)(row[e] + v * PER);
#pragma unroll
                        for (int q = 0; q < PER; ++q) acc[e] += (double)x[q] * (double)xw[q];
                    }
                }
#pragma unroll
                for (int e = 0; e < rec::MMR_PT; ++e) {
                    const int p = p0 + 64 * e + lane;
                    if (id[e] >= 0) cc[p] = fmax(cc[p], acc[e] * (ma.inv[id[e]] * invw));
                }
            }
        } else {
            static_assert(rec::MMR_ROWS == 8, "the transposing butterfly below reduces eight rows");
            for (int c = lane; c < ld; c += 64) wr[c] = c < r ? (double)V[(size_t)(unsigned)jw * (unsigned)ld + c] : 0.0;
            wave_sync();
            for (int i0 = 0; i0 < L; i0 += rec::MMR_ROWS) {
                double acc[rec::MMR_ROWS];
                int id[rec::MMR_ROWS];
                bool any = false;
#pragma unroll
                for (int e = 0; e < rec::MMR_ROWS; ++e) {
                    id[e] = __builtin_amdgcn_readfirstlane(i0 + e < L ? si[i0 + e] : -1);
                    any = any || id[e] >= 0;
                    acc[e] = 0.0;
                }
                if (!any) continue;                                  // (wave-uniform)
                for (int cb = 0; cb < r; cb += 64 * rec::DIV_CH) {
                    T x[rec::MMR_ROWS][rec::DIV_CH];
#pragma unroll
                    for (int e = 0; e < rec::MMR_ROWS; ++e)
#pragma unroll
                        for (int q = 0; q < rec::DIV_CH; ++q) {
                            const int c = cb + 64 * q + lane;
                            x[e][q] = (id[e] >= 0 && c < r) ? V[(size_t)(unsigned)id[e] * (unsigned)ld + c] : (T)0;
                        }
#pragma unroll
                    for (int q = 0; q < rec::DIV_CH; ++q) {
                        const int c = cb + 64 * q + lane;
                        const double wv = c < r ? wr[c] : 0.0;
#pragma unroll
                        for (int e = 0; e < rec::MMR_ROWS; ++e) acc[e] += (double)x[e][q] * wv;
                    }
                }
                // eight sums over the 64 lanes at once: each xor step halves the values a lane carries
                const bool h32 = (lane & 32) != 0, h16 = (lane & 16) != 0, h8 = (lane & 8) != 0;
                double a4[4], a2[2];
#pragma unroll
                for (int e = 0; e < 4; ++e) a4[e] = (h32 ? acc[e + 4] : acc[e]) + lane_xor<32>(h32 ? acc[e] : acc[e + 4]);
#pragma unroll
                for (int e = 0; e < 2; ++e) a2[e] = (h16 ? a4[e + 2] : a4[e]) + lane_xor<16>(h16 ? a4[e] : a4[e + 2]);
                double a1 = (h8 ? a2[1] : a2[0]) + lane_xor<8>(h8 ? a2[0] : a2[1]);
                a1 += lane_xor<4>(a1);
                a1 += lane_xor2(a1);
                a1 += lane_xor1(a1);
                const int p = i0 + (h32 ? 4 : 0) + (h16 ? 2 : 0) + (h8 ? 1 : 0);   // the candidate this lane's sum belongs to
                if ((lane & 7) == 0 && p < L) {
                    const int j = si[p];
                    if (j >= 0) cc[p] = fmax(cc[p], a1 * (ma.inv[j] * invw));
                }
            }
        }
        wave_sync();
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// Group-capped top-K (pcr_recommend_capped, include/primalcr.h): the first topk entries of the merged
// pool of K = pool entries that are kept by the rule "at most cap entries of one group"; group[j] < 0: item j is never capped.

// LDS of one wave of k_rec_merge_cap: the pool's scores [K], ids [K] and group ids [K]
template <typename T>
__host__ __device__ inline size_t cap_wave_lds(int K) {
    const size_t b = (size_t)K * (sizeof(T) + 2 * sizeof(int));
    return (b + 15) & ~(size_t)15;
}

// k_rec_merge with the selection fused into its tail, one wave per user, four users per workgroup: the merged pool goes to the
// wave's LDS (ids, scores) with group[j_i] next to it.  The wave then walks the pool 64 positions at a time: lane p counts the
// earlier positions e < p with its group id -- broadcast LDS reads over e = 0 .. the chunk's last position, the same trip count
// for every lane, a lane adding only while its count is below cap -- and keeps its entry when the count stays below cap (or its
// group id is negative).  A ballot and the popcount of the lanes below give every kept entry its output slot behind the kept
// entries of the chunks before, a wave-uniform number; the walk ends as soon as that number reaches topk.  The scores are copied
// (converted to double), nothing is computed from them: a row depends on its pool, group[] and cap alone.
// status[idx] (NULL: not written): PCR_CAP_EXACT when the row holds topk items or the pool is shorter than K (it is the user's
// whole eligible catalogue), PCR_CAP_POOL_EXHAUSTED otherwise.
template <typename T>
__global__ __launch_bounds__(256) void k_rec_merge_cap(const T* __restrict__ lst_s, const int32_t* __restrict__ lst_i,
                                                       const int32_t* __restrict__ lst_n, int nsplit, int64_t n, int K,
                                                       const int32_t* __restrict__ group, int cap, int topk,
                                                       int32_t* __restrict__ out_i, double* __restrict__ out_s,
                                                       unsigned char* __restrict__ out_st) {
    extern __shared__ __align__(16) char rec_lds[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t idx = (int64_t)blockIdx.x * 4 + w;
    if (idx >= n) return;                               // (the whole wave)
    char* wl = rec_lds + (size_t)w * cap_wave_lds<T>(K);
    T* ss = (T*)wl;
    int* si = (int*)(ss + K);
    int* sg = si + K;
    const int tot = rec_merge_ranks(lst_s, lst_i, lst_n, nsplit, n, K, idx, lane, [&](int rk, int j, T s) {
        si[rk] = j; ss[rk] = s; sg[rk] = group[j];
    });
    const int L = __builtin_amdgcn_readfirstlane(min(tot, K));      // the pool is [0, L): no padding inside
    int32_t* oi = out_i + (size_t)idx * topk;
    double* os = out_s + (size_t)idx * topk;
    wave_sync();
    int kept = 0;                                                    // (wave-uniform)
    for (int c0 = 0; c0 < L && kept < topk; c0 += 64) {
        const int p = c0 + lane;
        const int g = p < L ? sg[p] : -1;
        const int ce = min(L, c0 + 64) - 1;                          // positions before the chunk's last one
        int cnt = 0;
        for (int e = 0; e < ce; ++e) cnt += (e < p && cnt < cap && sg[e] == g) ? 1 : 0;
        const bool keep = p < L && (g < 0 || cnt < cap);
        const unsigned long long km = __ballot(keep);
        const int slot = kept + __popcll(km & ((1ull << lane) - 1ull));
        if (keep && slot < topk) { oi[slot] = si[p]; os[slot] = (double)ss[p]; }
        kept += __popcll(km);
    }
    kept = min(kept, topk);
    for (int p = kept + lane; p < topk; p += 64) { oi[p] = -1; os[p] = -INFINITY; }
    if (out_st && lane == 0) out_st[idx] = (kept == topk || L < K) ? PCR_CAP_EXACT : PCR_CAP_POOL_EXHAUSTED;
}
