// pcr_ccd.h -- CCDR1 (CCD++ rank-one squared-loss matrix factorisation, solver type 0) on the device: ccd-r1.cpp:97-212.
//
// Included by pcr_solver.hip after Solver<T>: a CcdSolver<T> holds a Solver<T> for what the two solvers share -- the factor
// storage (U d1 x ld, V d2 x ld, row-major, the storage type T), the test-set evaluator (k_eval / k_eval2, util.cpp:434-542)
// and the stream -- and keeps its own state next to it:
//   * the residual over the training ratings twice, in user-major (CSR) order and in item-major (CSC) order, so that both
//     sweeps read it sequentially.  The two copies are updated by the same expression (an explicit fma with the same operands)
//     on both sides and stay bitwise identical (pcr_solver_counter "ccd_residual_mismatch" checks it);
//   * the test residuals behind the printed rmse (util.cpp:206-215);
//   * fp64 work vectors u (d1), v (d2) and their values at the start of the rank, oldu / oldv (ccd-r1.cpp:120-125);
//   * a control block (CcdCtl): the stopping state of ccd-r1.cpp:126-172 lives on the device, so that no inner iteration
//     needs a host round trip;
//   * optionally one confidence weight per rating (pcr_solver_set_rating_weights): in both orders next to the two
//     residual copies, in their storage type, and the fp64 sums W per user and per item that stand where the rating counts stood;
//     the weighted launches are the _w kernels, the unweighted ones keep their symbols and code;
//   * optionally a weight alpha on every UNRATED cell (pcr_solver_set_implicit): kernels of their own (_i) further
//     down, 7 T + 5 launches per rank.
// Kernels per rank: k_ccd_begin, then per inner iteration k_ccd_sweep over the CSC (v), k_ccd_sweep over the
// CSR (u) and k_ccd_decide, then k_ccd_resid and k_ccd_final: 3 T + 3 launches.  Every sum is accumulated in fp64 and reduced in
// a fixed order (per-block partials summed by one block): results do not depend on timing and repeat bit for bit.
#pragma once

struct CcdCtl {
    // stopping state (ccd-r1.cpp:126-129, :165-172)
    double fundec_max, rankfundec;
    int early_stop, broken, skip, pad0;
    // objective bookkeeping (ccd-r1.cpp:110-118, :181-199)
    double reg, loss, obj, oldobj, rmse;
    // counters: inner iterations executed, ranks executed (cumulative since the start of training)
    long long inner_iters, ranks_done;
    // the record of the last rank: 1 if it ran (a skipped rank prints nothing)
    int printed, pad1;
};

namespace ccd {
constexpr int BLOCK = 256;          // 4 waves
constexpr int LONG = 4096;          // columns with more ratings than this get a whole workgroup (Netflix-shaped long tails)
constexpr int PART_MAX = 1024;      // blocks of the element-wise segments (fixed by the shape, never by the device)

__device__ inline long long bits(double x) { return __double_as_longlong(x); }
__device__ inline long long bits(float x) { return __float_as_int(x); }
__device__ inline double wave_sum(double x) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}
// fixed-order sum of a[0..n) by one block: thread j sums j, j + B, ... in order, then a tree over the threads
__device__ inline double block_sum_fixed(const double* a, int n, double* lds) {
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += BLOCK) s += a[i];
    lds[threadIdx.x] = s;
    __syncthreads();
    for (int w = BLOCK / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) lds[threadIdx.x] += lds[threadIdx.x + w];
        __syncthreads();
    }
    const double r = lds[0];
    __syncthreads();
    return r;
}
__device__ inline double block_reduce(double s, double* lds) {
    lds[threadIdx.x] = s;
    __syncthreads();
    for (int w = BLOCK / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) lds[threadIdx.x] += lds[threadIdx.x + w];
        __syncthreads();
    }
    const double r = lds[0];
    __syncthreads();
    return r;
}
// RankOneUpdate's closing arithmetic (ccd-r1.cpp:7-30) for a non-empty column; *fundec receives the column's term
__device__ inline double rank_one_new(double g, double h, double vj, int do_nmf, double* fundec) {
    const double newvj = g / h;
    if (do_nmf > 0 && newvj < 0) {
        // ccd-r1.cpp:19: `fundec = -2*g*vj; + h*vj*vj;` -- the stray semicolon drops the h term; reproduced
        *fundec = -2 * g * vj;
        return 0.0;
    }
    const double delta = vj - newvj;
    *fundec = h * delta * delta;
    return newvj;
}
}  // namespace ccd

// Start of rank t (ccd-r1.cpp:113-125): u = oldu = U[:, t]; v = V[:, t], oldv = 0 in outer iteration 1 (:124), else v.
// Rank 1 of an outer iteration resets fundec_max and early_stop (:126-129); a rank after five first-iteration breaks is
// skipped (:131) -- every later kernel of the rank exits at entry.
template <typename T>
__global__ void __launch_bounds__(ccd::BLOCK) k_ccd_begin(CcdCtl* ctl, const T* U, const T* V, int ld, int t, int oiter, int64_t d1, int64_t d2,
                                                          double* u, double* oldu, double* v, double* oldv) {
    const bool skip = t > 0 && ctl->early_stop >= 5;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (t == 0) { ctl->fundec_max = 0.0; ctl->rankfundec = 0.0; ctl->early_stop = 0; }
        ctl->broken = 0;
        ctl->skip = skip ? 1 : 0;
    }
    if (skip) return;
    const int64_t n = d1 > d2 ? d1 : d2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (i < d1) { const double x = (double)U[i * ld + t]; u[i] = x; oldu[i] = x; }
        if (i < d2) { const double x = (double)V[i * ld + t]; v[i] = x; oldv[i] = oiter == 1 ? 0.0 : x; }
    }
}

// One half of an inner iteration (ccd-r1.cpp:146-160): for every column c of the given orientation (items over the CSC for v,
// users over the CSR for u) y[c] = g / h with g = sum x_i r_ic, h = lambda * n_c + sum x_i^2 (:151,157: the regulariser is
// lambda times the column's rating count), 0 for an empty column.  Short columns: one wave each, four per workgroup; long ones:
// a workgroup each.  With `addback` (inner iteration 1 of an outer iteration > 1) the rank's old term is added back into this
// orientation's residual copy on the way (ccd-r1.cpp:127-130: r += oldu_i oldv_j), stored, and used.
// part[block] = the block's fundec, its columns in order.
// With WT (per-rating confidence weights c_z) wt holds c in this orientation's order, read at the residual's index,
// and Wc[c] = the column's sum of c_z: g = sum (c x) r, h = lambda W_c + sum (c x) x -- c x is formed first, so all-ones weights
// give the unweighted bits and weights that are all the same power of two scale g, h and fundec exactly.  An empty column is
// still decided by its count.
template <typename RT, bool WT>
__device__ __forceinline__ void ccd_sweep(const CcdCtl* ctl, const int64_t* ptr, const int32_t* idx, RT* res, const RT* wt, const double* Wc,
                                          const double* x, const double* oldx, const double* oldy, double* y, const int32_t* longs, int nlong,
                                          const int32_t* shorts, int nshort, double lambda, int do_nmf, int addback, double* part) {
    if (ctl->skip || ctl->broken) return;
    __shared__ double sg[ccd::BLOCK / 64], sh[ccd::BLOCK / 64], sf[ccd::BLOCK / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if ((int)blockIdx.x < nlong) {
        const int c = longs[blockIdx.x];
        const int64_t z0 = ptr[c], z1 = ptr[c + 1];
        const double oy = oldy[c];
        double g = 0.0, h = 0.0;
        for (int64_t z = z0 + threadIdx.x; z < z1; z += ccd::BLOCK) {
            const int i = idx[z];
            double r = (double)res[z];
            if (addback) { const RT rn = (RT)fma(oldx[i], oy, r); res[z] = rn; r = (double)rn; }
            const double xi = x[i];
            if (WT) { const double cx = (double)wt[z] * xi; g += cx * r; h += cx * xi; }
            else { g += xi * r; h += xi * xi; }
        }
        g = ccd::wave_sum(g); h = ccd::wave_sum(h);
        if (lane == 0) { sg[wv] = g; sh[wv] = h; }
        __syncthreads();
        if (threadIdx.x == 0) {
            double G = 0.0, H = 0.0;
            for (int w = 0; w < ccd::BLOCK / 64; ++w) { G += sg[w]; H += sh[w]; }
            double f = 0.0;
            y[c] = ccd::rank_one_new(G, lambda * (WT ? Wc[c] : (double)(z1 - z0)) + H, y[c], do_nmf, &f);
            part[blockIdx.x] = f;
        }
        return;
    }
    const int64_t s = (int64_t)(blockIdx.x - nlong) * (ccd::BLOCK / 64) + wv;
    double f = 0.0;
    if (s < nshort) {
        const int c = shorts[s];
        const int64_t z0 = ptr[c], z1 = ptr[c + 1];
        const double oy = oldy[c];
        double g = 0.0, h = 0.0;
        for (int64_t z = z0 + lane; z < z1; z += 64) {
            const int i = idx[z];
            double r = (double)res[z];
            if (addback) { const RT rn = (RT)fma(oldx[i], oy, r); res[z] = rn; r = (double)rn; }
            const double xi = x[i];
            if (WT) { const double cx = (double)wt[z] * xi; g += cx * r; h += cx * xi; }
            else { g += xi * r; h += xi * xi; }
        }
        g = ccd::wave_sum(g); h = ccd::wave_sum(h);
        if (lane == 0) {
            if (z1 > z0) y[c] = ccd::rank_one_new(g, lambda * (WT ? Wc[c] : (double)(z1 - z0)) + h, y[c], do_nmf, &f);
            else y[c] = 0.0;                                             // ccd-r1.cpp:9: an empty column returns 0, no fundec
        }
    }
    if (lane == 0) sf[wv] = f;
    __syncthreads();
    if (threadIdx.x == 0) {
        double F = 0.0;
        for (int w = 0; w < ccd::BLOCK / 64; ++w) F += sf[w];
        part[blockIdx.x] = F;
    }
}
template <typename RT>
__global__ void __launch_bounds__(ccd::BLOCK) k_ccd_sweep(const CcdCtl* ctl, const int64_t* ptr, const int32_t* idx, RT* res, const double* x,
                                                          const double* oldx, const double* oldy, double* y, const int32_t* longs, int nlong,
                                                          const int32_t* shorts, int nshort, double lambda, int do_nmf, int addback, double* part) {
    ccd_sweep<RT, false>(ctl, ptr, idx, res, nullptr, nullptr, x, oldx, oldy, y, longs, nlong, shorts, nshort, lambda, do_nmf, addback, part);
}
template <typename RT>
__global__ void __launch_bounds__(ccd::BLOCK) k_ccd_sweep_w(const CcdCtl* ctl, const int64_t* ptr, const int32_t* idx, RT* res, const RT* wt,
                                                            const double* Wc, const double* x, const double* oldx, const double* oldy, double* y,
                                                            const int32_t* longs, int nlong, const int32_t* shorts, int nshort, double lambda,
                                                            int do_nmf, int addback, double* part) {
    ccd_sweep<RT, true>(ctl, ptr, idx, res, wt, Wc, x, oldx, oldy, y, longs, nlong, shorts, nshort, lambda, do_nmf, addback, part);
}

// The stopping test after both sweeps of inner iteration `iter` (ccd-r1.cpp:161-172): innerfundec_cur = v-side + u-side sums;
// below fundec_max * eps the rank breaks (its later sweeps exit at entry; a break at iteration 1 counts towards early_stop);
// else fundec_max takes it, except at (outer 1, rank 1, inner 1) (:170-172).  The updated u and v are kept either way.
__global__ void __launch_bounds__(ccd::BLOCK) k_ccd_decide(CcdCtl* ctl, const double* vpart, int nv, const double* upart, int nu, double eps,
                                                           int oiter, int t, int iter) {
    if (ctl->skip || ctl->broken) return;
    __shared__ double lds[ccd::BLOCK];
    const double cur = ccd::block_sum_fixed(vpart, nv, lds) + ccd::block_sum_fixed(upart, nu, lds);
    if (threadIdx.x != 0) return;
    ctl->inner_iters += 1;
    if (cur < ctl->fundec_max * eps) {
        if (iter == 1) ctl->early_stop += 1;
        ctl->broken = 1;
        return;
    }
    ctl->rankfundec += cur;
    if (!(oiter == 1 && t == 0 && iter == 1)) ctl->fundec_max = fmax(ctl->fundec_max, cur);
}

// End of the rank (ccd-r1.cpp:175-199), element-wise segments of one launch, each with per-block partials:
//   blocks [0, B):        CSR copy  r -= u_i v_j, loss partials (the reference's loss is the sum over its CSR-ordered copy, :182)
//   blocks [B, 2B):       CSC copy  r -= u_i v_j (same expression, same operands: the copies stay bitwise identical)
//   blocks [2B, 2B + Bu): users: U[:, t] = u (rounded to the storage type: every later use, here included, sees the stored value),
//                         reg partials nnz_i (u_i^2 - oldu_i^2) (:187-194)
//   blocks [.., + Bv):    items: V[:, t] = v, reg partials
//   blocks [.., + Bt):    test residuals tv -= u_i v_j - oldu_i oldv_j and their squares (util.cpp:206-215)
// With WT: wt_r = the weights in CSR order (the loss is sum (c r) r over the CSR copy), Wu / Wv = the per-user / per-item sums of
// c_z in the place of the counts in the reg partials; the residuals and the test segment do not see weights.
template <typename T, typename RT, bool WT>
__device__ __forceinline__ void ccd_resid(const CcdCtl* ctl, int B, int Bu, int Bv, int Bt, int64_t nnz, int64_t d1, int64_t d2, int64_t tn,
                                          RT* res_r, const int32_t* row_r, const int32_t* col_r, RT* res_c, const int32_t* row_c,
                                          const int32_t* col_c, const int64_t* uptr, const int64_t* cptr, const RT* wt_r, const double* Wu,
                                          const double* Wv, const double* u, const double* oldu, const double* v, const double* oldv, T* U, T* V,
                                          int ld, int t, const int32_t* tu, const int32_t* ti, double* tres, double* p_loss, double* p_regu,
                                          double* p_regv, double* p_rmse, int addback) {
    if (ctl->skip) return;
    __shared__ double lds[ccd::BLOCK];
    int b = blockIdx.x;
    double s = 0.0;
    double* out = nullptr;
    if (b < 2 * B) {
        const bool csr = b < B;
        if (!csr) b -= B;
        RT* res = csr ? res_r : res_c;
        const int32_t* rr = csr ? row_r : row_c;       // user of every entry
        const int32_t* cc = csr ? col_r : col_c;       // item of every entry
        for (int64_t z = (int64_t)b * ccd::BLOCK + threadIdx.x; z < nnz; z += (int64_t)B * ccd::BLOCK) {
            const double ui = (double)(T)u[rr[z]], vj = (double)(T)v[cc[z]];
            RT r0 = res[z];
            if (addback) r0 = (RT)fma(oldu[rr[z]], oldv[cc[z]], (double)r0);   // no inner iteration ran (-T 0): the add-back is here
            const RT rn = (RT)fma(-ui, vj, (double)r0);
            res[z] = rn;
            const double r = (double)rn;
            if (WT) { if (csr) s += ((double)wt_r[z] * r) * r; }
            else s += r * r;
        }
        if (!csr) return;
        out = p_loss;
    } else if ((b -= 2 * B) < Bu) {
        for (int64_t i = (int64_t)b * ccd::BLOCK + threadIdx.x; i < d1; i += (int64_t)Bu * ccd::BLOCK) {
            const T x = (T)u[i];
            U[i * ld + t] = x;
            const double n = WT ? Wu[i] : (double)(uptr[i + 1] - uptr[i]), xd = (double)x;
            s += n * (xd * xd) - n * (oldu[i] * oldu[i]);
        }
        out = p_regu;
    } else if ((b -= Bu) < Bv) {
        for (int64_t j = (int64_t)b * ccd::BLOCK + threadIdx.x; j < d2; j += (int64_t)Bv * ccd::BLOCK) {
            const T x = (T)v[j];
            V[j * ld + t] = x;
            const double n = WT ? Wv[j] : (double)(cptr[j + 1] - cptr[j]), xd = (double)x;
            s += n * xd * xd - n * oldv[j] * oldv[j];
        }
        out = p_regv;
    } else {
        b -= Bv;
        for (int64_t z = (int64_t)b * ccd::BLOCK + threadIdx.x; z < tn; z += (int64_t)Bt * ccd::BLOCK) {
            const int i = tu[z], j = ti[z];
            if (i < 0) { s += tres[z] * tres[z]; continue; }            // (a user id past d1: see CcdSolver::init)
            const double r = tres[z] - ((double)(T)u[i] * (double)(T)v[j] - oldu[i] * oldv[j]);
            tres[z] = r;
            s += r * r;
        }
        out = p_rmse;
    }
    s = ccd::block_reduce(s, lds);
    if (threadIdx.x == 0) out[b] = s;
}
template <typename T, typename RT>
__global__ void __launch_bounds__(ccd::BLOCK) k_ccd_resid(const CcdCtl* ctl, int B, int Bu, int Bv, int Bt, int64_t nnz, int64_t d1, int64_t d2, int64_t tn,
                                                          RT* res_r, const int32_t* row_r, const int32_t* col_r,
                                                          RT* res_c, const int32_t* row_c, const int32_t* col_c,
                                                          const int64_t* uptr, const int64_t* cptr, const double* u, const double* oldu,
                                                          const double* v, const double* oldv, T* U, T* V, int ld, int t,
                                                          const int32_t* tu, const int32_t* ti, double* tres,
                                                          double* p_loss, double* p_regu, double* p_regv, double* p_rmse, int addback) {
    ccd_resid<T, RT, false>(ctl, B, Bu, Bv, Bt, nnz, d1, d2, tn, res_r, row_r, col_r, res_c, row_c, col_c, uptr, cptr, nullptr, nullptr, nullptr,
                            u, oldu, v, oldv, U, V, ld, t, tu, ti, tres, p_loss, p_regu, p_regv, p_rmse, addback);
}
template <typename T, typename RT>
__global__ void __launch_bounds__(ccd::BLOCK) k_ccd_resid_w(const CcdCtl* ctl, int B, int Bu, int Bv, int Bt, int64_t nnz, int64_t d1, int64_t d2,
                                                            int64_t tn, RT* res_r, const int32_t* row_r, const int32_t* col_r, RT* res_c,
                                                            const int32_t* row_c, const int32_t* col_c, const int64_t* uptr, const int64_t* cptr,
                                                            const RT* wt_r, const double* Wu, const double* Wv, const double* u, const double* oldu,
                                                            const double* v, const double* oldv, T* U, T* V, int ld, int t, const int32_t* tu,
                                                            const int32_t* ti, double* tres, double* p_loss, double* p_regu, double* p_regv,
                                                            double* p_rmse, int addback) {
    ccd_resid<T, RT, true>(ctl, B, Bu, Bv, Bt, nnz, d1, d2, tn, res_r, row_r, col_r, res_c, row_c, col_c, uptr, cptr, wt_r, Wu, Wv, u, oldu, v,
                           oldv, U, V, ld, t, tu, ti, tres, p_loss, p_regu, p_regv, p_rmse, addback);
}

// The rank's record (ccd-r1.cpp:180-199): reg += the item side then the user side, obj = loss + lambda reg, rmse over the test
// entries; oldobj carries over to the next rank
__global__ void __launch_bounds__(ccd::BLOCK) k_ccd_final(CcdCtl* ctl, const double* p_loss, int B, const double* p_regu, int Bu, const double* p_regv,
                                                          int Bv, const double* p_rmse, int Bt, int64_t tn, double lambda) {
    __shared__ double lds[ccd::BLOCK];
    if (ctl->skip) {
        if (threadIdx.x == 0) ctl->printed = 0;
        return;
    }
    const double loss = ccd::block_sum_fixed(p_loss, B, lds);
    const double rv = ccd::block_sum_fixed(p_regv, Bv, lds);
    const double ru = ccd::block_sum_fixed(p_regu, Bu, lds);
    const double se = ccd::block_sum_fixed(p_rmse, Bt, lds);
    if (threadIdx.x != 0) return;
    ctl->reg += rv;
    ctl->reg += ru;
    ctl->loss = loss;
    ctl->oldobj = ctl->obj;
    ctl->obj = loss + ctl->reg * lambda;
    ctl->rmse = tn > 0 ? sqrt(se / (double)tn) : 0.0;
    ctl->ranks_done += 1;
    ctl->printed = 1;
}

// Start of training (ccd-r1.cpp:107-118): V = 0 (the reference zeroes H), residuals = ratings, test residuals = test ratings
// (uploaded by the host), reg partials = sum_i nnz_i sum_t U_it^2
// (WT: sum_i W_i sum_t U_it^2, W_i = the user's sum of c_z)
template <typename T, bool WT>
__device__ __forceinline__ void ccd_init(T* V, int64_t nV, const T* U, int k, int ld, const int64_t* uptr, const double* Wu, int64_t d1, double* p_reg) {
    __shared__ double lds[ccd::BLOCK];
    for (int64_t i = (int64_t)blockIdx.x * ccd::BLOCK + threadIdx.x; i < nV; i += (int64_t)gridDim.x * ccd::BLOCK) V[i] = (T)0;
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * ccd::BLOCK + threadIdx.x; i < d1; i += (int64_t)gridDim.x * ccd::BLOCK) {
        const double n = WT ? Wu[i] : (double)(uptr[i + 1] - uptr[i]);
        for (int t = 0; t < k; ++t) { const double x = (double)U[i * ld + t]; s += x * x * n; }
    }
    s = ccd::block_reduce(s, lds);
    if (threadIdx.x == 0) p_reg[blockIdx.x] = s;
}
template <typename T>
__global__ void __launch_bounds__(ccd::BLOCK) k_ccd_init(T* V, int64_t nV, const T* U, int k, int ld, const int64_t* uptr, int64_t d1, double* p_reg) {
    ccd_init<T, false>(V, nV, U, k, ld, uptr, nullptr, d1, p_reg);
}
template <typename T>
__global__ void __launch_bounds__(ccd::BLOCK) k_ccd_init_w(T* V, int64_t nV, const T* U, int k, int ld, const int64_t* uptr, const double* Wu, int64_t d1,
                                                           double* p_reg) {
    ccd_init<T, true>(V, nV, U, k, ld, uptr, Wu, d1, p_reg);
}
__global__ void __launch_bounds__(ccd::BLOCK) k_ccd_init_fin(CcdCtl* ctl, const double* p_reg, int n) {
    __shared__ double lds[ccd::BLOCK];
    const double reg = ccd::block_sum_fixed(p_reg, n, lds);
    if (threadIdx.x != 0) return;
    ctl->fundec_max = 0.0; ctl->rankfundec = 0.0;
    ctl->early_stop = 0; ctl->broken = 0; ctl->skip = 0;
    ctl->reg = reg; ctl->loss = 0.0; ctl->obj = 0.0; ctl->oldobj = 0.0; ctl->rmse = 0.0;
    ctl->inner_iters = 0; ctl->ranks_done = 0; ctl->printed = 0;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Implicit feedback (pcr_solver_set_implicit): every unrated cell is a rating 0 of weight alpha.  The sums over all
// d1 x d2 cells are never formed: with x the other side's work vector and s = Fother^T x (a k-vector), the all-cells sum of
// x_i p^_ic of column c (p^ = the prediction without rank t) is q_c = sum_{s != t} F[c, s] s[s], and the all-cells sum of x^2 is
// one number Sxx; the rated cells are then taken back out of both next to the residual:
//   g = sum_Omega (c x) r^ - alpha (q_c - sum_Omega x p^),   h = lambda W_c + sum_Omega (c - alpha) x^2 + alpha Sxx,
// with p^ at a rated cell from an fp64 prediction kept per rating (see ccd_sweep_i),
// W_c = the column's sum of c_z + alpha (d - n_c).  Every term carries exactly one factor out of (c, alpha): scaling both by one
// power of two scales g, h, fundec, loss and reg exactly and leaves g / h.
namespace ccd {
constexpr int GRAM_ROWS = 64;       // the Gram-column kernel runs ceil(d / GRAM_ROWS) row blocks, i.e. that many partials per entry: a block
                                    // takes BLOCK / KW rows per step, strided over the grid, so at KW <= 2 most blocks find no row and
                                    // write zero partials, and at k = 100 a thread walks about 32 rows in sequence (follow-up: size the
                                    // partials from d * KW / BLOCK)
constexpr int GRAM_PART_MAX = 512;  // its row blocks (fixed by the shape, never by the device)
}  // namespace ccd

// s = F^T x and sum x^2 as per-block partials: part[b * (k + 1) + c] = the block's share of s[c], part[b * (k + 1) + k] of sum x^2.
// F is d x ld in the storage type, x fp64 -- or, with x == nullptr, F's own stored column xcol (the end-of-rank refresh of a Gram
// matrix's row).  KW = the power of two >= min(k, BLOCK) lanes run along a row's contiguous values, BLOCK / KW rows side by side;
// blockIdx.y takes the columns [y KW, (y + 1) KW) (one value of y up to k = 256).  A thread walks its rows b RPB + rr, + gridDim.x
// RPB, ... in order; the rows of one column meet in a fixed LDS tree.  `live`: 1 = inside the inner iterations (a broken rank's
// launches exit at entry), 0 = after them (a skipped rank's exit), -1 = at the start of training (the control block is not read).
template <typename T>
__global__ void __launch_bounds__(ccd::BLOCK) k_ccd_gramcol(const CcdCtl* ctl, int live, const T* F, int64_t d, int k, int ld, int kw, const double* x,
                                                            int xcol, double* part) {
    if (live >= 0 && (ctl->skip || (live && ctl->broken))) return;
    __shared__ double ls[ccd::BLOCK], lq[ccd::BLOCK];
    const int rpb = ccd::BLOCK / kw;
    const int cc = threadIdx.x & (kw - 1), rr = threadIdx.x / kw;
    const int c = blockIdx.y * kw + cc;
    const bool sq = cc == 0 && blockIdx.y == 0;
    double a = 0.0, q = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * rpb + rr; i < d; i += (int64_t)gridDim.x * rpb) {
        const double xi = x ? x[i] : (double)F[i * ld + xcol];
        if (c < k) a += (double)F[i * ld + c] * xi;
        if (sq) q += xi * xi;
    }
    ls[threadIdx.x] = a; lq[threadIdx.x] = q;
    __syncthreads();
    for (int w = rpb / 2; w > 0; w >>= 1) {
        if (rr < w) { ls[threadIdx.x] += ls[threadIdx.x + w * kw]; lq[threadIdx.x] += lq[threadIdx.x + w * kw]; }
        __syncthreads();
    }
    if (rr == 0) {
        if (c < k) part[(int64_t)blockIdx.x * (k + 1) + c] = ls[threadIdx.x];
        if (sq) part[(int64_t)blockIdx.x * (k + 1) + k] = lq[threadIdx.x];
    }
}
// s[c] = the partials of c in block order, c = 0 .. k (k: sum x^2); with G (k x k, at the start of training) row and column t of G
__global__ void __launch_bounds__(ccd::BLOCK) k_ccd_gramred(const CcdCtl* ctl, int live, const double* part, int P, int k, double* s, double* G, int t) {
    if (live > 0 && (ctl->skip || ctl->broken)) return;
    for (int c = threadIdx.x; c <= k; c += ccd::BLOCK) {
        double a = 0.0;
        for (int b = 0; b < P; ++b) a += part[(int64_t)b * (k + 1) + c];
        if (s) s[c] = a;
        if (G && c < k) { G[(int64_t)t * k + c] = a; G[(int64_t)c * k + t] = a; }
    }
}

// k_ccd_sweep under implicit feedback.  pd = the fp64 prediction u_i . v_j of the stored factors at every rated cell, in this
// orientation's order (next to the residual; k_ccd_resid_i keeps it): p^ = pd - oldx oldy is the prediction without rank t, so the rated
// cells leave the all-cells sum q_c as S = sum_Omega x p^ (the stored residual cannot give p^: in fp32 it carries its own rounding).
// F = this side's stored factors (the column's own row, one coalesced read by the wave that owns the column), sv = k_ccd_gramred's s and Sxx of the
// other side's CURRENT work vector, Wc = the column's total weight.  Every column is updated, an empty one too (its h is
// lambda W_c + alpha Sxx > 0).  WT: weights c_z in wt, else c = 1.
template <typename T, typename RT, bool WT>
__device__ __forceinline__ void ccd_sweep_i(const CcdCtl* ctl, const int64_t* ptr, const int32_t* idx, RT* res, const double* pd, const RT* wt,
                                            const double* Wc, const T* F, int ld, int k, int t, const double* sv, double alpha, const double* x,
                                            const double* oldx, const double* oldy, double* y, const int32_t* longs, int nlong,
                                            const int32_t* shorts, int nshort, double lambda, int do_nmf, int addback, double* part) {
    if (ctl->skip || ctl->broken) return;
    __shared__ double sg[ccd::BLOCK / 64], sh[ccd::BLOCK / 64], sf[ccd::BLOCK / 64], sp[ccd::BLOCK / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const bool is_long = (int)blockIdx.x < nlong;
    const int64_t s = is_long ? 0 : (int64_t)(blockIdx.x - nlong) * (ccd::BLOCK / 64) + wv;
    const bool have = is_long || s < nshort;
    double f = 0.0;
    if (have) {
        const int c = is_long ? longs[blockIdx.x] : shorts[s];
        const int64_t z0 = ptr[c], z1 = ptr[c + 1];
        const double oy = oldy[c];
        double g = 0.0, h = 0.0, S = 0.0;
        const int step = is_long ? ccd::BLOCK : 64;
        for (int64_t z = z0 + (is_long ? (int)threadIdx.x : lane); z < z1; z += step) {
            const int i = idx[z];
            double r = (double)res[z];
            const double ox = oldx[i];
            if (addback) { const RT rn = (RT)fma(ox, oy, r); res[z] = rn; r = (double)rn; }
            const double xi = x[i], cz = WT ? (double)wt[z] : 1.0;
            g += (cz * xi) * r;
            S += xi * fma(-ox, oy, pd[z]);
            h += ((cz - alpha) * xi) * xi;
        }
        double q = 0.0;
        if (!is_long || wv == 0)
            for (int j = lane; j < k; j += 64)
                if (j != t) q += (double)F[(int64_t)c * ld + j] * sv[j];
        g = ccd::wave_sum(g); h = ccd::wave_sum(h); S = ccd::wave_sum(S); q = ccd::wave_sum(q);
        if (is_long) {
            if (lane == 0) { sg[wv] = g; sh[wv] = h; sp[wv] = S; }
            __syncthreads();
            if (threadIdx.x == 0) {
                double G = 0.0, H = 0.0, SS = 0.0;
                for (int w = 0; w < ccd::BLOCK / 64; ++w) { G += sg[w]; H += sh[w]; SS += sp[w]; }
                y[c] = ccd::rank_one_new(G - alpha * (q - SS), lambda * Wc[c] + H + alpha * sv[k], y[c], do_nmf, &f);
                part[blockIdx.x] = f;
            }
            return;
        }
        if (lane == 0) y[c] = ccd::rank_one_new(g - alpha * (q - S), lambda * Wc[c] + h + alpha * sv[k], y[c], do_nmf, &f);
    }
    if (lane == 0) sf[wv] = f;
    __syncthreads();
    if (threadIdx.x == 0) {
        double Fs = 0.0;
        for (int w = 0; w < ccd::BLOCK / 64; ++w) Fs += sf[w];
        part[blockIdx.x] = Fs;
    }
}
template <typename T, typename RT>
__global__ void __launch_bounds__(ccd::BLOCK) k_ccd_sweep_i(const CcdCtl* ctl, const int64_t* ptr, const int32_t* idx, RT* res, const double* pd,
                                                            const double* Wc, const T* F, int ld, int k, int t, const double* sv, double alpha,
                                                            const double* x, const double* oldx, const double* oldy, double* y,
                                                            const int32_t* longs, int nlong, const int32_t* shorts, int nshort, double lambda,
                                                            int do_nmf, int addback, double* part) {
    ccd_sweep_i<T, RT, false>(ctl, ptr, idx, res, pd, nullptr, Wc, F, ld, k, t, sv, alpha, x, oldx, oldy, y, longs, nlong, shorts, nshort, lambda,
                              do_nmf, addback, part);
}
template <typename T, typename RT>
__global__ void __launch_bounds__(ccd::BLOCK) k_ccd_sweep_iw(const CcdCtl* ctl, const int64_t* ptr, const int32_t* idx, RT* res, const double* pd,
                                                             const RT* wt, const double* Wc, const T* F, int ld, int k, int t, const double* sv,
                                                             double alpha, const double* x, const double* oldx, const double* oldy, double* y,
                                                             const int32_t* longs, int nlong, const int32_t* shorts, int nshort, double lambda,
                                                             int do_nmf, int addback, double* part) {
    ccd_sweep_i<T, RT, true>(ctl, ptr, idx, res, pd, wt, Wc, F, ld, k, t, sv, alpha, x, oldx, oldy, y, longs, nlong, shorts, nshort, lambda,
                             do_nmf, addback, part);
}

// k_ccd_resid under implicit feedback: the same segments; the loss partials are the rated cells' share of the objective,
// sum (c r) r - (alpha p) p with p the prediction at a rated cell (k_ccd_final_i adds alpha sum_all p^2 from the Gram matrices);
// pd_r / pd_c = that prediction in fp64 in CSR / CSC order, both moved by the same expression from rank t's old term to its stored new
// one (0 at the start of training, where V = 0); wt_r = the weights in CSR order or nullptr (c = 1); Wu / Wv = the total weights.
template <typename T, typename RT>
__global__ void __launch_bounds__(ccd::BLOCK) k_ccd_resid_i(const CcdCtl* ctl, int B, int Bu, int Bv, int Bt, int64_t nnz, int64_t d1, int64_t d2,
                                                            int64_t tn, RT* res_r, const int32_t* row_r, const int32_t* col_r, RT* res_c,
                                                            const int32_t* row_c, const int32_t* col_c, double* pd_r, double* pd_c, const RT* wt_r, double alpha,
                                                            const double* Wu, const double* Wv, const double* u, const double* oldu, const double* v,
                                                            const double* oldv, T* U, T* V, int ld, int t, const int32_t* tu, const int32_t* ti,
                                                            double* tres, double* p_loss, double* p_regu, double* p_regv, double* p_rmse,
                                                            int addback) {
    if (ctl->skip) return;
    __shared__ double lds[ccd::BLOCK];
    int b = blockIdx.x;
    double s = 0.0;
    double* out = nullptr;
    if (b < 2 * B) {
        const bool csr = b < B;
        if (!csr) b -= B;
        RT* res = csr ? res_r : res_c;
        const int32_t* rr = csr ? row_r : row_c;
        const int32_t* cc = csr ? col_r : col_c;
        double* pd = csr ? pd_r : pd_c;
        for (int64_t z = (int64_t)b * ccd::BLOCK + threadIdx.x; z < nnz; z += (int64_t)B * ccd::BLOCK) {
            const double ui = (double)(T)u[rr[z]], vj = (double)(T)v[cc[z]];
            const double ou = oldu[rr[z]], ov = oldv[cc[z]];
            RT r0 = res[z];
            if (addback) r0 = (RT)fma(ou, ov, (double)r0);
            const RT rn = (RT)fma(-ui, vj, (double)r0);
            res[z] = rn;
            const double p = fma(ui, vj, fma(-ou, ov, pd[z]));
            pd[z] = p;
            if (csr) {
                const double r = (double)rn;
                s += ((wt_r ? (double)wt_r[z] : 1.0) * r) * r - (alpha * p) * p;
            }
        }
        if (!csr) return;
        out = p_loss;
    } else if ((b -= 2 * B) < Bu) {
        for (int64_t i = (int64_t)b * ccd::BLOCK + threadIdx.x; i < d1; i += (int64_t)Bu * ccd::BLOCK) {
            const T x = (T)u[i];
            U[i * ld + t] = x;
            const double n = Wu[i], xd = (double)x;
            s += n * (xd * xd) - n * (oldu[i] * oldu[i]);
        }
        out = p_regu;
    } else if ((b -= Bu) < Bv) {
        for (int64_t j = (int64_t)b * ccd::BLOCK + threadIdx.x; j < d2; j += (int64_t)Bv * ccd::BLOCK) {
            const T x = (T)v[j];
            V[j * ld + t] = x;
            const double n = Wv[j], xd = (double)x;
            s += n * xd * xd - n * oldv[j] * oldv[j];
        }
        out = p_regv;
    } else {
        b -= Bv;
        for (int64_t z = (int64_t)b * ccd::BLOCK + threadIdx.x; z < tn; z += (int64_t)Bt * ccd::BLOCK) {
            const int i = tu[z], j = ti[z];
            if (i < 0) { s += tres[z] * tres[z]; continue; }
            const double r = tres[z] - ((double)(T)u[i] * (double)(T)v[j] - oldu[i] * oldv[j]);
            tres[z] = r;
            s += r * r;
        }
        out = p_rmse;
    }
    s = ccd::block_reduce(s, lds);
    if (threadIdx.x == 0) out[b] = s;
}

// k_ccd_final under implicit feedback.  gu / gv = k_ccd_gramcol's partials of the STORED column t of U and of V (Pu / Pv blocks):
// row and column t of the two k x k fp64 Gram matrices GU = U^T U, GV = V^T V are refreshed from them, then
// loss = the rated cells' share + alpha sum_{s, s'} GU[s, s'] GV[s, s']  (= alpha times the sum of p^2 over ALL cells).
__global__ void __launch_bounds__(ccd::BLOCK) k_ccd_final_i(CcdCtl* ctl, const double* p_loss, int B, const double* p_regu, int Bu, const double* p_regv,
                                                            int Bv, const double* p_rmse, int Bt, int64_t tn, double lambda, double alpha,
                                                            const double* gu, int Pu, const double* gv, int Pv, double* GU, double* GV, int k, int t) {
    __shared__ double lds[ccd::BLOCK];
    if (ctl->skip) {
        if (threadIdx.x == 0) ctl->printed = 0;
        return;
    }
    for (int c = threadIdx.x; c < k; c += ccd::BLOCK) {
        double a = 0.0, b = 0.0;
        for (int p = 0; p < Pu; ++p) a += gu[(int64_t)p * (k + 1) + c];
        for (int p = 0; p < Pv; ++p) b += gv[(int64_t)p * (k + 1) + c];
        GU[(int64_t)t * k + c] = a; GU[(int64_t)c * k + t] = a;
        GV[(int64_t)t * k + c] = b; GV[(int64_t)c * k + t] = b;
    }
    __syncthreads();
    double dot = 0.0;
    for (int i = threadIdx.x; i < k * k; i += ccd::BLOCK) dot += GU[i] * GV[i];
    dot = ccd::block_reduce(dot, lds);
    const double loss = ccd::block_sum_fixed(p_loss, B, lds) + alpha * dot;
    const double rv = ccd::block_sum_fixed(p_regv, Bv, lds);
    const double ru = ccd::block_sum_fixed(p_regu, Bu, lds);
    const double se = ccd::block_sum_fixed(p_rmse, Bt, lds);
    if (threadIdx.x != 0) return;
    ctl->reg += rv;
    ctl->reg += ru;
    ctl->loss = loss;
    ctl->oldobj = ctl->obj;
    ctl->obj = loss + ctl->reg * lambda;
    ctl->rmse = tn > 0 ? sqrt(se / (double)tn) : 0.0;
    ctl->ranks_done += 1;
    ctl->printed = 1;
}

// k_ccd_init under implicit feedback: reg = sum_i W_i sum_t U_it^2 with the total weights, V = 0 and with it V^T V = 0
template <typename T>
__global__ void __launch_bounds__(ccd::BLOCK) k_ccd_init_i(T* V, int64_t nV, const T* U, int k, int ld, const int64_t* uptr, const double* Wu, int64_t d1,
                                                           double* p_reg, double* GV) {
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < k * k; i += ccd::BLOCK) GV[i] = 0.0;
    ccd_init<T, true>(V, nV, U, k, ld, uptr, Wu, d1, p_reg);
}

// the "ccd_residual_mismatch" diagnostic: positions where the CSC copy differs from the CSR copy, bit for bit
template <typename RT>
__global__ void __launch_bounds__(ccd::BLOCK) k_ccd_mismatch(const RT* res_r, const RT* res_c, const int32_t* c2r, int64_t nnz, double* part) {
    __shared__ double lds[ccd::BLOCK];
    double s = 0.0;
    for (int64_t z = (int64_t)blockIdx.x * ccd::BLOCK + threadIdx.x; z < nnz; z += (int64_t)gridDim.x * ccd::BLOCK) {
        s += ccd::bits(res_c[z]) != ccd::bits(res_r[c2r[z]]) ? 1.0 : 0.0;
    }
    s = ccd::block_reduce(s, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// ------------------------------------------------------------------------------------------------------------------------------
// host side
template <typename T>
struct CcdSolver final : pcr_solver {
    typedef T RT;                                     // storage type of the residuals
    std::unique_ptr<Solver<T>> base;                  // factors, evaluator, stream
    pcr_params prm;
    pcr_ccd_params cp;
    int64_t d1 = 0, d2 = 0, nnz = 0, tn = 0, tnnz_file = 0;
    int k = 1, ld = 4;
    hipStream_t st = nullptr;
    // CSR (user-major) and CSC (item-major) structure; row_* / col_* = user / item of every entry
    DBuf<int64_t> d_cptr;
    DBuf<int32_t> d_row_r, d_row_c, d_col_c, d_c2r, d_ilong, d_ishort, d_ulong, d_ushort, d_tu, d_ti;
    DBuf<RT> d_res_r, d_res_c;
    DBuf<double> d_u, d_oldu, d_v, d_oldv, d_tres;
    DBuf<double> d_vpart, d_upart, d_ploss, d_pregu, d_pregv, d_prmse, d_pmis;
    DBuf<CcdCtl> d_ctl;
    CcdCtl* h_ctl = nullptr;                          // pinned
    std::vector<RT> h_val_r, h_val_c;                 // the ratings in both orders (a training run starts from them)
    std::vector<double> h_tval;
    // per-rating confidence weights (pcr_solver_set_rating_weights): c_z rounded to RT in both orders, each read by its
    // sweep at the residual's index; W = their fp64 sums per user and per item, summed on the host in CSR / CSC order
    bool weighted = false;
    DBuf<RT> d_w_r, d_w_c;
    DBuf<double> d_Wu, d_Wv;
    std::vector<int32_t> h_c2r;
    std::vector<int64_t> h_uptr, h_cptr;
    // implicit feedback (pcr_solver_set_implicit): alpha as stored (rounded to RT; 0 = off), the fp64 predictions next to both
    // residual copies, the total weights W = Wobs + alpha (d - n) summed on the host, the Gram-column partials and reduced k-vectors of
    // both sides (k + 1 values: s and sum x^2) and the two k x k fp64 Gram matrices behind the loss
    double alpha = 0.0;
    std::vector<double> h_Wu, h_Wv;                   // Wobs while weights are set
    DBuf<double> d_pd_r, d_pd_c;
    DBuf<double> d_Wiu, d_Wiv, d_gpu, d_gpv, d_su, d_sv, d_GU, d_GV;
    int Pu = 1, Pv = 1, kw = 1;
    int nvb = 0, nub = 0, nilong = 0, nishort = 0, nulong = 0, nushort = 0;
    int B = 1, Bu = 1, Bv = 1, Bt = 1, Bi = 1;
    bool begun = false;
    int oiter = 0;                                    // outer iterations run since the start of training
    double secs = 0.0;                                // device seconds of the CCDR1 kernels since the start of training
    hipEvent_t ev_a = nullptr, ev_b = nullptr;

    ~CcdSolver() override {
        if (st) (void)hipStreamSynchronize(st);
        if (ev_a) (void)hipEventDestroy(ev_a);
        if (ev_b) (void)hipEventDestroy(ev_b);
        if (h_ctl) (void)hipHostFree(h_ctl);
    }

    static int parts(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(ccd::PART_MAX, (n + ccd::BLOCK * 4 - 1) / (ccd::BLOCK * 4))); }

    int init(const pcr_dataset* ds, const pcr_params* p) {
        prm = *p;
        pcr_ccd_params_default(&cp);
        if (prm.k < 1) { pcr_set_error("rank k must be >= 1"); return PCR_ERR_ARG; }
        pcr_params bp = *p;
        bp.solver_type = PCR_SOLVER_PCRPP;             // the shared machinery: factor storage, evaluator, stream
        base.reset(new Solver<T>());
        RC(base->init(ds, &bp, 0, 1));
        const auto t0 = std::chrono::steady_clock::now();
        st = base->st;
        d1 = base->d1; d2 = base->d2; nnz = base->nnz_local; tnnz_file = ds->tnnz_file;
        k = prm.k; ld = base->geo.ld;
        first_user = 0; n_users = d1; nnz_local = nnz;
        const PcrCsr& X = ds->train;
        // CSC by a counting sort over the CSR (entries of one item in user order)
        std::vector<int64_t> cptr((size_t)d2 + 1, 0);
        for (int64_t z = 0; z < nnz; ++z) cptr[(size_t)X.item[(size_t)z] + 1]++;
        for (int64_t j = 0; j < d2; ++j) cptr[(size_t)j + 1] += cptr[(size_t)j];
        std::vector<int32_t> row_r((size_t)nnz), row_c((size_t)nnz), col_c((size_t)nnz), c2r((size_t)nnz);
        h_val_r.resize((size_t)nnz); h_val_c.resize((size_t)nnz);
        {
            std::vector<int64_t> fill(cptr.begin(), cptr.end() - 1);
            for (int64_t u = 0; u < d1; ++u)
                for (int64_t z = X.index[(size_t)u]; z < X.index[(size_t)u + 1]; ++z) {
                    const int32_t j = X.item[(size_t)z];
                    const int64_t q = fill[(size_t)j]++;
                    row_r[(size_t)z] = (int32_t)u;
                    row_c[(size_t)q] = (int32_t)u; col_c[(size_t)q] = j; c2r[(size_t)q] = (int32_t)z;
                    h_val_r[(size_t)z] = (RT)X.val[(size_t)z];
                    h_val_c[(size_t)q] = (RT)X.val[(size_t)z];
                }
        }
        // column classes of the two sweeps
        auto classes = [](const std::vector<int64_t>& ptr, int64_t n, std::vector<int32_t>& lo, std::vector<int32_t>& hi) {
            for (int64_t c = 0; c < n; ++c) (ptr[(size_t)c + 1] - ptr[(size_t)c] > ccd::LONG ? hi : lo).push_back((int32_t)c);
        };
        std::vector<int32_t> ishort, ilong, ushort, ulong;
        classes(cptr, d2, ishort, ilong);
        classes(X.index, d1, ushort, ulong);
        nishort = (int)ishort.size(); nilong = (int)ilong.size(); nushort = (int)ushort.size(); nulong = (int)ulong.size();
        nvb = std::max(1, nilong + cdiv(nishort, ccd::BLOCK / 64));
        nub = std::max(1, nulong + cdiv(nushort, ccd::BLOCK / 64));
        // the test entries: util.cpp:206-215 walks T, the file's triplets in file order -- the data set's raw triplets where it
        // kept them (a test file that is not user-sorted), else the test CSR, which then is the file row by row
        std::vector<int32_t> tu, ti;
        if (!ds->traw_val.empty()) {
            tn = (int64_t)ds->traw_val.size();
            tu = ds->traw_user; ti = ds->traw_item; h_tval = ds->traw_val;
            // a user id >= d1 makes the reference read past W (util.cpp:211, undefined); here its residual stays at its rating
            for (int32_t& x : tu) if (x >= d1) x = -1;
        } else {
            const PcrCsr& TT = ds->test;
            tn = TT.nnz();
            tu.resize((size_t)tn);
            for (int64_t u = 0; u < TT.d1; ++u)
                for (int64_t z = TT.index[(size_t)u]; z < TT.index[(size_t)u + 1]; ++z) tu[(size_t)z] = (int32_t)u;
            ti.assign(TT.item.begin(), TT.item.begin() + tn);
            h_tval.assign(TT.val.begin(), TT.val.begin() + tn);
        }
        B = parts(nnz); Bu = parts(d1); Bv = parts(d2); Bt = parts(tn); Bi = parts(d1);
        RC(d_cptr.upload(cptr, st));
        RC(d_row_r.upload(row_r, st)); RC(d_row_c.upload(row_c, st)); RC(d_col_c.upload(col_c, st)); RC(d_c2r.upload(c2r, st));
        h_c2r.swap(c2r); h_cptr.swap(cptr); h_uptr.assign(X.index.begin(), X.index.begin() + d1 + 1);
        RC(d_ilong.upload(ilong, st)); RC(d_ishort.upload(ishort, st)); RC(d_ulong.upload(ulong, st)); RC(d_ushort.upload(ushort, st));
        RC(d_tu.upload(tu, st)); RC(d_ti.upload(ti, st));
        RC(d_res_r.alloc((size_t)nnz)); RC(d_res_c.alloc((size_t)nnz)); RC(d_tres.alloc((size_t)tn));
        RC(d_u.alloc((size_t)d1)); RC(d_oldu.alloc((size_t)d1)); RC(d_v.alloc((size_t)d2)); RC(d_oldv.alloc((size_t)d2));
        RC(d_vpart.alloc((size_t)nvb)); RC(d_upart.alloc((size_t)nub));
        RC(d_ploss.alloc((size_t)B)); RC(d_pregu.alloc((size_t)std::max(Bu, Bi))); RC(d_pregv.alloc((size_t)Bv)); RC(d_prmse.alloc((size_t)Bt));
        RC(d_pmis.alloc((size_t)B));
        RC(d_ctl.alloc(1));
        HIPCHK(hipMemset(d_ctl.p, 0, sizeof(CcdCtl)));
        HIPCHK(hipHostMalloc((void**)&h_ctl, sizeof(CcdCtl), hipHostMallocDefault));
        memset(h_ctl, 0, sizeof(CcdCtl));
        HIPCHK(hipEventCreate(&ev_a)); HIPCHK(hipEventCreate(&ev_b));
        setup_ms = base->setup_ms;
        setup_ms.emplace_back("CCDR1 CSC and residuals", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        return PCR_OK;
    }

    // ---- the training loop (timed in this solver's own profiler, pcr_solver::prof: the "ccd/..." slots)
    // ccd-r1.cpp:107-118: V = 0, residuals = ratings, reg from U
    int begin() {
        HIPCHK(hipMemcpyAsync(d_res_r.p, h_val_r.data(), (size_t)nnz * sizeof(RT), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_res_c.p, h_val_c.data(), (size_t)nnz * sizeof(RT), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_tres.p, h_tval.data(), (size_t)tn * sizeof(double), hipMemcpyHostToDevice, st));
        if (alpha > 0.0) {
            HIPCHK(hipMemsetAsync(d_pd_r.p, 0, (size_t)nnz * sizeof(double), st));       // V = 0: every prediction is 0
            HIPCHK(hipMemsetAsync(d_pd_c.p, 0, (size_t)nnz * sizeof(double), st));
            // reg from the total weights, V^T V = 0; U^T U once, a row per stored column
            ProfScope ps(&prof, "ccd/init.i", st);
            hipLaunchKernelGGL((k_ccd_init_i<T>), dim3(Bi), dim3(ccd::BLOCK), 0, st, base->d_V.p, d2 * ld, (const T*)base->d_U.p, k, ld,
                               (const int64_t*)base->d_uptr.p, (const double*)d_Wiu.p, d1, d_pregu.p, d_GV.p);
            hipLaunchKernelGGL(k_ccd_init_fin, dim3(1), dim3(ccd::BLOCK), 0, st, d_ctl.p, (const double*)d_pregu.p, Bi);
            for (int t = 0; t < k; ++t) {
                gramcol(-1, (const T*)base->d_U.p, d1, Pu, nullptr, t, d_gpu.p);
                hipLaunchKernelGGL(k_ccd_gramred, dim3(1), dim3(ccd::BLOCK), 0, st, (const CcdCtl*)d_ctl.p, 0, (const double*)d_gpu.p, Pu, k,
                                   (double*)nullptr, d_GU.p, t);
            }
        } else {
            ProfScope ps(&prof, weighted ? "ccd/init.w" : "ccd/init", st);
            if (weighted)
                hipLaunchKernelGGL((k_ccd_init_w<T>), dim3(Bi), dim3(ccd::BLOCK), 0, st, base->d_V.p, d2 * ld, (const T*)base->d_U.p, k, ld,
                                   (const int64_t*)base->d_uptr.p, (const double*)d_Wu.p, d1, d_pregu.p);
            else
                hipLaunchKernelGGL((k_ccd_init<T>), dim3(Bi), dim3(ccd::BLOCK), 0, st, base->d_V.p, d2 * ld, (const T*)base->d_U.p, k, ld,
                                   (const int64_t*)base->d_uptr.p, d1, d_pregu.p);
            hipLaunchKernelGGL(k_ccd_init_fin, dim3(1), dim3(ccd::BLOCK), 0, st, d_ctl.p, (const double*)d_pregu.p, Bi);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));
        begun = true;
        oiter = 0;
        secs = 0.0;
        return PCR_OK;
    }
    static int gram_parts(int64_t d) { return (int)std::max<int64_t>(1, std::min<int64_t>(ccd::GRAM_PART_MAX, (d + ccd::GRAM_ROWS - 1) / ccd::GRAM_ROWS)); }
    void gramcol(int live, const T* F, int64_t d, int P, const double* x, int xcol, double* part) {
        hipLaunchKernelGGL((k_ccd_gramcol<T>), dim3(P, cdiv(k, kw)), dim3(ccd::BLOCK), 0, st, (const CcdCtl*)d_ctl.p, live, F, d, k, ld, kw, x, xcol, part);
    }
    // s = F^T x and sum x^2 of the current work vector x, for the sweep of the other side: two launches
    void gram_vector(const T* F, int64_t d, int P, const double* x, double* part, double* s) {
        ProfScope ps(&prof, "ccd/gramcol", st);
        gramcol(1, F, d, P, x, 0, part);
        hipLaunchKernelGGL(k_ccd_gramred, dim3(1), dim3(ccd::BLOCK), 0, st, (const CcdCtl*)d_ctl.p, 1, (const double*)part, P, k, s, (double*)nullptr, 0);
    }
    // rank t under implicit feedback: 7 maxinneriter + 5 launches, no host round trip
    int enqueue_rank_implicit(int oi, int t) {
        const int T_in = cp.maxinneriter;
        {
            ProfScope ps(&prof, "ccd/begin", st);
            const int g = std::max(1, std::min(4096, cdiv(std::max(d1, d2), ccd::BLOCK)));
            hipLaunchKernelGGL((k_ccd_begin<T>), dim3(g), dim3(ccd::BLOCK), 0, st, d_ctl.p, (const T*)base->d_U.p, (const T*)base->d_V.p, ld, t, oi, d1, d2,
                               d_u.p, d_oldu.p, d_v.p, d_oldv.p);
        }
        const T* U = (const T*)base->d_U.p;
        const T* V = (const T*)base->d_V.p;
        for (int iter = 1; iter <= T_in; ++iter) {
            const int addback = (iter == 1 && oi > 1) ? 1 : 0;
            gram_vector(U, d1, Pu, (const double*)d_u.p, d_gpu.p, d_su.p);                  // s = U^T u, sum u^2: from the CURRENT u
            {
                ProfScope ps(&prof, "ccd/vsweep.i", st);
                if (weighted)
                    hipLaunchKernelGGL((k_ccd_sweep_iw<T, RT>), dim3(nvb), dim3(ccd::BLOCK), 0, st, (const CcdCtl*)d_ctl.p, (const int64_t*)d_cptr.p,
                                       (const int32_t*)d_row_c.p, d_res_c.p, (const double*)d_pd_c.p, (const RT*)d_w_c.p, (const double*)d_Wiv.p, V, ld, k, t,
                                       (const double*)d_su.p, alpha, (const double*)d_u.p, (const double*)d_oldu.p, (const double*)d_oldv.p, d_v.p,
                                       (const int32_t*)d_ilong.p, nilong, (const int32_t*)d_ishort.p, nishort, prm.lambda, cp.do_nmf, addback, d_vpart.p);
                else
                    hipLaunchKernelGGL((k_ccd_sweep_i<T, RT>), dim3(nvb), dim3(ccd::BLOCK), 0, st, (const CcdCtl*)d_ctl.p, (const int64_t*)d_cptr.p,
                                       (const int32_t*)d_row_c.p, d_res_c.p, (const double*)d_pd_c.p, (const double*)d_Wiv.p, V, ld, k, t,
                                       (const double*)d_su.p, alpha, (const double*)d_u.p, (const double*)d_oldu.p, (const double*)d_oldv.p, d_v.p,
                                       (const int32_t*)d_ilong.p, nilong, (const int32_t*)d_ishort.p, nishort, prm.lambda, cp.do_nmf, addback, d_vpart.p);
            }
            gram_vector(V, d2, Pv, (const double*)d_v.p, d_gpv.p, d_sv.p);                  // s = V^T v from the v just written
            {
                ProfScope ps(&prof, "ccd/usweep.i", st);
                if (weighted)
                    hipLaunchKernelGGL((k_ccd_sweep_iw<T, RT>), dim3(nub), dim3(ccd::BLOCK), 0, st, (const CcdCtl*)d_ctl.p, (const int64_t*)base->d_uptr.p,
                                       (const int32_t*)base->d_item.p, d_res_r.p, (const double*)d_pd_r.p, (const RT*)d_w_r.p, (const double*)d_Wiu.p, U, ld, k,
                                       t, (const double*)d_sv.p, alpha, (const double*)d_v.p, (const double*)d_oldv.p, (const double*)d_oldu.p, d_u.p,
                                       (const int32_t*)d_ulong.p, nulong, (const int32_t*)d_ushort.p, nushort, prm.lambda, cp.do_nmf, addback, d_upart.p);
                else
                    hipLaunchKernelGGL((k_ccd_sweep_i<T, RT>), dim3(nub), dim3(ccd::BLOCK), 0, st, (const CcdCtl*)d_ctl.p, (const int64_t*)base->d_uptr.p,
                                       (const int32_t*)base->d_item.p, d_res_r.p, (const double*)d_pd_r.p, (const double*)d_Wiu.p, U, ld, k, t,
                                       (const double*)d_sv.p, alpha, (const double*)d_v.p, (const double*)d_oldv.p, (const double*)d_oldu.p, d_u.p,
                                       (const int32_t*)d_ulong.p, nulong, (const int32_t*)d_ushort.p, nushort, prm.lambda, cp.do_nmf, addback, d_upart.p);
            }
            {
                ProfScope ps(&prof, "ccd/decide", st);
                hipLaunchKernelGGL(k_ccd_decide, dim3(1), dim3(ccd::BLOCK), 0, st, d_ctl.p, (const double*)d_vpart.p, nvb, (const double*)d_upart.p, nub,
                                   cp.eps, oi, t, iter);
            }
        }
        {
            ProfScope ps(&prof, "ccd/resid.i", st);
            hipLaunchKernelGGL((k_ccd_resid_i<T, RT>), dim3(2 * B + Bu + Bv + Bt), dim3(ccd::BLOCK), 0, st, (const CcdCtl*)d_ctl.p, B, Bu, Bv, Bt, nnz,
                               d1, d2, tn, d_res_r.p, (const int32_t*)d_row_r.p, (const int32_t*)base->d_item.p, d_res_c.p, (const int32_t*)d_row_c.p,
                               (const int32_t*)d_col_c.p, d_pd_r.p, d_pd_c.p, weighted ? (const RT*)d_w_r.p : (const RT*)nullptr, alpha,
                               (const double*)d_Wiu.p, (const double*)d_Wiv.p, (const double*)d_u.p, (const double*)d_oldu.p, (const double*)d_v.p,
                               (const double*)d_oldv.p, base->d_U.p, base->d_V.p, ld, t, (const int32_t*)d_tu.p, (const int32_t*)d_ti.p, d_tres.p,
                               d_ploss.p, d_pregu.p, d_pregv.p, d_prmse.p, (T_in < 1 && oi > 1) ? 1 : 0);
        }
        {
            // row t of both Gram matrices from the STORED column t, then the record
            ProfScope ps(&prof, "ccd/final.i", st);
            gramcol(0, U, d1, Pu, nullptr, t, d_gpu.p);
            gramcol(0, V, d2, Pv, nullptr, t, d_gpv.p);
            hipLaunchKernelGGL(k_ccd_final_i, dim3(1), dim3(ccd::BLOCK), 0, st, d_ctl.p, (const double*)d_ploss.p, B, (const double*)d_pregu.p, Bu,
                               (const double*)d_pregv.p, Bv, (const double*)d_prmse.p, Bt, tn, prm.lambda, alpha, (const double*)d_gpu.p, Pu,
                               (const double*)d_gpv.p, Pv, d_GU.p, d_GV.p, k, t);
        }
        HIPCHK(hipGetLastError());
        return PCR_OK;
    }
    // rank t of outer iteration `oi` (ccd-r1.cpp:130-199): 3 maxinneriter + 3 launches, no host round trip
    int enqueue_rank(int oi, int t) {
        if (alpha > 0.0) return enqueue_rank_implicit(oi, t);
        const int T_in = cp.maxinneriter;
        {
            ProfScope ps(&prof, "ccd/begin", st);
            const int g = std::max(1, std::min(4096, cdiv(std::max(d1, d2), ccd::BLOCK)));
            hipLaunchKernelGGL((k_ccd_begin<T>), dim3(g), dim3(ccd::BLOCK), 0, st, d_ctl.p, (const T*)base->d_U.p, (const T*)base->d_V.p, ld, t, oi, d1, d2,
                               d_u.p, d_oldu.p, d_v.p, d_oldv.p);
        }
        for (int iter = 1; iter <= T_in; ++iter) {
            const int addback = (iter == 1 && oi > 1) ? 1 : 0;          // ccd-r1.cpp:127-130, fused into the first sweeps
            if (weighted) {
                {
                    ProfScope ps(&prof, "ccd/vsweep.w", st);
                    hipLaunchKernelGGL((k_ccd_sweep_w<RT>), dim3(nvb), dim3(ccd::BLOCK), 0, st, (const CcdCtl*)d_ctl.p, (const int64_t*)d_cptr.p,
                                       (const int32_t*)d_row_c.p, d_res_c.p, (const RT*)d_w_c.p, (const double*)d_Wv.p, (const double*)d_u.p,
                                       (const double*)d_oldu.p, (const double*)d_oldv.p, d_v.p, (const int32_t*)d_ilong.p, nilong,
                                       (const int32_t*)d_ishort.p, nishort, prm.lambda, cp.do_nmf, addback, d_vpart.p);
                }
                {
                    ProfScope ps(&prof, "ccd/usweep.w", st);
                    hipLaunchKernelGGL((k_ccd_sweep_w<RT>), dim3(nub), dim3(ccd::BLOCK), 0, st, (const CcdCtl*)d_ctl.p, (const int64_t*)base->d_uptr.p,
                                       (const int32_t*)base->d_item.p, d_res_r.p, (const RT*)d_w_r.p, (const double*)d_Wu.p, (const double*)d_v.p,
                                       (const double*)d_oldv.p, (const double*)d_oldu.p, d_u.p, (const int32_t*)d_ulong.p, nulong,
                                       (const int32_t*)d_ushort.p, nushort, prm.lambda, cp.do_nmf, addback, d_upart.p);
                }
            } else {
            {
                ProfScope ps(&prof, "ccd/vsweep", st);
                hipLaunchKernelGGL((k_ccd_sweep<RT>), dim3(nvb), dim3(ccd::BLOCK), 0, st, (const CcdCtl*)d_ctl.p, (const int64_t*)d_cptr.p,
                                   (const int32_t*)d_row_c.p, d_res_c.p, (const double*)d_u.p, (const double*)d_oldu.p, (const double*)d_oldv.p, d_v.p,
                                   (const int32_t*)d_ilong.p, nilong, (const int32_t*)d_ishort.p, nishort, prm.lambda, cp.do_nmf, addback, d_vpart.p);
            }
            {
                ProfScope ps(&prof, "ccd/usweep", st);
                hipLaunchKernelGGL((k_ccd_sweep<RT>), dim3(nub), dim3(ccd::BLOCK), 0, st, (const CcdCtl*)d_ctl.p, (const int64_t*)base->d_uptr.p,
                                   (const int32_t*)base->d_item.p, d_res_r.p, (const double*)d_v.p, (const double*)d_oldv.p, (const double*)d_oldu.p, d_u.p,
                                   (const int32_t*)d_ulong.p, nulong, (const int32_t*)d_ushort.p, nushort, prm.lambda, cp.do_nmf, addback, d_upart.p);
            }
            }
            {
                ProfScope ps(&prof, "ccd/decide", st);
                hipLaunchKernelGGL(k_ccd_decide, dim3(1), dim3(ccd::BLOCK), 0, st, d_ctl.p, (const double*)d_vpart.p, nvb, (const double*)d_upart.p, nub,
                                   cp.eps, oi, t, iter);
            }
        }
        if (weighted) {
            ProfScope ps(&prof, "ccd/resid.w", st);
            hipLaunchKernelGGL((k_ccd_resid_w<T, RT>), dim3(2 * B + Bu + Bv + Bt), dim3(ccd::BLOCK), 0, st, (const CcdCtl*)d_ctl.p, B, Bu, Bv, Bt, nnz,
                               d1, d2, tn, d_res_r.p, (const int32_t*)d_row_r.p, (const int32_t*)base->d_item.p, d_res_c.p, (const int32_t*)d_row_c.p,
                               (const int32_t*)d_col_c.p, (const int64_t*)base->d_uptr.p, (const int64_t*)d_cptr.p, (const RT*)d_w_r.p,
                               (const double*)d_Wu.p, (const double*)d_Wv.p, (const double*)d_u.p, (const double*)d_oldu.p, (const double*)d_v.p,
                               (const double*)d_oldv.p, base->d_U.p, base->d_V.p, ld, t, (const int32_t*)d_tu.p, (const int32_t*)d_ti.p, d_tres.p,
                               d_ploss.p, d_pregu.p, d_pregv.p, d_prmse.p, (T_in < 1 && oi > 1) ? 1 : 0);
        } else {
            ProfScope ps(&prof, "ccd/resid", st);
            hipLaunchKernelGGL((k_ccd_resid<T, RT>), dim3(2 * B + Bu + Bv + Bt), dim3(ccd::BLOCK), 0, st, (const CcdCtl*)d_ctl.p, B, Bu, Bv, Bt, nnz,
                               d1, d2, tn, d_res_r.p, (const int32_t*)d_row_r.p, (const int32_t*)base->d_item.p, d_res_c.p, (const int32_t*)d_row_c.p,
                               (const int32_t*)d_col_c.p, (const int64_t*)base->d_uptr.p, (const int64_t*)d_cptr.p, (const double*)d_u.p,
                               (const double*)d_oldu.p, (const double*)d_v.p, (const double*)d_oldv.p, base->d_U.p, base->d_V.p, ld, t,
                               (const int32_t*)d_tu.p, (const int32_t*)d_ti.p, d_tres.p, d_ploss.p, d_pregu.p, d_pregv.p, d_prmse.p,
                               (T_in < 1 && oi > 1) ? 1 : 0);
        }
        {
            ProfScope ps(&prof, "ccd/final", st);
            hipLaunchKernelGGL(k_ccd_final, dim3(1), dim3(ccd::BLOCK), 0, st, d_ctl.p, (const double*)d_ploss.p, B, (const double*)d_pregu.p, Bu,
                               (const double*)d_pregv.p, Bv, (const double*)d_prmse.p, Bt, tn, prm.lambda);
        }
        HIPCHK(hipGetLastError());
        return PCR_OK;
    }
    int read_ctl() {
        HIPCHK(hipMemcpyAsync(h_ctl, d_ctl.p, sizeof(CcdCtl), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return PCR_OK;
    }
    double elapsed_s() {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ev_a, ev_b) != hipSuccess) return 0.0;
        return ms / 1e3;
    }
    // outer iteration oi in one go: its k ranks between the timing events, one host round trip; secs += its device time
    int run_outer(int oi) {
        HIPCHK(hipEventRecord(ev_a, st));
        for (int t = 0; t < k; ++t) RC(enqueue_rank(oi, t));
        HIPCHK(hipEventRecord(ev_b, st));
        RC(read_ctl());
        secs += elapsed_s();
        return PCR_OK;
    }

    // ccd-r1.cpp:97-212 ccdr1(): from the current U (V is zeroed); with verbose one line per rank, evaluated after every printed
    // rank when do_predict and the test set is not empty (:196-206).  hist[0] is zero (nothing is printed before the first rank);
    // hist[o]: outer iteration o -- obj of its last rank, the last evaluation, cumulative device seconds of the CCDR1 kernels,
    // cg_v = inner iterations executed, cg_u = ranks executed.
    int train(pcr_log_fn log, void* ctx, pcr_iter_stats* hist) override {
        auto emit = [&](const char* s) { if (log) log(ctx, s); else { fputs(s, stdout); fputc('\n', stdout); fflush(stdout); } };
        RC(begin());
        if (hist) {
            memset(hist, 0, sizeof(pcr_iter_stats) * (size_t)(std::max(0, prm.maxiter) + 1));
        }
        double te = 0.0, tndcg = 0.0;
        const bool logging = prm.verbose != 0;
        const bool evalp = prm.do_predict != 0 && tnnz_file != 0;
        char line[1024];
        for (int oi = 1; oi <= prm.maxiter; ++oi) {
            oiter = oi;
            if (!logging) {
                RC(run_outer(oi));
            } else {
                for (int t = 0; t < k; ++t) {
                    HIPCHK(hipEventRecord(ev_a, st));
                    RC(enqueue_rank(oi, t));
                    HIPCHK(hipEventRecord(ev_b, st));
                    RC(read_ctl());
                    if (!h_ctl->printed) break;                   // ccd-r1.cpp:131: every later rank is skipped too
                    secs += elapsed_s();
                    int n = snprintf(line, sizeof line, "iter %d rank %d time %.10g loss %.10g obj %.10g diff %.10g gnorm %.6g reg %.7g ", oi,
                                     t + 1, secs, h_ctl->loss, h_ctl->obj, h_ctl->oldobj - h_ctl->obj, 0.0, h_ctl->reg);
                    if (evalp) {
                        RC(base->evaluate(1, prm.ndcg_k, &te, &tndcg));
                        n += snprintf(line + n, sizeof line - (size_t)n, "rmse %.10g", h_ctl->rmse);
                        snprintf(line + n, sizeof line - (size_t)n, "(Testing) pairwise error %lf NDCG %lf", te, tndcg);
                    }
                    emit(line);
                }
            }
            if (hist) {
                pcr_iter_stats& r = hist[oi];
                r.obj = h_ctl->obj; r.test_err = te; r.test_ndcg = tndcg; r.seconds = secs;
                r.cg_v = h_ctl->inner_iters; r.cg_u = h_ctl->ranks_done;
            }
        }
        return PCR_OK;
    }
    // n more outer iterations without evaluation, one host round trip each (a training run is started first if none is); seconds
    // in the records carry on from pcr_train and earlier calls: cumulative since the start of training
    int iterate_abi(int n, pcr_iter_stats* out) override {
        if (n < 0) { pcr_set_error("n must be >= 0"); return PCR_ERR_ARG; }
        if (!begun) RC(begin());
        for (int q = 0; q < n; ++q) {
            RC(run_outer(++oiter));
            if (out) {
                memset(&out[q], 0, sizeof(pcr_iter_stats));
                out[q].obj = h_ctl->obj; out[q].seconds = secs;
                out[q].cg_v = h_ctl->inner_iters; out[q].cg_u = h_ctl->ranks_done;
            }
        }
        return PCR_OK;
    }

    int set_factors(const double* U, const double* V, bool local) override { begun = false; return base->set_factors(U, V, local); }
    // w: nnz weights in the training CSR's order, each finite and > 0 as given and as stored (rounded to RT, as the ratings are); NULL:
    // the unweighted kernels.  Nothing is changed before every weight has passed.  Ends a running training, like set_factors.
    int set_rating_weights(const double* w) override {
        HIPCHK(hipStreamSynchronize(st));
        if (!w) {
            weighted = false; begun = false;
            h_Wu.clear(); h_Wv.clear();
            return alpha > 0.0 ? total_weights(alpha) : PCR_OK;
        }
        std::vector<RT> w_r((size_t)nnz), w_c((size_t)nnz);
        for (int64_t z = 0; z < nnz; ++z) {
            const bool in_range = w[z] > 0.0 && w[z] <= (double)std::numeric_limits<RT>::max();     // (NaN fails both)
            const RT c = in_range ? (RT)w[z] : (RT)0;
            if (!(c > (RT)0)) {
                pcr_set_error("pcr_solver_set_rating_weights: the weight of training rating " + std::to_string(z) +
                              " is not a finite number > 0 in the solver's precision");
                return PCR_ERR_ARG;
            }
            w_r[(size_t)z] = c;
        }
        std::vector<double> Wu((size_t)d1, 0.0), Wv((size_t)d2, 0.0);
        for (int64_t u = 0; u < d1; ++u) {
            double s = 0.0;
            for (int64_t z = h_uptr[(size_t)u]; z < h_uptr[(size_t)u + 1]; ++z) s += (double)w_r[(size_t)z];
            Wu[(size_t)u] = s;
        }
        for (int64_t j = 0; j < d2; ++j) {                                // (CSC order: the entries of one item in user order)
            double s = 0.0;
            for (int64_t q = h_cptr[(size_t)j]; q < h_cptr[(size_t)j + 1]; ++q) {
                w_c[(size_t)q] = w_r[(size_t)h_c2r[(size_t)q]];
                s += (double)w_c[(size_t)q];
            }
            Wv[(size_t)j] = s;
        }
        RC(d_w_r.upload(w_r, st)); RC(d_w_c.upload(w_c, st)); RC(d_Wu.upload(Wu, st)); RC(d_Wv.upload(Wv, st));
        weighted = true;
        begun = false;
        h_Wu.swap(Wu); h_Wv.swap(Wv);
        return alpha > 0.0 ? total_weights(alpha) : PCR_OK;
    }
    int rating_weights_set(double* value) override { *value = weighted ? 1.0 : 0.0; return PCR_OK; }
    // W = Wobs + a (d - n) per user and per item (Wobs = the sum of c_z, the count without weights): the row's total weight, the
    // unrated cells included
    int total_weights(double a) {
        std::vector<double> Wu((size_t)d1), Wv((size_t)d2);
        for (int64_t u = 0; u < d1; ++u) {
            const int64_t n = h_uptr[(size_t)u + 1] - h_uptr[(size_t)u];
            Wu[(size_t)u] = (weighted ? h_Wu[(size_t)u] : (double)n) + a * (double)(d2 - n);
        }
        for (int64_t j = 0; j < d2; ++j) {
            const int64_t n = h_cptr[(size_t)j + 1] - h_cptr[(size_t)j];
            Wv[(size_t)j] = (weighted ? h_Wv[(size_t)j] : (double)n) + a * (double)(d1 - n);
        }
        RC(d_Wiu.upload(Wu, st)); RC(d_Wiv.upload(Wv, st));
        return PCR_OK;
    }
    // a: the weight of every unrated cell (target 0), finite and >= 0 as given, > 0 as stored (rounded to RT, as weights are) when
    // > 0 as given; 0: the explicit kernels.  Nothing is changed before a has passed.  Ends a running training, like set_factors.
    int set_implicit(double a) override {
        const bool in_range = a >= 0.0 && a <= (double)std::numeric_limits<RT>::max();      // (NaN fails both)
        const double as = in_range ? (double)(RT)a : -1.0;
        if (!in_range || (a > 0.0 && !(as > 0.0))) {
            pcr_set_error("pcr_solver_set_implicit: alpha must be a finite number >= 0, and > 0 in the solver's precision when it is > 0");
            return PCR_ERR_ARG;
        }
        HIPCHK(hipStreamSynchronize(st));
        if (as > 0.0) {
            if (!d_pd_r.p) {
                Pu = gram_parts(d1); Pv = gram_parts(d2);
                for (kw = 1; kw < k && kw < ccd::BLOCK; kw <<= 1) {}
                RC(d_pd_r.alloc((size_t)nnz)); RC(d_pd_c.alloc((size_t)nnz));
                RC(d_gpu.alloc((size_t)Pu * (size_t)(k + 1))); RC(d_gpv.alloc((size_t)Pv * (size_t)(k + 1)));
                RC(d_su.alloc((size_t)k + 1)); RC(d_sv.alloc((size_t)k + 1));
                RC(d_GU.alloc((size_t)k * (size_t)k)); RC(d_GV.alloc((size_t)k * (size_t)k));
            }
            RC(total_weights(as));
        }
        alpha = as;
        begun = false;
        return PCR_OK;
    }
    int implicit_alpha(double* value) override { *value = alpha; return PCR_OK; }
    int get_factors(double* U, double* V, bool local) override { return base->get_factors(U, V, local); }
    int evaluate(int which, int ndcg_k, double* err, double* ndcg) override { return base->evaluate(which, ndcg_k, err, ndcg); }
    double ridge_lambda() override { return prm.lambda; }
    void serve_view(ServeView* v) override { base->serve_view(v); v->prof = &prof; }   // (the "recommend/..." slots are this solver's)
    int residual_mismatch(double* value) override {
        hipLaunchKernelGGL((k_ccd_mismatch<RT>), dim3(B), dim3(ccd::BLOCK), 0, st, (const RT*)d_res_r.p, (const RT*)d_res_c.p, (const int32_t*)d_c2r.p,
                           nnz, d_pmis.p);
        HIPCHK(hipGetLastError());
        std::vector<double> h((size_t)B);
        HIPCHK(hipMemcpyAsync(h.data(), d_pmis.p, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        double s = 0.0;
        for (double x : h) s += x;
        *value = s;
        return PCR_OK;
    }
    // any values, as the reference takes them: maxinneriter <= 0 runs no inner iteration (each rank only re-forms its residual)
    int set_ccd_params(const pcr_ccd_params* p) override {
        cp = *p;
        return PCR_OK;
    }
    int comm_init(const void*) override { pcr_set_error("CCDR1 runs on one rank"); return PCR_ERR_UNSUPPORTED; }
    int comm_init_p2p(const char*) override { pcr_set_error("CCDR1 runs on one rank"); return PCR_ERR_UNSUPPORTED; }
    void comm_abort() override {}
    int comm_nranks() override { return 1; }
    int sync() override { HIPCHK(hipStreamSynchronize(st)); return PCR_OK; }
    std::string ustep_classes() override { return ""; }
    int class_rows(const std::string& slot, double*) override { pcr_set_error("no U-step class '" + slot + "' on a CCDR1 solver"); return PCR_ERR_ARG; }
};
