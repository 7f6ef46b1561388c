// pcr_serve.hip -- the serving layer behind the C ABI of include/primalcr.h: top-K recommendation, its top-N, rank and
// beyond-accuracy evaluations, the MMR re-ranking, the group cap and the metrics of given and re-ranked lists, over the kernels of
// pcr_topk.h.
//
// Every entry exists twice: on a trained solver (pcr_recommend, ...) and on a model in host memory (pcr_recommend_model, ...).
// Both come down to a ServeView (pcr_dev.h) -- filled by the solver (pcr_solver::serve_view) or by ModelDev, which uploads the
// model for one call -- and one function per entry over that view, which picks the precision.  Training is pcr_solver.hip; the
// four fold-in families are pcr_fold.hip.
// There is NO CPU compute path in this file: every [device] entry point fails with PCR_ERR_DEVICE when HIP is unusable.
#include <cmath>

#include "pcr_dev.h"
#include "pcr_prims.h"
#include "pcr_topk.h"

int ServeView::sum(double* dev, size_t count) const { return owner ? owner->allreduce_f64(dev, count) : PCR_OK; }
int ServeView::wait() const { if (owner) return owner->sync(); HIPCHK(hipStreamSynchronize(st)); return PCR_OK; }
// the cut[] array of TopnArgs / DivArgs: the ncut cutoffs, then zeros
static void fill_cuts(int* dst, int ncut, const int* cuts) {
    for (int c = 0; c < PCR_TOPN_MAX_CUTOFFS; ++c) dst[c] = c < ncut ? cuts[c] : 0;
}

// Top-K recommendation (pcr_topk.h) for the n users h_users[0..n) -- rows of v's U and of its exclusion CSR (xptr() NULL:
// none), or rows 0..n-1 when h_users is NULL.  Users go in batches whose partial lists stay under REC_SCRATCH bytes; the item
// range is split across workgroups until the grid holds about REC_TARGET_WG workgroups (ml1m's 6 040 users are 95 workgroups
// of 64).  Each batch's partial lists go to the sink: sink.begin(nb) once with the largest batch, then sink.batch(b0, m, ...)
// per batch, which merges them (RecCopy: into pcr_recommend's host arrays; RecTopn: into the top-N metrics).  The launches
// are timed in v.prof's "recommend/..." slots (NULL: not profiled).  v.allow (NULL but in a filtered call) goes to the score kernel as it is.
// select = 0 only for tools/exp_recommend.py's GEMM-alone timing (lists come back empty).
static const size_t REC_SCRATCH = (size_t)1 << 30;
static const int REC_TARGET_WG = 1024, REC_MAX_SPLIT = 16, REC_MIN_SPLIT_ITEMS = 1024;
// The user batches and item splits of a sweep over n users whose scratch takes per_user bytes per user and split (rec_run and
// rank_run share this arithmetic): nb users per batch, at most smax splits
struct RecGeom {
    int64_t d2, nb = 0;
    int smax = 1;
    static constexpr int64_t users_per_wg = (int64_t)rec::WAVES * rec::UW;
    int splits_for(int64_t users) const {
        const int64_t wg = (users + users_per_wg - 1) / users_per_wg;
        int64_t s = std::max<int64_t>(1, (REC_TARGET_WG + wg - 1) / wg);
        s = std::min<int64_t>(s, std::max<int64_t>(1, d2 / REC_MIN_SPLIT_ITEMS));
        return (int)std::min<int64_t>(s, REC_MAX_SPLIT);
    }
    RecGeom(int64_t n, int64_t d2_, size_t per_user) : d2(d2_) {
        nb = std::min<int64_t>(n, std::max<int64_t>(users_per_wg, (int64_t)(REC_SCRATCH / (per_user * 2)) / users_per_wg * users_per_wg));
        while (nb > users_per_wg && (size_t)nb * (size_t)splits_for(nb) * per_user > REC_SCRATCH) nb = std::max<int64_t>(users_per_wg, nb / 2);
        smax = splits_for(std::min(nb, n));
    }
    // a batch of m users: the items per split (whole steps) and the splits launched
    void batch(int64_t m, int* per, int* nsp) const {
        const int ns = std::min(splits_for(m), smax);      // (a short last batch keeps the scratch of the first)
        *per = (int)(((d2 + ns - 1) / ns + rec::TILE - 1) / rec::TILE * rec::TILE);
        *nsp = (int)((d2 + *per - 1) / *per);
    }
};

template <typename T, class Sink>
static int rec_run(const ServeView& v, int64_t n, const int32_t* h_users, int K, int select, Sink&& sink) {
    if (n <= 0) return PCR_OK;
    hipStream_t st = v.st;
    const size_t per_user = (size_t)K * (sizeof(T) + sizeof(int32_t)) + sizeof(int32_t);
    const RecGeom geom(n, v.d2, per_user);
    const int64_t users_per_wg = RecGeom::users_per_wg, nb = geom.nb;
    const int smax = geom.smax;
    DBuf<T> ls; DBuf<int32_t> li, ln, du;
    RC(ls.alloc((size_t)nb * smax * K)); RC(li.alloc((size_t)nb * smax * K)); RC(ln.alloc((size_t)nb * smax));
    RC(du.alloc((size_t)nb)); RC(sink.begin(nb));
    const size_t lds = rec_wave_lds<T>(K) * rec::WAVES;
    HIPCHK(hipFuncSetAttribute((const void*)k_rec_score<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    std::vector<int32_t> seq;
    for (int64_t b0 = 0; b0 < n; b0 += nb) {
        const int64_t m = std::min(nb, n - b0);
        const int32_t* hu = h_users ? h_users + b0 : nullptr;
        if (!hu) { seq.resize((size_t)m); for (int64_t i = 0; i < m; ++i) seq[(size_t)i] = (int32_t)(b0 + i); hu = seq.data(); }
        HIPCHK(hipMemcpyAsync(du.p, hu, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, st));
        int per, nsp;
        geom.batch(m, &per, &nsp);
        {
            ProfScope ps(v.prof, "recommend/score", st);
            hipLaunchKernelGGL((k_rec_score<T>), dim3((unsigned)cdiv(m, users_per_wg), (unsigned)nsp), dim3(rec::WAVES * 64), lds, st, serve_U<T>(v),
                               serve_V<T>(v), v.r, v.ld, (int)v.d2, du.p, m, v.xptr(), v.xitem(), K, per, ls.p, li.p, ln.p, select, v.allow);
            HIPCHK(hipGetLastError());
        }
        RC(sink.batch(b0, m, (const T*)ls.p, (const int32_t*)li.p, (const int32_t*)ln.p, nsp));
        HIPCHK(hipStreamSynchronize(st));                  // (the next batch's users overwrite du / seq)
    }
    return PCR_OK;
}

// rec_run's sink for pcr_recommend: merged lists to the host arrays items / scores (n x K)
template <typename T>
struct RecCopy {
    const ServeView& v;
    int K;
    int32_t* items;
    double* scores;
    DBuf<int32_t> oi;
    DBuf<double> os;
    int begin(int64_t nb) { RC(oi.alloc((size_t)nb * K)); RC(os.alloc((size_t)nb * K)); return PCR_OK; }
    int batch(int64_t b0, int64_t m, const T* ls, const int32_t* li, const int32_t* ln, int nsp) {
        {
            ProfScope ps(v.prof, "recommend/merge", v.st);
            hipLaunchKernelGGL((k_rec_merge<T>), dim3((unsigned)cdiv(m, 4)), dim3(256), 0, v.st, ls, li, ln, nsp, m, K, oi.p, os.p);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipMemcpyAsync(items + b0 * K, oi.p, (size_t)m * K * sizeof(int32_t), hipMemcpyDeviceToHost, v.st));
        HIPCHK(hipMemcpyAsync(scores + b0 * K, os.p, (size_t)m * K * sizeof(double), hipMemcpyDeviceToHost, v.st));
        return PCR_OK;
    }
};

// Top-K over candidate lists (k_rec_cand of pcr_topk.h) for the n users h_users (rows of v's U and of its
// exclusion CSR, as rec_run; NULL: rows 0..n-1): row i of the host CSR cptr[n + 1] / citem holds users[i]'s candidates.  Users go
// in batches of at most CAND_BATCH list entries and, past the first user of a batch, CAND_ITEMS candidates; a batch uploads its
// users, its slice of cptr (absolute values: the kernel subtracts the first) and its candidates, and one launch, timed in
// "recommend/candidates", writes the finished lists, which are copied to items / scores (n x K).  v.allow as in rec_run.
static const int64_t CAND_BATCH = (int64_t)1 << 24, CAND_ITEMS = (int64_t)1 << 26;
template <typename T>
static int cand_run(const ServeView& v, int64_t n, const int32_t* h_users, const int64_t* cptr, const int32_t* citem, int K, int32_t* items,
                    double* scores) {
    if (n <= 0) return PCR_OK;
    hipStream_t st = v.st;
    const int64_t nb = std::min(n, std::max<int64_t>(4, CAND_BATCH / K));
    DBuf<int32_t> du, dc, oi;
    DBuf<int64_t> dp;
    DBuf<double> os;
    RC(du.alloc((size_t)nb)); RC(dp.alloc((size_t)nb + 1)); RC(oi.alloc((size_t)nb * K)); RC(os.alloc((size_t)nb * K));
    const size_t lds = cand_wave_lds<T>(K) * 4;
    HIPCHK(hipFuncSetAttribute((const void*)k_rec_cand<T, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    std::vector<int32_t> seq;
    for (int64_t b0 = 0; b0 < n;) {
        int64_t m = 1;
        while (m < nb && b0 + m < n && cptr[b0 + m + 1] - cptr[b0] <= CAND_ITEMS) ++m;
        const int64_t nc = cptr[b0 + m] - cptr[b0];
        const int32_t* hu = h_users ? h_users + b0 : nullptr;
        if (!hu) { seq.resize((size_t)m); for (int64_t i = 0; i < m; ++i) seq[(size_t)i] = (int32_t)(b0 + i); hu = seq.data(); }
        if (dc.n < (size_t)nc) RC(dc.alloc((size_t)nc));
        HIPCHK(hipMemcpyAsync(du.p, hu, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(dp.p, cptr + b0, (size_t)(m + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
        if (nc > 0) HIPCHK(hipMemcpyAsync(dc.p, citem + cptr[b0], (size_t)nc * sizeof(int32_t), hipMemcpyHostToDevice, st));
        {
            ProfScope ps(v.prof, "recommend/candidates", st);
            hipLaunchKernelGGL((k_rec_cand<T, false>), dim3((unsigned)cdiv(m, 4)), dim3(256), lds, st, serve_U<T>(v), serve_V<T>(v), v.r, v.ld,
                               (const int32_t*)du.p, m, (const int64_t*)dp.p, (const int32_t*)dc.p, v.allow, v.xptr(), v.xitem(), K, oi.p, os.p,
                               TopnArgs{});
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipMemcpyAsync(items + b0 * K, oi.p, (size_t)m * K * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(scores + b0 * K, os.p, (size_t)m * K * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));                  // (the next batch overwrites du / dp / dc / seq)
        b0 += m;
    }
    return PCR_OK;
}

static int no_more() { return PCR_OK; }
// The end of an evaluation: the fixed-order sums over the n per-user rows met[n][ncut][6] into sums[ncut * 8 + 1] ([ncut][8], then the
// count: k_topn_sum1 / k_topn_fin's two stages, one block row per cutoff; timed in v.prof's `slot`), summed across the ranks and read
// back into hs once v.wait() has synchronised.  A caller with more to finish (div_run's exposure) launches it from in_slot(), in
// the slot's scope, and exchanges it and queues its read-backs in before_wait().
template <class InSlot = int (*)(), class BeforeWait = int (*)()>
static int met_sums(const ServeView& v, const char* slot, const double* met, int64_t n, int ncut, DBuf<double>& part, double* sums, double* hs,
                    InSlot&& in_slot = no_more, BeforeWait&& before_wait = no_more) {
    {
        ProfScope ps(v.prof, slot, v.st);
        const int nb = (int)std::min<int64_t>(512, std::max<int64_t>(1, cdiv(n, 2048)));
        const int per = cdiv(std::max<int64_t>(n, 1), nb);
        if (part.n < (size_t)nb * ncut * 8) RC(part.alloc((size_t)nb * ncut * 8));
        hipLaunchKernelGGL(k_topn_sum1, dim3(nb, ncut), dim3(PCR_EW_BLOCK), 0, v.st, met, n, ncut, per, part.p);
        hipLaunchKernelGGL(k_topn_fin, dim3(ncut), dim3(PCR_EW_BLOCK), 0, v.st, (const double*)part.p, nb, n, sums);
        RC(in_slot());
        HIPCHK(hipGetLastError());
    }
    RC(v.sum(sums, (size_t)ncut * 8 + 1));
    RC(before_wait());
    HIPCHK(hipMemcpyAsync(hs, sums, ((size_t)ncut * 8 + 1) * sizeof(double), hipMemcpyDeviceToHost, v.st));
    return v.wait();
}

// Top-N evaluation's device tables (PcrTopnRel of pcr_host.h, uploaded once per (threshold, cutoffs)) and its outputs: the
// per-user metric rows met[n][ncut][6] of the counted users and the reduced sums [ncut][8] + the count (k_topn_fin)
struct TopnDev {
    PcrTopnRel rel;
    int ncut = 0;
    int cut[PCR_TOPN_MAX_CUTOFFS] = {};
    double threshold = 0.0;
    bool valid = false;
    DBuf<int64_t> rptr;
    DBuf<int32_t> ritem;
    DBuf<double> rgain, idcg, disc, met, part, sums;
    bool same(int nc, const int* cuts, double thr) const {
        if (!valid || nc != ncut || !(thr == threshold)) return false;
        for (int c = 0; c < nc; ++c) if (cuts[c] != cut[c]) return false;
        return true;
    }
    // the relevance tables of rows [0, rows) of the test CSR, to the device
    int build(int64_t rows, const int64_t* tptr, const int32_t* titem, const double* tval, int nc, const int* cuts, double thr) {
        valid = false;
        pcr_topn_relevance(rows, tptr, titem, tval, thr, nc, cuts, rel);
        ncut = nc; threshold = thr;
        fill_cuts(cut, nc, cuts);
        RC(rptr.upload(rel.rptr, nullptr)); RC(ritem.upload(rel.ritem, nullptr)); RC(rgain.upload(rel.rgain, nullptr));
        RC(idcg.upload(rel.idcg, nullptr)); RC(disc.upload(rel.disc, nullptr));
        RC(met.alloc(rel.users.size() * (size_t)ncut * 6)); RC(sums.alloc((size_t)ncut * 8 + 1));
        valid = true;
        return PCR_OK;
    }
    // the tables and the output rows of the batch of counted users that starts at b0, for a kernel that counts from 0
    TopnArgs args(int64_t b0) const {
        TopnArgs ta;
        ta.rptr = rptr.p + b0; ta.ritem = ritem.p; ta.rgain = rgain.p; ta.idcg = idcg.p + (size_t)b0 * ncut * 2;
        ta.disc = disc.p; ta.out = met.p + (size_t)b0 * ncut * 6; ta.ncut = ncut;
        fill_cuts(ta.cut, ncut, cut);
        return ta;
    }
    // The end of an evaluation, after rec_run: met_sums over the counted users ("recommend/metrics") into stats; with per_user,
    // per_user[rows][ncut][6]: NaN, then the counted users' rows
    int finish(const ServeView& v, pcr_topn_stats* stats, double* per_user) {
        std::vector<double> hs((size_t)ncut * 8 + 1);
        RC(met_sums(v, "recommend/metrics", met.p, (int64_t)rel.users.size(), ncut, part, sums.p, hs.data()));
        pcr_topn_stats_from(hs.data(), ncut, cut, stats);
        if (!per_user) return PCR_OK;
        const size_t w = (size_t)ncut * 6;
        std::vector<double> h(rel.users.size() * w);
        if (!h.empty()) HIPCHK(hipMemcpyAsync(h.data(), met.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, v.st));
        HIPCHK(hipStreamSynchronize(v.st));
        std::fill(per_user, per_user + (size_t)v.rows * w, (double)NAN);
        for (size_t i = 0; i < rel.users.size(); ++i) std::copy(h.begin() + i * w, h.begin() + (i + 1) * w, per_user + (size_t)rel.users[i] * w);
        return PCR_OK;
    }
};

// rec_run's sink for the top-N evaluation: merge + metrics (k_rec_merge_topn) into d.met at the batch's rows
template <typename T>
struct RecTopn {
    const ServeView& v;
    int K;
    TopnDev& d;
    int begin(int64_t) { return PCR_OK; }
    int batch(int64_t b0, int64_t m, const T* ls, const int32_t* li, const int32_t* ln, int nsp) {
        const TopnArgs ta = d.args(b0);
        ProfScope ps(v.prof, "recommend/metrics", v.st);
        hipLaunchKernelGGL((k_rec_merge_topn<T>), dim3((unsigned)cdiv(m, 4)), dim3(256), (size_t)4 * K * sizeof(int32_t), v.st, ls, li, ln, nsp, m, K, ta);
        HIPCHK(hipGetLastError());
        return PCR_OK;
    }
};

// Beyond-accuracy metrics (pcr_evaluate_diversity, pcr_topk.h): the per-item tables and the outputs of one call -- the exposure
// counters [ncut][d2] (they live across rec_run's user batches and are zeroed once per call), the per-user rows met[n][ncut][6]
// in the column order k_topn_sum1 reduces, the reduced sums [ncut][8] + the count
struct DivDev {
    int ncut = 0;
    int cut[PCR_TOPN_MAX_CUTOFFS] = {};
    DBuf<double> inv, q, met, part, sums, expod;
    DBuf<unsigned long long> expo;
    const double* info = nullptr;
};

// rec_run's sink for the beyond-accuracy metrics: merge + exposure, novelty and ILD (k_rec_merge_div) into d.expo and d.met
template <typename T>
struct RecDiversity {
    const ServeView& v;
    int K;
    DivDev& d;
    int begin(int64_t) { return PCR_OK; }
    int batch(int64_t b0, int64_t m, const T* ls, const int32_t* li, const int32_t* ln, int nsp) {
        DivArgs da;
        da.inv = d.inv.p; da.q = d.q.p; da.info = d.info; da.expo = d.expo.p; da.out = d.met.p + (size_t)b0 * d.ncut * 6;
        da.d2 = v.d2; da.ncut = d.ncut;
        fill_cuts(da.cut, d.ncut, d.cut);
        ProfScope ps(v.prof, "recommend/diversity", v.st);
        hipLaunchKernelGGL((k_rec_merge_div<T>), dim3((unsigned)cdiv(m, 4)), dim3(256), (size_t)4 * K * sizeof(int32_t), v.st, ls, li, ln, nsp, m, K,
                           serve_V<T>(v), v.r, v.ld, da);
        HIPCHK(hipGetLastError());
        return PCR_OK;
    }
};

// info[] of v's training ratings item[0, nnz) on the device (NULL: pop = 0) into `info`: the counts by integer adds, summed
// across the ranks, the logarithms on the host (pcr_diversity_info), like the top-N discount table
static int div_info_build(const ServeView& v, DBuf<double>& info) {
    hipStream_t st = v.st;
    const int64_t d2 = v.d2;
    DBuf<unsigned long long> cnt;
    DBuf<double> pop;
    RC(cnt.alloc((size_t)d2)); RC(pop.alloc((size_t)d2));
    HIPCHK(hipMemsetAsync(cnt.p, 0, (size_t)d2 * sizeof(unsigned long long), st));
    if (v.item && v.nnz > 0)
        hipLaunchKernelGGL(k_div_pop, dim3((unsigned)std::min<int64_t>(4096, cdiv(v.nnz, 256))), dim3(256), 0, st, v.item, v.nnz, cnt.p);
    hipLaunchKernelGGL(k_div_pop_f64, dim3((unsigned)cdiv(d2, 256)), dim3(256), 0, st, (const unsigned long long*)cnt.p, d2, pop.p);
    HIPCHK(hipGetLastError());
    RC(v.sum(pop.p, (size_t)d2));
    std::vector<double> h((size_t)d2), hi((size_t)d2);
    HIPCHK(hipMemcpyAsync(h.data(), pop.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    RC(v.wait());
    pcr_diversity_info(v.d1, h.data(), d2, hi.data());
    RC(info.upload(hi, st));
    return PCR_OK;
}

// The beyond-accuracy evaluation of the n users h_users (rows of U and of the exclusion CSR, as rec_run; NULL: rows 0..n-1)
// with the self-information table info: the row norms, the sweep with RecDiversity, the fixed-order sums over the users
// (met_sums, unchanged) and the cumulative exposure; sums and exposure are summed across the ranks and read back once
// v.wait() has synchronised the stream.  "recommend/diversity" times everything but the score kernel.
template <typename T>
static int div_run(const ServeView& v, const double* info, int64_t n, const int32_t* h_users, int ncut, const int* cuts,
                   pcr_diversity_stats* stats, double* per_user, int64_t* exposure) {
    hipStream_t st = v.st;
    const int64_t d2 = v.d2;
    DivDev D;
    D.ncut = ncut; D.info = info;
    fill_cuts(D.cut, ncut, cuts);
    const int K = cuts[ncut - 1];
    RC(D.inv.alloc((size_t)d2)); RC(D.q.alloc((size_t)d2)); RC(D.expo.alloc((size_t)ncut * d2)); RC(D.expod.alloc((size_t)ncut * d2));
    RC(D.met.alloc((size_t)n * ncut * 6)); RC(D.sums.alloc((size_t)ncut * 8 + 1));
    {
        ProfScope ps(v.prof, "recommend/diversity", st);
        HIPCHK(hipMemsetAsync(D.expo.p, 0, (size_t)ncut * d2 * sizeof(unsigned long long), st));
        hipLaunchKernelGGL((k_div_prepare<T>), dim3((unsigned)cdiv(d2, 4)), dim3(256), 0, st, serve_V<T>(v), v.r, v.ld, d2, D.inv.p, D.q.p);
        HIPCHK(hipGetLastError());
    }
    RC(rec_run<T>(v, n, h_users, K, 1, RecDiversity<T>{v, K, D}));
    std::vector<double> hs((size_t)ncut * 8 + 1), he((size_t)ncut * d2), hm;
    RC(met_sums(v, "recommend/diversity", D.met.p, n, ncut, D.part, D.sums.p, hs.data(),
                [&]() -> int {   // (the exposure counters as doubles, in the same slot)
                    hipLaunchKernelGGL(k_div_expo_finish, dim3((unsigned)cdiv(d2, 256)), dim3(256), 0, st, (const unsigned long long*)D.expo.p, d2, ncut, D.expod.p);
                    return PCR_OK;
                },
                [&]() -> int {
                    RC(v.sum(D.expod.p, (size_t)ncut * d2));
                    HIPCHK(hipMemcpyAsync(he.data(), D.expod.p, he.size() * sizeof(double), hipMemcpyDeviceToHost, st));
                    if (per_user && n > 0) {
                        hm.resize((size_t)n * ncut * 6);
                        HIPCHK(hipMemcpyAsync(hm.data(), D.met.p, hm.size() * sizeof(double), hipMemcpyDeviceToHost, st));
                    }
                    return PCR_OK;
                }));
    RC(pcr_diversity_stats_from(hs.data(), ncut, cuts, he.data(), d2, stats, exposure));
    for (size_t i = 0; i < hm.size() / 6; ++i) {           // met: len, novelty (0 when len = 0), -, -, -, ild
        const double* m = hm.data() + i * 6;
        double* o = per_user + i * PCR_DIVERSITY_FIELDS;
        o[0] = m[0]; o[1] = m[0] > 0.0 ? m[1] : (double)NAN; o[2] = m[5];
    }
    return PCR_OK;
}

// MMR re-ranking (pcr_recommend_diverse, pcr_topk.h): the form and the workgroup shape of k_rec_merge_mmr for a pool of K rows
// of ld values.  The streaming form is the default: it was the faster one at every shape measured.
// pcr_tune("rerank_lds", "1") takes the LDS form, which stages the pool's rows, whenever one wave's image fits a workgroup's
// 160 KiB.  waves = users per workgroup (4, 2 or 1, as many as fit).
struct MmrShape { int form = 0, waves = 0; size_t lds = 0; };
template <typename T>
static MmrShape mmr_shape(int K, int ld, int knob) {
    MmrShape s;
    s.form = (knob > 0 && mmr_wave_lds<T>(K, ld, 1) <= PCR_LDS_CU) ? 1 : 0;
    const size_t per = mmr_wave_lds<T>(K, ld, s.form);
    for (int w = 4; w >= 1; w >>= 1) if ((size_t)w * per <= PCR_LDS_CU) { s.waves = w; break; }
    s.lds = (size_t)s.waves * per;
    return s;
}

// rec_run's sink for the re-ranking: merge + greedy selection (k_rec_merge_mmr) of topk from the pool of K, to the host arrays
// items / scores (n x topk)
template <typename T>
struct RecRerank {
    const ServeView& v;
    int K, topk;
    double theta;
    const double* inv;
    MmrShape shape;
    int32_t* items;
    double* scores;
    DBuf<int32_t> oi;
    DBuf<double> os;
    int begin(int64_t nb) { RC(oi.alloc((size_t)nb * topk)); RC(os.alloc((size_t)nb * topk)); return PCR_OK; }
    int batch(int64_t b0, int64_t m, const T* ls, const int32_t* li, const int32_t* ln, int nsp) {
        hipStream_t st = v.st; const T* V = serve_V<T>(v);
        const int r = v.r, ld = v.ld;
        MmrArgs ma;
        ma.inv = inv; ma.out_i = oi.p; ma.out_s = os.p; ma.topk = topk; ma.theta = theta;
        {
            ProfScope ps(v.prof, "recommend/rerank", st);
            const dim3 grid((unsigned)cdiv(m, shape.waves)), block(64 * shape.waves);
            if (shape.form) hipLaunchKernelGGL((k_rec_merge_mmr<T, 1>), grid, block, shape.lds, st, ls, li, ln, nsp, m, K, V, r, ld, ma);
            else hipLaunchKernelGGL((k_rec_merge_mmr<T, 0>), grid, block, shape.lds, st, ls, li, ln, nsp, m, K, V, r, ld, ma);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipMemcpyAsync(items + b0 * topk, oi.p, (size_t)m * topk * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(scores + b0 * topk, os.p, (size_t)m * topk * sizeof(double), hipMemcpyDeviceToHost, st));
        return PCR_OK;
    }
};

// The re-ranked lists of the n users h_users (rows of U and of the exclusion CSR, as rec_run; NULL: rows 0..n-1): the row norms
// (k_div_prepare, as the ILD's), then the sweep with K = pool and RecRerank.  "recommend/rerank" times everything but the
// score kernel.  pcr_tune("rerank_lds") is read at every call.  k_div_prepare is reused as it is, so its second table q[d2] (the
// ILD's |v^_j|^2) is allocated and written here too although the re-ranking never reads it: one d2-sized buffer per call.
template <typename T>
static int rerank_run(const ServeView& v, int64_t n, const int32_t* h_users, int topk, int pool, double theta, int32_t* items, double* scores) {
    if (n <= 0) return PCR_OK;
    const MmrShape shape = mmr_shape<T>(pool, v.ld, pcr_tune_int("rerank_lds", 0));
    if (shape.waves < 1) { pcr_set_error("pcr_recommend_diverse: rank " + std::to_string(v.r) + " is too large for the re-ranking kernel's LDS"); return PCR_ERR_UNSUPPORTED; }
    DBuf<double> inv, q;
    RC(inv.alloc((size_t)v.d2)); RC(q.alloc((size_t)v.d2));
    if (shape.form) HIPCHK(hipFuncSetAttribute((const void*)k_rec_merge_mmr<T, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shape.lds));
    else HIPCHK(hipFuncSetAttribute((const void*)k_rec_merge_mmr<T, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shape.lds));
    {
        ProfScope ps(v.prof, "recommend/rerank", v.st);
        hipLaunchKernelGGL((k_div_prepare<T>), dim3((unsigned)cdiv(v.d2, 4)), dim3(256), 0, v.st, serve_V<T>(v), v.r, v.ld, v.d2, inv.p, q.p);
        HIPCHK(hipGetLastError());
    }
    return rec_run<T>(v, n, h_users, pool, 1, RecRerank<T>{v, pool, topk, theta, inv.p, shape, items, scores});
}

// rec_run's sink for the group cap: merge + selection (k_rec_merge_cap) of topk from the pool of K, to the host arrays items /
// scores (n x topk) and status (n)
template <typename T>
struct RecCap {
    const ServeView& v;
    int K, topk, cap;
    const int32_t* group;         // device, [d2]
    int32_t* items;
    double* scores;
    uint8_t* status;
    DBuf<int32_t> oi;
    DBuf<double> os;
    DBuf<unsigned char> ost;
    int begin(int64_t nb) {
        RC(oi.alloc((size_t)nb * topk)); RC(os.alloc((size_t)nb * topk)); RC(ost.alloc((size_t)nb));
        HIPCHK(hipFuncSetAttribute((const void*)k_rec_merge_cap<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(cap_wave_lds<T>(K) * 4)));
        return PCR_OK;
    }
    int batch(int64_t b0, int64_t m, const T* ls, const int32_t* li, const int32_t* ln, int nsp) {
        hipStream_t st = v.st;
        {
            ProfScope ps(v.prof, "recommend/cap", st);
            hipLaunchKernelGGL((k_rec_merge_cap<T>), dim3((unsigned)cdiv(m, 4)), dim3(256), cap_wave_lds<T>(K) * 4, st, ls, li, ln, nsp, m, K, group,
                               cap, topk, oi.p, os.p, ost.p);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipMemcpyAsync(items + b0 * topk, oi.p, (size_t)m * topk * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(scores + b0 * topk, os.p, (size_t)m * topk * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(status + b0, ost.p, (size_t)m, hipMemcpyDeviceToHost, st));
        return PCR_OK;
    }
};

// The group-capped lists of the n users h_users (rows of U and of the exclusion CSR, as rec_run; NULL: rows 0..n-1): group[d2]
// goes to the device once per call, then the sweep with K = pool and RecCap.  "recommend/cap" times the merge with the selection
// fused in.  status is never NULL here (serve_recommend_capped brings its own when the caller has none).
template <typename T>
static int cap_run(const ServeView& v, int64_t n, const int32_t* h_users, int topk, int pool, const int32_t* group, int cap, int32_t* items,
                   double* scores, uint8_t* status) {
    if (n <= 0) return PCR_OK;
    DBuf<int32_t> dg;
    RC(dg.upload_n(group, (size_t)v.d2));
    return rec_run<T>(v, n, h_users, pool, 1, RecCap<T>{v, pool, topk, cap, dg.p, items, scores, status});
}

// Metrics of device-resident lists (pcr_evaluate_lists_model, pcr_evaluate_rerank; k_list_metrics of pcr_topk.h, DESIGN.md
// section 3.15): the tables and outputs of one evaluation of `groups` sets of n lists of length L (the caller's lists: one
// group; the theta sweep: one per theta).  The relevance tables have a row for every request (pcr_list_relevance; acc = false:
// no accuracy part); the per-item tables are DivDev's; the exposure counters [groups][ncut][d2] are zeroed once per call; the
// per-user rows dmet / tmet are [groups][n][ncut][6] in the column order k_topn_sum1 reduces.  "recommend/listmetrics" times the
// row norms, the metric kernel and the reductions.
struct ListEval {
    int ncut = 0, groups = 1, L = 0;
    int cut[PCR_TOPN_MAX_CUTOFFS] = {};
    int64_t n = 0, d2 = 0, counted = 0;
    bool acc = false;
    PcrTopnRel rel;
    DBuf<int64_t> rptr;
    DBuf<int32_t> ritem;
    DBuf<double> rgain, idcg, disc, inv, q, dmet, tmet, part, sums, expod;
    DBuf<unsigned long long> expo;
    const double* info = nullptr;
    static constexpr const char* SLOT = "recommend/listmetrics";

    // h_users: the requests as rows of v's test CSR (NULL: rows 0..n-1)
    template <typename T>
    int begin(const ServeView& v, const double* info_, bool acc_, int64_t n_, const int32_t* h_users, int L_, int groups_, int nc,
              const int* cuts, double thr) {
        info = info_; acc = acc_; n = n_; L = L_; groups = groups_; ncut = nc; d2 = v.d2;
        fill_cuts(cut, nc, cuts);
        const size_t g = (size_t)groups;
        if (acc) {
            counted = pcr_list_relevance(v.rows, v.tptr, v.titem, v.tval, thr, nc, cuts, n, h_users, L, rel);
            RC(rptr.upload(rel.rptr, nullptr)); RC(ritem.upload(rel.ritem, nullptr)); RC(rgain.upload(rel.rgain, nullptr));
            RC(idcg.upload(rel.idcg, nullptr)); RC(disc.upload(rel.disc, nullptr));
            RC(tmet.alloc(g * (size_t)n * ncut * 6));
        }
        RC(inv.alloc((size_t)d2)); RC(q.alloc((size_t)d2)); RC(expo.alloc(g * ncut * d2)); RC(expod.alloc(g * ncut * d2));
        RC(dmet.alloc(g * (size_t)n * ncut * 6)); RC(sums.alloc((size_t)ncut * 8 + 1));
        ProfScope ps(v.prof, SLOT, v.st);
        HIPCHK(hipMemsetAsync(expo.p, 0, g * ncut * d2 * sizeof(unsigned long long), v.st));
        hipLaunchKernelGGL((k_div_prepare<T>), dim3((unsigned)cdiv(d2, 4)), dim3(256), 0, v.st, serve_V<T>(v), v.r, v.ld, d2, inv.p, q.p);
        HIPCHK(hipGetLastError());
        return PCR_OK;
    }
    // the metrics of the m lists dlists[m][L] (device) of group g, requests [b0, b0 + m)
    template <typename T>
    int launch(const ServeView& v, int g, int64_t b0, int64_t m, const int32_t* dlists) {
        const size_t row0 = (size_t)g * (size_t)n + (size_t)b0;
        DivArgs da;
        da.inv = inv.p; da.q = q.p; da.info = info; da.expo = expo.p + (size_t)g * ncut * d2; da.out = dmet.p + row0 * ncut * 6;
        da.d2 = d2; da.ncut = ncut;
        fill_cuts(da.cut, ncut, cut);
        TopnArgs ta = {};
        if (acc) {
            ta.rptr = rptr.p + b0; ta.ritem = ritem.p; ta.rgain = rgain.p; ta.idcg = idcg.p + (size_t)b0 * ncut * 2;
            ta.disc = disc.p; ta.out = tmet.p + row0 * ncut * 6;
        }
        ta.ncut = ncut;
        fill_cuts(ta.cut, ncut, cut);
        ProfScope ps(v.prof, SLOT, v.st);
        hipLaunchKernelGGL((k_list_metrics<T>), dim3((unsigned)cdiv(m, 4)), dim3(256), (size_t)4 * L * sizeof(int32_t), v.st, dlists, m, L,
                           serve_V<T>(v), v.r, v.ld, ta, da);
        HIPCHK(hipGetLastError());
        return PCR_OK;
    }
    // The end of the evaluation: per group met_sums over the n diversity rows (with the cumulative exposure, as div_run) and, with
    // an accuracy part, over the n accuracy rows -- an uncounted request's row adds nothing to any sum, and the count k_topn_fin
    // leaves behind (n) is replaced by the counted requests before the exchange.  topn / div are [groups][ncut]; the optional
    // per_user_topn [groups][n][ncut][6] (NaN for an uncounted request), per_user_div [groups][n][ncut][3], exposure [groups][ncut][d2].
    int finish(const ServeView& v, const int* cuts, pcr_topn_stats* topn, pcr_diversity_stats* div, double* per_user_topn, double* per_user_div,
               int64_t* exposure) {
        hipStream_t st = v.st;
        const size_t w = (size_t)ncut * 6, rows = (size_t)n * w, ex = (size_t)ncut * d2;
        std::vector<double> hs((size_t)ncut * 8 + 1), he(ex), hm;
        const double cnt = (double)counted;
        for (int g = 0; g < groups; ++g) {
            const unsigned long long* eg = expo.p + (size_t)g * ex;
            double* ed = expod.p + (size_t)g * ex;
            hm.clear();
            RC(met_sums(v, SLOT, dmet.p + (size_t)g * rows, n, ncut, part, sums.p, hs.data(),
                        [&]() -> int {
                            hipLaunchKernelGGL(k_div_expo_finish, dim3((unsigned)cdiv(d2, 256)), dim3(256), 0, st, eg, d2, ncut, ed);
                            return PCR_OK;
                        },
                        [&]() -> int {
                            RC(v.sum(ed, ex));
                            HIPCHK(hipMemcpyAsync(he.data(), ed, ex * sizeof(double), hipMemcpyDeviceToHost, st));
                            if (per_user_div && n > 0) {
                                hm.resize(rows);
                                HIPCHK(hipMemcpyAsync(hm.data(), dmet.p + (size_t)g * rows, rows * sizeof(double), hipMemcpyDeviceToHost, st));
                            }
                            return PCR_OK;
                        }));
            RC(pcr_diversity_stats_from(hs.data(), ncut, cuts, he.data(), d2, div + (size_t)g * ncut, exposure ? exposure + (size_t)g * ex : nullptr));
            for (size_t i = 0; i < hm.size() / 6; ++i) {       // met: len, novelty (0 when len = 0), -, -, -, ild
                const double* m = hm.data() + i * 6;
                double* o = per_user_div + ((size_t)g * (size_t)n * ncut + i) * PCR_DIVERSITY_FIELDS;
                o[0] = m[0]; o[1] = m[0] > 0.0 ? m[1] : (double)NAN; o[2] = m[5];
            }
            if (!acc) continue;
            hm.clear();
            RC(met_sums(v, SLOT, tmet.p + (size_t)g * rows, n, ncut, part, sums.p, hs.data(),
                        [&]() -> int {
                            HIPCHK(hipMemcpyAsync(sums.p + (size_t)ncut * 8, &cnt, sizeof(double), hipMemcpyHostToDevice, st));
                            return PCR_OK;
                        },
                        [&]() -> int {
                            if (per_user_topn && n > 0) {
                                hm.resize(rows);
                                HIPCHK(hipMemcpyAsync(hm.data(), tmet.p + (size_t)g * rows, rows * sizeof(double), hipMemcpyDeviceToHost, st));
                            }
                            return PCR_OK;
                        }));
            pcr_topn_stats_from(hs.data(), ncut, cut, topn + (size_t)g * ncut);
            for (size_t i = 0; i < hm.size() / w; ++i) {
                double* o = per_user_topn + (size_t)g * rows + i * w;
                if (rel.rptr[i + 1] > rel.rptr[i]) std::copy(hm.begin() + i * w, hm.begin() + (i + 1) * w, o);
                else std::fill(o, o + w, (double)NAN);
            }
        }
        return PCR_OK;
    }
};

// pcr_evaluate_lists_model: the caller's lists[n][L] go to the device in batches of at most LIST_BATCH entries, each batch
// through k_list_metrics
static const int64_t LIST_BATCH = (int64_t)1 << 24;
template <typename T>
static int lists_run(const ServeView& v, const double* info, int64_t n, const int32_t* h_users, int L, const int32_t* lists, int ncut,
                     const int* cuts, double thr, bool acc, pcr_topn_stats* topn, double* per_user_topn, pcr_diversity_stats* div,
                     double* per_user_div, int64_t* exposure) {
    ListEval E;
    RC(E.begin<T>(v, info, acc, n, h_users, L, 1, ncut, cuts, thr));
    const int64_t nb = std::max<int64_t>(4, LIST_BATCH / L);
    DBuf<int32_t> dl;
    RC(dl.alloc((size_t)std::min(nb, n) * L));
    for (int64_t b0 = 0; b0 < n; b0 += nb) {
        const int64_t m = std::min(nb, n - b0);
        HIPCHK(hipMemcpyAsync(dl.p, lists + (size_t)b0 * L, (size_t)m * L * sizeof(int32_t), hipMemcpyHostToDevice, v.st));
        RC(E.launch<T>(v, 0, b0, m, dl.p));
        HIPCHK(hipStreamSynchronize(v.st));                // (the next batch overwrites dl)
    }
    return E.finish(v, cuts, topn, div, per_user_topn, per_user_div, exposure);
}

// rec_run's sink for the theta sweep (pcr_evaluate_rerank): per theta the merge + greedy selection (k_rec_merge_mmr, exactly
// RecRerank's launch) into the device lists oi [nb][topk], then their metrics (k_list_metrics) into group t of E.  The score
// kernel has run once for the batch, whatever nth is.
template <typename T>
struct RecTradeoff {
    const ServeView& v;
    int K, topk, nth;
    const double* thetas;
    MmrShape shape;
    ListEval& E;
    DBuf<int32_t> oi;
    DBuf<double> os;
    int begin(int64_t nb) { RC(oi.alloc((size_t)nb * topk)); RC(os.alloc((size_t)nb * topk)); return PCR_OK; }
    int batch(int64_t b0, int64_t m, const T* ls, const int32_t* li, const int32_t* ln, int nsp) {
        hipStream_t st = v.st; const T* V = serve_V<T>(v);
        const int r = v.r, ld = v.ld;
        for (int t = 0; t < nth; ++t) {
            MmrArgs ma;
            ma.inv = E.inv.p; ma.out_i = oi.p; ma.out_s = os.p; ma.topk = topk; ma.theta = thetas[t];
            {
                ProfScope ps(v.prof, "recommend/rerank", st);
                const dim3 grid((unsigned)cdiv(m, shape.waves)), block(64 * shape.waves);
                if (shape.form) hipLaunchKernelGGL((k_rec_merge_mmr<T, 1>), grid, block, shape.lds, st, ls, li, ln, nsp, m, K, V, r, ld, ma);
                else hipLaunchKernelGGL((k_rec_merge_mmr<T, 0>), grid, block, shape.lds, st, ls, li, ln, nsp, m, K, V, r, ld, ma);
                HIPCHK(hipGetLastError());
            }
            RC(E.launch<T>(v, t, b0, m, oi.p));
        }
        return PCR_OK;
    }
};

// The sweep over the n users h_users (rows of U, of the exclusion CSR and of the test CSR, as rec_run; NULL: rows 0..n-1): the
// row norms and the tables once (ListEval::begin), one rec_run with K = pool and RecTradeoff, the reductions per theta.
// pcr_tune("rerank_lds") is read at every call, as rerank_run does.
template <typename T>
static int tradeoff_run(const char* who, const ServeView& v, const double* info, int64_t n, const int32_t* h_users, int nth, const double* thetas,
                        int pool, int ncut, const int* cuts, double thr, bool acc, pcr_topn_stats* topn, pcr_diversity_stats* div,
                        double* per_user_topn, double* per_user_div, int64_t* exposure) {
    const int topk = cuts[ncut - 1];
    const MmrShape shape = mmr_shape<T>(pool, v.ld, pcr_tune_int("rerank_lds", 0));
    if (shape.waves < 1) { pcr_set_error(std::string(who) + ": rank " + std::to_string(v.r) + " is too large for the re-ranking kernel's LDS"); return PCR_ERR_UNSUPPORTED; }
    if (shape.form) HIPCHK(hipFuncSetAttribute((const void*)k_rec_merge_mmr<T, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shape.lds));
    else HIPCHK(hipFuncSetAttribute((const void*)k_rec_merge_mmr<T, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shape.lds));
    ListEval E;
    RC(E.begin<T>(v, info, acc, n, h_users, topk, nth, ncut, cuts, thr));
    RC(rec_run<T>(v, n, h_users, pool, 1, RecTradeoff<T>{v, pool, topk, nth, thetas, shape, E, {}, {}}));
    return E.finish(v, cuts, topn, div, per_user_topn, per_user_div, exposure);
}

// Exact rank metrics (pcr_evaluate_ranks, pcr_topk.h): the relevance table of a threshold on the device (PcrTopnRel's users,
// rptr and ritem; uploaded once per threshold) and the outputs: rrank[nrel] the ranks of ritem entry for entry, met[n][6]
// k_rank_finish's rows, the reduced sums [8] + the count
struct RankDev {
    PcrTopnRel rel;
    double threshold = 0.0;
    bool valid = false;
    DBuf<int64_t> rptr, rrank;
    DBuf<int32_t> ritem, rslot, users;
    DBuf<double> met, part, sums;
    bool same(double thr) const { return valid && thr == threshold; }
    int build(int64_t rows, const int64_t* tptr, const int32_t* titem, const double* tval, double thr) {
        valid = false;
        const int one = 1;
        pcr_topn_relevance(rows, tptr, titem, tval, thr, 1, &one, rel);
        threshold = thr;
        RC(rptr.upload(rel.rptr, nullptr)); RC(ritem.upload(rel.ritem, nullptr)); RC(users.upload(rel.users, nullptr));
        RC(rslot.alloc(rel.ritem.size())); RC(rrank.alloc(rel.ritem.size()));
        RC(met.alloc(rel.users.size() * 6)); RC(sums.alloc(9));
        valid = true;
        return PCR_OK;
    }
    // The end of an evaluation, after rank_run: met_sums with one "cutoff" ("ranks/finish"; the same two kernels sum met's
    // columns), then per_user[rows][PCR_RANK_FIELDS] and ranks[] of v's test CSR (the rows of this table's build)
    int finish(const ServeView& v, pcr_rank_stats* stats, double* per_user, int64_t* ranks) {
        hipStream_t st = v.st;
        const int64_t n = (int64_t)rel.users.size();
        double hs[9];
        RC(met_sums(v, "ranks/finish", met.p, n, 1, part, sums.p, hs));
        pcr_rank_stats_from(hs, stats);
        if (per_user) {
            std::vector<double> h((size_t)n * 6);
            if (n) HIPCHK(hipMemcpyAsync(h.data(), met.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            std::fill(per_user, per_user + (size_t)v.rows * PCR_RANK_FIELDS, (double)NAN);
            for (int64_t i = 0; i < n; ++i) {           // met: |R_u|, rr, mean_rank, mpr, first_rank, auc
                const double* m = h.data() + (size_t)i * 6;
                double* o = per_user + (size_t)rel.users[(size_t)i] * PCR_RANK_FIELDS;
                o[0] = m[4]; o[1] = m[1]; o[2] = m[2]; o[3] = m[5]; o[4] = m[3];
            }
        }
        if (ranks) {
            std::vector<int64_t> h(rel.ritem.size());
            if (!h.empty()) HIPCHK(hipMemcpyAsync(h.data(), rrank.p, h.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            pcr_rank_scatter(v.rows, v.tptr, v.titem, v.tval, threshold, rel, h.data(), ranks);
        }
        return PCR_OK;
    }
};

// the relevant items' scores and their sort for all counted users of d ("ranks/relscore"): rs / ri the sorted rows, d.rslot
template <typename T>
static int rank_relsort(const ServeView& v, RankDev& d, DBuf<T>& us, DBuf<T>& rs, DBuf<int32_t>& ri) {
    hipStream_t st = v.st;
    const int64_t n = (int64_t)d.rel.users.size(), nrel = (int64_t)d.rel.ritem.size();
    RC(us.alloc((size_t)nrel)); RC(rs.alloc((size_t)nrel)); RC(ri.alloc((size_t)nrel));
    ProfScope ps(v.prof, "ranks/relscore", st);
    hipLaunchKernelGGL((k_rank_relscore<T>), dim3((unsigned)cdiv(n, 4)), dim3(256), 0, st, serve_U<T>(v), serve_V<T>(v), v.r, v.ld,
                       (const int32_t*)d.users.p, n, (const int64_t*)d.rptr.p, (const int32_t*)d.ritem.p, us.p);
    hipLaunchKernelGGL((k_rank_sort<T>), dim3((unsigned)cdiv(n, 4)), dim3(256), 0, st, n, (const int64_t*)d.rptr.p, (const int32_t*)d.ritem.p,
                       (const T*)us.p, rs.p, ri.p, d.rslot.p);
    HIPCHK(hipGetLastError());
    return PCR_OK;
}

// The rank metrics' sweep for the counted users of d (rows of U and of the exclusion CSR, as rec_run): the relevant items'
// scores and their sort once for all users ("ranks/relscore"), then per user batch (RecGeom, the scratch being the splits'
// histograms: |R_u| + 1 counters per user) the counting sweep ("ranks/count") and the scan ("ranks/finish") into d.rrank / d.met.
// pcr_tune("ranks_batch_users") is read at every call.  v.allow (NULL but in a filtered call) goes to the counting sweep as it is.
template <typename T>
static int rank_run(const ServeView& v, RankDev& d) {
    hipStream_t st = v.st; const T *U = serve_U<T>(v), *V = serve_V<T>(v);
    const int r = v.r, ld = v.ld;
    const int64_t d2 = v.d2, n = (int64_t)d.rel.users.size(), nrel = (int64_t)d.rel.ritem.size();
    if (n <= 0) return PCR_OK;
    DBuf<T> us, rs;
    DBuf<int32_t> ri, hist;
    RC(rank_relsort<T>(v, d, us, rs, ri));
    RecGeom geom(n, d2, sizeof(int32_t) * (size_t)((nrel + n + n - 1) / n));
    const int64_t cap = pcr_tune_int("ranks_batch_users", 0);
    if (cap > 0) {
        geom.nb = std::min(geom.nb, (cap + RecGeom::users_per_wg - 1) / RecGeom::users_per_wg * RecGeom::users_per_wg);
        geom.smax = geom.splits_for(std::min(geom.nb, n));
    }
    const std::vector<int64_t>& rp = d.rel.rptr;
    auto buckets = [&](int64_t b0, int64_t m) { return rp[(size_t)(b0 + m)] - rp[(size_t)b0] + m; };
    size_t hmax = 0;
    for (int64_t b0 = 0; b0 < n; b0 += geom.nb) hmax = std::max(hmax, (size_t)buckets(b0, std::min(geom.nb, n - b0)));
    RC(hist.alloc(hmax * (size_t)geom.smax));
    const size_t lds = rank_wave_lds<T>() * rec::WAVES;
    for (int64_t b0 = 0; b0 < n; b0 += geom.nb) {
        const int64_t m = std::min(geom.nb, n - b0), hsplit = buckets(b0, m);
        int per, nsp;
        geom.batch(m, &per, &nsp);
        {
            ProfScope ps(v.prof, "ranks/count", st);
            HIPCHK(hipMemsetAsync(hist.p, 0, (size_t)nsp * (size_t)hsplit * sizeof(int32_t), st));
            hipLaunchKernelGGL((k_rank_count<T>), dim3((unsigned)cdiv(m, RecGeom::users_per_wg), (unsigned)nsp), dim3(rec::WAVES * 64), lds, st, U, V,
                               r, ld, (int)d2, (const int32_t*)d.users.p + b0, m, v.xptr(), v.xitem(), per, (const int64_t*)d.rptr.p + b0, (const T*)rs.p,
                               (const int32_t*)ri.p, hist.p, hsplit, v.allow);
            HIPCHK(hipGetLastError());
        }
        ProfScope ps(v.prof, "ranks/finish", st);
        hipLaunchKernelGGL(k_rank_finish, dim3((unsigned)cdiv(m, 4)), dim3(256), 0, st, (const int32_t*)hist.p, hsplit, nsp, m,
                           (const int64_t*)d.rptr.p + b0, (const int32_t*)d.rslot.p, d.rrank.p, d.met.p + (size_t)b0 * 6);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(st));                      // (us / rs / ri / hist are freed on return)
    return PCR_OK;
}

// Filtered evaluation with candidate rows: the batches of cand_run over the candidate rows of the counted
// users `users` (ascending rows of f's candidate CSR, and of v's U and exclusion CSR).  A batch uploads its users, its rows'
// pointers (absolute values: the kernels subtract the first) and its candidates -- straight from the caller's arrays when the
// batch's users are consecutive rows, which every batch is when all users are counted; gathered into a staging row otherwise --
// then launch(b0, m, users, cptr, citem) -- device pointers, counted from the batch's start -- queues the batch's kernels; the
// stream is synchronised before the next batch overwrites the uploads.
template <class Launch>
static int cand_batches(const ServeView& v, const std::vector<int32_t>& users, const pcr_item_filter& f, int64_t nb, Launch&& launch) {
    hipStream_t st = v.st;
    const int64_t n = (int64_t)users.size();
    const int64_t* cp = f.cand_ptr;
    auto len = [&](int64_t i) { return cp[users[(size_t)i] + 1] - cp[users[(size_t)i]]; };
    nb = std::min(n, std::max<int64_t>(4, nb));
    DBuf<int32_t> du, dc;
    DBuf<int64_t> dp;
    RC(du.alloc((size_t)nb)); RC(dp.alloc((size_t)nb + 1));
    std::vector<int64_t> bptr;
    std::vector<int32_t> stage;
    for (int64_t b0 = 0; b0 < n;) {
        int64_t m = 1, nc = len(b0);
        while (m < nb && b0 + m < n && nc + len(b0 + m) <= CAND_ITEMS) { nc += len(b0 + m); ++m; }
        const int64_t* hp = cp + users[(size_t)b0];
        const int32_t* hc = f.cand_item + cp[users[(size_t)b0]];
        if ((int64_t)users[(size_t)(b0 + m - 1)] - users[(size_t)b0] != m - 1) {       // rows with gaps between them
            bptr.resize((size_t)m + 1); stage.resize((size_t)nc);
            bptr[0] = 0;
            for (int64_t i = 0; i < m; ++i) bptr[(size_t)i + 1] = bptr[(size_t)i] + len(b0 + i);
            pcr_parallel_ranges(m, pcr_host_threads(), [&](int, int64_t lo, int64_t hi) {
                for (int64_t i = lo; i < hi; ++i) {
                    const int32_t* row = f.cand_item + cp[users[(size_t)(b0 + i)]];
                    std::copy(row, row + len(b0 + i), stage.begin() + bptr[(size_t)i]);
                }
            });
            hp = bptr.data(); hc = stage.data();
        }
        if (dc.n < (size_t)nc) RC(dc.alloc((size_t)nc));
        HIPCHK(hipMemcpyAsync(du.p, users.data() + b0, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(dp.p, hp, (size_t)(m + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
        if (nc > 0) HIPCHK(hipMemcpyAsync(dc.p, hc, (size_t)nc * sizeof(int32_t), hipMemcpyHostToDevice, st));
        RC(launch(b0, m, (const int32_t*)du.p, (const int64_t*)dp.p, (const int32_t*)dc.p));
        HIPCHK(hipStreamSynchronize(st));
        b0 += m;
    }
    return PCR_OK;
}

// top-N within candidate rows: k_rec_cand's selection with the metrics tail, one launch per batch ("recommend/candidates_metrics"),
// into d.met at the batch's rows; no list leaves the device
template <typename T>
static int cand_topn_run(const ServeView& v, TopnDev& d, int K, const pcr_item_filter& f) {
    if (d.rel.users.empty()) return PCR_OK;
    const size_t lds = cand_wave_lds<T>(K) * 4;
    HIPCHK(hipFuncSetAttribute((const void*)k_rec_cand<T, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return cand_batches(v, d.rel.users, f, CAND_BATCH / K, [&](int64_t b0, int64_t m, const int32_t* du, const int64_t* dp, const int32_t* dc) -> int {
        ProfScope ps(v.prof, "recommend/candidates_metrics", v.st);
        hipLaunchKernelGGL((k_rec_cand<T, true>), dim3((unsigned)cdiv(m, 4)), dim3(256), lds, v.st, serve_U<T>(v), serve_V<T>(v), v.r, v.ld, du, m, dp, dc,
                           v.allow, v.xptr(), v.xitem(), K, (int32_t*)nullptr, (double*)nullptr, d.args(b0));
        HIPCHK(hipGetLastError());
        return PCR_OK;
    });
}

// rank metrics within candidate rows: rank_run with k_cand_count ("ranks/candidates") in place of the counting sweep -- one split,
// the batch's histogram zeroed before it, k_rank_finish ("ranks/finish") unchanged behind it
template <typename T>
static int cand_rank_run(const ServeView& v, RankDev& d, const pcr_item_filter& f) {
    hipStream_t st = v.st;
    const int64_t n = (int64_t)d.rel.users.size();
    if (n <= 0) return PCR_OK;
    DBuf<T> us, rs;
    DBuf<int32_t> ri, hist;
    RC(rank_relsort<T>(v, d, us, rs, ri));
    const std::vector<int64_t>& rp = d.rel.rptr;
    RC(cand_batches(v, d.rel.users, f, CAND_BATCH, [&](int64_t b0, int64_t m, const int32_t* du, const int64_t* dp, const int32_t* dc) -> int {
        const int64_t hsplit = rp[(size_t)(b0 + m)] - rp[(size_t)b0] + m;
        if (hist.n < (size_t)hsplit) RC(hist.alloc((size_t)hsplit));
        {
            ProfScope ps(v.prof, "ranks/candidates", st);
            HIPCHK(hipMemsetAsync(hist.p, 0, (size_t)hsplit * sizeof(int32_t), st));
            hipLaunchKernelGGL((k_cand_count<T>), dim3((unsigned)cdiv(m, 4)), dim3(256), 0, st, serve_U<T>(v), serve_V<T>(v), v.r, v.ld, du, m, dp, dc,
                               v.allow, v.xptr(), v.xitem(), (const int64_t*)d.rptr.p + b0, (const T*)rs.p, (const int32_t*)ri.p, hist.p);
            HIPCHK(hipGetLastError());
        }
        ProfScope ps(v.prof, "ranks/finish", st);
        hipLaunchKernelGGL(k_rank_finish, dim3((unsigned)cdiv(m, 4)), dim3(256), 0, st, (const int32_t*)hist.p, hsplit, 1, m,
                           (const int64_t*)d.rptr.p + b0, (const int32_t*)d.rslot.p, d.rrank.p, d.met.p + (size_t)b0 * 6);
        HIPCHK(hipGetLastError());
        return PCR_OK;
    }));
    HIPCHK(hipStreamSynchronize(st));                      // (us / rs / ri / hist are freed on return)
    return PCR_OK;
}

// ---- the five entries over a view, for a solver and for a model alike
static int serve_recommend(const ServeView& v, int64_t n, const int32_t* rows, int K, int32_t* items, double* scores) {
    return by_precision(v, [&](auto zero) -> int {
        using T = decltype(zero);
        return rec_run<T>(v, n, rows, K, v.select, RecCopy<T>{v, K, items, scores});
    });
}
// filtered lists (pcr_recommend_filtered): the allow set is packed into 64-bit words (bit j & 63 of word
// j >> 6) and hung on the view for this call; candidate lists take k_rec_cand alone, an allow set alone the sweep
static int pack_allow(ServeView& v, const pcr_item_filter& f, DBuf<unsigned long long>& aw) {
    if (!f.allow) return PCR_OK;
    std::vector<unsigned long long> w((size_t)((v.d2 + 63) >> 6), 0ull);
    for (int64_t j = 0; j < v.d2; ++j) if (f.allow[j]) w[(size_t)(j >> 6)] |= 1ull << (j & 63);
    RC(aw.upload(w, v.st));
    v.allow = aw.p;
    return PCR_OK;
}
static int serve_recommend_filtered(ServeView v, int64_t n, const int32_t* rows, int K, const pcr_item_filter& f, int32_t* items, double* scores) {
    if (n <= 0) return PCR_OK;
    DBuf<unsigned long long> aw;
    RC(pack_allow(v, f, aw));
    return by_precision(v, [&](auto zero) -> int {
        using T = decltype(zero);
        if (f.cand_ptr) return cand_run<T>(v, n, rows, f.cand_ptr, f.cand_item, K, items, scores);
        return rec_run<T>(v, n, rows, K, 1, RecCopy<T>{v, K, items, scores});
    });
}
// MMR re-ranked lists: per user, nothing is exchanged
static int serve_recommend_diverse(const ServeView& v, int64_t n, const int32_t* rows, int topk, int pool, double theta, int32_t* items,
                                   double* scores) {
    return by_precision(v, [&](auto zero) -> int { return rerank_run<decltype(zero)>(v, n, rows, topk, pool, theta, items, scores); });
}
// group-capped lists (pcr_recommend_capped): an allow set rides on the view as in
// serve_recommend_filtered; per user, nothing is exchanged; the summary is counted on the host from the finished rows
static int serve_recommend_capped(ServeView v, int64_t n, const int32_t* rows, int topk, int pool, const int32_t* group, int cap,
                                  const pcr_item_filter* f, int32_t* items, double* scores, uint8_t* status, pcr_cap_stats* stats) {
    std::vector<uint8_t> own;
    if (!status) { own.resize((size_t)std::max<int64_t>(n, 0)); status = own.data(); }
    if (n > 0) {
        DBuf<unsigned long long> aw;
        if (f) RC(pack_allow(v, *f, aw));
        RC(by_precision(v, [&](auto zero) -> int { return cap_run<decltype(zero)>(v, n, rows, topk, pool, group, cap, items, scores, status); }));
    }
    if (stats) pcr_cap_stats_from(std::max<int64_t>(n, 0), topk, status, items, stats);
    return PCR_OK;
}
// full-catalogue top-N evaluation of v's rows against their test ratings; the relevance tables are built on the first call for a
// (threshold, cutoffs) and kept in D
static int serve_topn(const ServeView& v, TopnDev& D, int ncut, const int* cuts, double thr, pcr_topn_stats* stats, double* per_user) {
    if (!D.same(ncut, cuts, thr)) RC(D.build(v.rows, v.tptr, v.titem, v.tval, ncut, cuts, thr));
    const int K = cuts[ncut - 1];
    RC(by_precision(v, [&](auto zero) -> int {
        using T = decltype(zero);
        return rec_run<T>(v, (int64_t)D.rel.users.size(), D.rel.users.data(), K, 1, RecTopn<T>{v, K, D});
    }));
    return D.finish(v, stats, per_user);
}
// exact rank metrics of v's rows against their test ratings; the relevance table is built on the first call for a threshold and
// kept in D
static int serve_ranks(const ServeView& v, RankDev& D, double thr, pcr_rank_stats* stats, double* per_user, int64_t* ranks) {
    if (!D.same(thr)) RC(D.build(v.rows, v.tptr, v.titem, v.tval, thr));
    RC(by_precision(v, [&](auto zero) -> int { return rank_run<decltype(zero)>(v, D); }));
    return D.finish(v, stats, per_user, ranks);
}
// The filtered evaluations (pcr_evaluate_topn_filtered, pcr_evaluate_ranks_filtered) of v's rows: the test
// rows are restricted to F_u on the host (pcr_filter_test_rows) and the relevance tables built from them, per call, in tables of
// the call's own -- a solver's cached unfiltered tables are not looked at.  An allow set alone takes the unfiltered sweeps with
// the packed set on the view; candidate rows take k_rec_cand's metrics form and k_cand_count.  The reductions are the unfiltered ones.
static int serve_topn_filtered(ServeView v, const pcr_item_filter& f, int ncut, const int* cuts, double thr, pcr_topn_stats* stats, double* per_user) {
    DBuf<unsigned long long> aw;
    RC(pack_allow(v, f, aw));
    PcrFilteredTest ft;
    pcr_filter_test_rows(v.rows, v.tptr, v.titem, v.tval, f, ft);
    TopnDev D;
    RC(D.build(v.rows, ft.ptr.data(), ft.item.data(), ft.val.data(), ncut, cuts, thr));
    const int K = cuts[ncut - 1];
    RC(by_precision(v, [&](auto zero) -> int {
        using T = decltype(zero);
        if (f.cand_ptr) return cand_topn_run<T>(v, D, K, f);
        return rec_run<T>(v, (int64_t)D.rel.users.size(), D.rel.users.data(), K, 1, RecTopn<T>{v, K, D});
    }));
    return D.finish(v, stats, per_user);
}
static int serve_ranks_filtered(ServeView v, const pcr_item_filter& f, double thr, pcr_rank_stats* stats, double* per_user, int64_t* ranks) {
    DBuf<unsigned long long> aw;
    RC(pack_allow(v, f, aw));
    PcrFilteredTest ft;
    pcr_filter_test_rows(v.rows, v.tptr, v.titem, v.tval, f, ft);
    const int64_t tnnz = v.tptr[v.rows];
    v.tptr = ft.ptr.data(); v.titem = ft.item.data(); v.tval = ft.val.data();      // (RankDev::finish scatters over the rows it was built from)
    RankDev D;
    RC(D.build(v.rows, v.tptr, v.titem, v.tval, thr));
    RC(by_precision(v, [&](auto zero) -> int {
        using T = decltype(zero);
        return f.cand_ptr ? cand_rank_run<T>(v, D, f) : rank_run<T>(v, D);
    }));
    std::vector<int64_t> fr(ranks ? ft.item.size() + 1 : 0);
    RC(D.finish(v, stats, per_user, ranks ? fr.data() : nullptr));
    if (ranks) {                                           // a rating outside F_u has rank 0
        std::fill(ranks, ranks + tnnz, (int64_t)0);
        for (size_t z = 0; z < ft.pos.size(); ++z) ranks[ft.pos[z]] = fr[z];
    }
    return PCR_OK;
}
// beyond-accuracy metrics of v's rows; the self-information table comes from the training ratings (summed across the ranks with
// a communicator) and is kept in info: the ratings never change, the exchange mode can (info_mode 0: not built, 1: from this
// shard's ratings alone, 2: all-reduced)
static int div_info_ready(const char* who, const ServeView& v, DBuf<double>& info, int& info_mode) {
    // (the peer-to-peer communicator's fp64 exchange is its 64-double scalar slot: the d2-sized tables do not fit it)
    if (v.exchange == SERVE_P2P) { pcr_set_error(std::string(who) + ": not available on a peer-to-peer communicator (use RCCL, or local-only shards and pcr_exposure_stats)"); return PCR_ERR_UNSUPPORTED; }
    const int mode = v.exchange == SERVE_LOCAL ? 1 : 2;
    if (info_mode != mode) {
        info_mode = 0;
        RC(div_info_build(v, info));
        info_mode = mode;
    }
    return PCR_OK;
}
static int serve_diversity(const ServeView& v, DBuf<double>& info, int& info_mode, int64_t n, const int32_t* rows, int ncut, const int* cuts,
                           pcr_diversity_stats* stats, double* per_user, int64_t* exposure) {
    RC(div_info_ready("pcr_evaluate_diversity", v, info, info_mode));
    return by_precision(v, [&](auto zero) -> int { return div_run<decltype(zero)>(v, info.p, n, rows, ncut, cuts, stats, per_user, exposure); });
}

// what a solver keeps between calls of the serving layer
struct ServeState {
    TopnDev topn;
    RankDev rankd;
    DBuf<double> div_info;        // info[d2] of pcr_evaluate_diversity
    int div_info_mode = 0;
};
pcr_solver::pcr_solver() : serve(new ServeState) {}
pcr_solver::~pcr_solver() {}

extern "C" {

// users[n] (global ids, NULL: the whole shard) as rows of s's shard in loc (left empty for NULL); *n the count
static int shard_rows(const char* who, const pcr_solver* s, int64_t* n, const int32_t* users, std::vector<int32_t>& loc) {
    if (!users) { *n = s->n_users; return PCR_OK; }
    loc.resize((size_t)*n);
    for (int64_t i = 0; i < *n; ++i) {
        const int64_t x = (int64_t)users[i] - s->first_user;
        if (x < 0 || x >= s->n_users) {
            pcr_set_error(std::string(who) + ": user " + std::to_string(users[i]) + " is not in this shard [" + std::to_string(s->first_user) + ", " +
                          std::to_string(s->first_user + s->n_users) + ")");
            return PCR_ERR_ARG;
        }
        loc[(size_t)i] = (int32_t)x;
    }
    return PCR_OK;
}

int pcr_evaluate_diversity(pcr_solver* s, int64_t n, const int32_t* users, int ncut, const int* cutoffs, int flags, pcr_diversity_stats* stats,
                           double* per_user, int64_t* exposure) {
    S_OR_ARG;
    RC(pcr_cutoffs_check("pcr_evaluate_diversity", ncut, cutoffs));
    if (!stats) { pcr_set_error("pcr_evaluate_diversity: null stats"); return PCR_ERR_ARG; }
    if (flags & ~PCR_REC_EXCLUDE_TRAIN) { pcr_set_error("pcr_evaluate_diversity: unknown flags"); return PCR_ERR_ARG; }
    if (users && n < 0) { pcr_set_error("pcr_evaluate_diversity: bad argument"); return PCR_ERR_ARG; }
    return abi_guard("pcr_evaluate_diversity", [&]() -> int {
        std::vector<int32_t> loc;
        RC(shard_rows("pcr_evaluate_diversity", s, &n, users, loc));
        return serve_diversity(solver_view(s, flags), s->serve->div_info, s->serve->div_info_mode, n, users ? loc.data() : nullptr, ncut, cutoffs,
                               stats, per_user, exposure);
    });
}

int pcr_evaluate_rerank(pcr_solver* s, int64_t n, const int32_t* users, int nth, const double* thetas, int pool, int ncut, const int* cutoffs,
                        double threshold, int flags, pcr_topn_stats* topn, pcr_diversity_stats* div, double* per_user_topn, double* per_user_div,
                        int64_t* exposure) {
    S_OR_ARG;
    RC(pcr_tradeoff_check("pcr_evaluate_rerank", nth, thetas, pool, ncut, cutoffs, threshold, div));
    if (flags & ~PCR_REC_EXCLUDE_TRAIN) { pcr_set_error("pcr_evaluate_rerank: unknown flags"); return PCR_ERR_ARG; }
    if (users && n < 0) { pcr_set_error("pcr_evaluate_rerank: bad argument"); return PCR_ERR_ARG; }
    if (!topn && per_user_topn) { pcr_set_error("pcr_evaluate_rerank: per_user_topn must be NULL without topn"); return PCR_ERR_ARG; }
    return abi_guard("pcr_evaluate_rerank", [&]() -> int {
        std::vector<int32_t> loc;
        RC(shard_rows("pcr_evaluate_rerank", s, &n, users, loc));
        const ServeView v = solver_view(s, flags);
        RC(div_info_ready("pcr_evaluate_rerank", v, s->serve->div_info, s->serve->div_info_mode));
        return by_precision(v, [&](auto zero) -> int {
            return tradeoff_run<decltype(zero)>("pcr_evaluate_rerank", v, s->serve->div_info.p, n, users ? loc.data() : nullptr, nth, thetas, pool,
                                                ncut, cutoffs, threshold, topn != nullptr, topn, div, per_user_topn, per_user_div, exposure);
        });
    });
}

int pcr_recommend(pcr_solver* s, int64_t n, const int32_t* users, int topk, int flags, int32_t* items, double* scores) {
    S_OR_ARG;
    if (topk < 1 || topk > PCR_RECOMMEND_MAX_K) { pcr_set_error("pcr_recommend: K = " + std::to_string(topk) + " outside [1, " + std::to_string(PCR_RECOMMEND_MAX_K) + "]"); return PCR_ERR_ARG; }
    if (flags & ~PCR_REC_EXCLUDE_TRAIN) { pcr_set_error("pcr_recommend: unknown flags"); return PCR_ERR_ARG; }
    if (!users) n = s->n_users;
    if (n < 0 || (n > 0 && (!items || !scores))) { pcr_set_error("pcr_recommend: bad argument"); return PCR_ERR_ARG; }
    return abi_guard("pcr_recommend", [&]() -> int {
        std::vector<int32_t> loc;
        RC(shard_rows("pcr_recommend", s, &n, users, loc));
        return serve_recommend(solver_view(s, flags), n, users ? loc.data() : nullptr, topk, items, scores);
    });
}

int pcr_recommend_filtered(pcr_solver* s, int64_t n, const int32_t* users, int topk, int flags, const pcr_item_filter* f, int32_t* items,
                           double* scores) {
    S_OR_ARG;
    if (topk < 1 || topk > PCR_RECOMMEND_MAX_K) { pcr_set_error("pcr_recommend_filtered: K = " + std::to_string(topk) + " outside [1, " + std::to_string(PCR_RECOMMEND_MAX_K) + "]"); return PCR_ERR_ARG; }
    if (flags & ~PCR_REC_EXCLUDE_TRAIN) { pcr_set_error("pcr_recommend_filtered: unknown flags"); return PCR_ERR_ARG; }
    if (!users) n = s->n_users;
    if (n < 0 || (n > 0 && (!items || !scores))) { pcr_set_error("pcr_recommend_filtered: bad argument"); return PCR_ERR_ARG; }
    return abi_guard("pcr_recommend_filtered", [&]() -> int {
        const ServeView v = solver_view(s, flags);
        RC(pcr_item_filter_check("pcr_recommend_filtered", v.d2, n, users, f));
        std::vector<int32_t> loc;
        RC(shard_rows("pcr_recommend_filtered", s, &n, users, loc));
        return serve_recommend_filtered(v, n, users ? loc.data() : nullptr, topk, *f, items, scores);
    });
}

int pcr_recommend_filtered_model(const double* U, int64_t d1, const double* V, int64_t d2, int64_t k, const int64_t* index, const int32_t* item,
                                 int64_t n, const int32_t* users, int topk, int dtype, const pcr_item_filter* f, int32_t* items, double* scores,
                                 int device) {
    return abi_guard("pcr_recommend_filtered_model", [&]() -> int {
    bool sorted = true;
    RC(pcr_recommend_filtered_model_check(U, d1, V, d2, k, index, item, n, users, topk, dtype, f, items, scores, &sorted));
    RC(model_device(device));
    if (n == 0) return PCR_OK;
    ServeView v;
    ModelDev M;
    RC(M.open(U, d1, V, d2, k, index, item, sorted, dtype, &v));
    return serve_recommend_filtered(v, n, users, topk, *f, items, scores);
    });
}

int pcr_recommend_diverse(pcr_solver* s, int64_t n, const int32_t* users, int topk, int pool, double theta, int flags, int32_t* items,
                          double* scores) {
    S_OR_ARG;
    RC(pcr_rerank_check("pcr_recommend_diverse", topk, pool, theta));
    if (flags & ~PCR_REC_EXCLUDE_TRAIN) { pcr_set_error("pcr_recommend_diverse: unknown flags"); return PCR_ERR_ARG; }
    if (!users) n = s->n_users;
    if (n < 0 || (n > 0 && (!items || !scores))) { pcr_set_error("pcr_recommend_diverse: bad argument"); return PCR_ERR_ARG; }
    return abi_guard("pcr_recommend_diverse", [&]() -> int {
        std::vector<int32_t> loc;
        RC(shard_rows("pcr_recommend_diverse", s, &n, users, loc));
        return serve_recommend_diverse(solver_view(s, flags), n, users ? loc.data() : nullptr, topk, pool, theta, items, scores);
    });
}

int pcr_recommend_capped(pcr_solver* s, int64_t n, const int32_t* users, int topk, int pool, const int32_t* group, int cap, int flags,
                         const pcr_item_filter* f, int32_t* items, double* scores, uint8_t* status, pcr_cap_stats* stats) {
    S_OR_ARG;
    RC(pcr_cap_check("pcr_recommend_capped", topk, pool, group, cap));
    if (flags & ~PCR_REC_EXCLUDE_TRAIN) { pcr_set_error("pcr_recommend_capped: unknown flags"); return PCR_ERR_ARG; }
    if (!users) n = s->n_users;
    if (n < 0 || (n > 0 && (!items || !scores))) { pcr_set_error("pcr_recommend_capped: bad argument"); return PCR_ERR_ARG; }
    RC(pcr_cap_filter_check("pcr_recommend_capped", f));
    return abi_guard("pcr_recommend_capped", [&]() -> int {
        std::vector<int32_t> loc;
        RC(shard_rows("pcr_recommend_capped", s, &n, users, loc));
        return serve_recommend_capped(solver_view(s, flags), n, users ? loc.data() : nullptr, topk, pool, group, cap, f, items, scores, status, stats);
    });
}

int pcr_recommend_capped_model(const double* U, int64_t d1, const double* V, int64_t d2, int64_t k, const int64_t* index, const int32_t* item,
                               int64_t n, const int32_t* users, int topk, int pool, const int32_t* group, int cap, int dtype,
                               const pcr_item_filter* f, int32_t* items, double* scores, uint8_t* status, pcr_cap_stats* stats, int device) {
    return abi_guard("pcr_recommend_capped_model", [&]() -> int {
    bool sorted = true;
    RC(pcr_recommend_capped_model_check(U, d1, V, d2, k, index, item, n, users, topk, pool, group, cap, dtype, f, items, scores, &sorted));
    RC(model_device(device));
    ServeView v; ModelDev M;
    if (n > 0) RC(M.open(U, d1, V, d2, k, index, item, sorted, dtype, &v));
    return serve_recommend_capped(v, n, users, topk, pool, group, cap, f, items, scores, status, stats);
    });
}

int pcr_evaluate_topn(pcr_solver* s, int ncut, const int* cutoffs, double threshold, int flags, pcr_topn_stats* stats, double* per_user) {
    S_OR_ARG;
    RC(pcr_topn_check("pcr_evaluate_topn", ncut, cutoffs, threshold, stats));
    if (flags & ~PCR_REC_EXCLUDE_TRAIN) { pcr_set_error("pcr_evaluate_topn: unknown flags"); return PCR_ERR_ARG; }
    return abi_guard("pcr_evaluate_topn", [&]() -> int { return serve_topn(solver_view(s, flags), s->serve->topn, ncut, cutoffs, threshold, stats, per_user); });
}

int pcr_evaluate_ranks(pcr_solver* s, double threshold, int flags, pcr_rank_stats* stats, double* per_user, int64_t* ranks) {
    S_OR_ARG;
    if (std::isnan(threshold)) { pcr_set_error("pcr_evaluate_ranks: threshold is NaN"); return PCR_ERR_ARG; }
    if (!stats) { pcr_set_error("pcr_evaluate_ranks: null stats"); return PCR_ERR_ARG; }
    if (flags & ~PCR_REC_EXCLUDE_TRAIN) { pcr_set_error("pcr_evaluate_ranks: unknown flags"); return PCR_ERR_ARG; }
    return abi_guard("pcr_evaluate_ranks", [&]() -> int { return serve_ranks(solver_view(s, flags), s->serve->rankd, threshold, stats, per_user, ranks); });
}

int pcr_evaluate_topn_filtered(pcr_solver* s, int ncut, const int* cutoffs, double threshold, int flags, const pcr_item_filter* f,
                               pcr_topn_stats* stats, double* per_user) {
    S_OR_ARG;
    RC(pcr_topn_check("pcr_evaluate_topn_filtered", ncut, cutoffs, threshold, stats));
    if (flags & ~PCR_REC_EXCLUDE_TRAIN) { pcr_set_error("pcr_evaluate_topn_filtered: unknown flags"); return PCR_ERR_ARG; }
    return abi_guard("pcr_evaluate_topn_filtered", [&]() -> int {
        const ServeView v = solver_view(s, flags);
        RC(pcr_eval_filter_check("pcr_evaluate_topn_filtered", "pcr_evaluate_topn", v.d2, v.rows, f));
        return serve_topn_filtered(v, *f, ncut, cutoffs, threshold, stats, per_user);
    });
}

int pcr_evaluate_ranks_filtered(pcr_solver* s, double threshold, int flags, const pcr_item_filter* f, pcr_rank_stats* stats, double* per_user,
                                int64_t* ranks) {
    S_OR_ARG;
    if (std::isnan(threshold)) { pcr_set_error("pcr_evaluate_ranks_filtered: threshold is NaN"); return PCR_ERR_ARG; }
    if (!stats) { pcr_set_error("pcr_evaluate_ranks_filtered: null stats"); return PCR_ERR_ARG; }
    if (flags & ~PCR_REC_EXCLUDE_TRAIN) { pcr_set_error("pcr_evaluate_ranks_filtered: unknown flags"); return PCR_ERR_ARG; }
    return abi_guard("pcr_evaluate_ranks_filtered", [&]() -> int {
        const ServeView v = solver_view(s, flags);
        RC(pcr_eval_filter_check("pcr_evaluate_ranks_filtered", "pcr_evaluate_ranks", v.d2, v.rows, f));
        return serve_ranks_filtered(v, *f, threshold, stats, per_user, ranks);
    });
}

int pcr_evaluate_topn_filtered_model(const double* U, int64_t d1, const double* V, int64_t d2, int64_t k, const int64_t* index, const int32_t* item,
                                     const int64_t* tindex, const int32_t* titem, const double* tval, int ncut, const int* cutoffs,
                                     double threshold, int dtype, const pcr_item_filter* f, pcr_topn_stats* stats, double* per_user, int device) {
    return abi_guard("pcr_evaluate_topn_filtered_model", [&]() -> int {
    bool sorted = true;
    RC(pcr_evaluate_topn_model_check(U, d1, V, d2, k, index, item, tindex, titem, tval, ncut, cutoffs, threshold, dtype, stats, &sorted,
                                     "pcr_evaluate_topn_filtered_model"));
    RC(pcr_eval_filter_check("pcr_evaluate_topn_filtered_model", "pcr_evaluate_topn_model", d2, d1, f));
    RC(model_device(device));
    ServeView v;
    v.tptr = tindex; v.titem = titem; v.tval = tval;
    ModelDev M;
    RC(M.open(U, d1, V, d2, k, index, item, sorted, dtype, &v));
    return serve_topn_filtered(v, *f, ncut, cutoffs, threshold, stats, per_user);
    });
}

int pcr_evaluate_ranks_filtered_model(const double* U, int64_t d1, const double* V, int64_t d2, int64_t k, const int64_t* index, const int32_t* item,
                                      const int64_t* tindex, const int32_t* titem, const double* tval, double threshold, int dtype,
                                      const pcr_item_filter* f, pcr_rank_stats* stats, double* per_user, int64_t* ranks, int device) {
    return abi_guard("pcr_evaluate_ranks_filtered_model", [&]() -> int {
    bool sorted = true;
    RC(pcr_evaluate_ranks_model_check(U, d1, V, d2, k, index, item, tindex, titem, tval, threshold, dtype, stats, &sorted,
                                      "pcr_evaluate_ranks_filtered_model"));
    RC(pcr_eval_filter_check("pcr_evaluate_ranks_filtered_model", "pcr_evaluate_ranks_model", d2, d1, f));
    RC(model_device(device));
    ServeView v;
    v.tptr = tindex; v.titem = titem; v.tval = tval;
    ModelDev M;
    RC(M.open(U, d1, V, d2, k, index, item, sorted, dtype, &v));
    return serve_ranks_filtered(v, *f, threshold, stats, per_user, ranks);
    });
}

int pcr_recommend_model(const double* U, int64_t d1, const double* V, int64_t d2, int64_t k, const int64_t* index, const int32_t* item,
                        int64_t n, const int32_t* users, int topk, int dtype, int32_t* items, double* scores, int device) {
    return abi_guard("pcr_recommend_model", [&]() -> int {
    bool sorted = true;
    RC(pcr_recommend_model_check(U, d1, V, d2, k, index, item, n, users, topk, dtype, items, scores, &sorted));
    RC(model_device(device));
    if (n == 0) return PCR_OK;
    ServeView v;
    v.select = pcr_tune_int("recommend_select", 1);
    ModelDev M;
    RC(M.open(U, d1, V, d2, k, index, item, sorted, dtype, &v));
    return serve_recommend(v, n, users, topk, items, scores);
    });
}

int pcr_evaluate_topn_model(const double* U, int64_t d1, const double* V, int64_t d2, int64_t k, const int64_t* index, const int32_t* item,
                            const int64_t* tindex, const int32_t* titem, const double* tval, int ncut, const int* cutoffs, double threshold,
                            int dtype, pcr_topn_stats* stats, double* per_user, int device) {
    return abi_guard("pcr_evaluate_topn_model", [&]() -> int {
    bool sorted = true;
    RC(pcr_evaluate_topn_model_check(U, d1, V, d2, k, index, item, tindex, titem, tval, ncut, cutoffs, threshold, dtype, stats, &sorted));
    RC(model_device(device));
    ServeView v;
    v.tptr = tindex; v.titem = titem; v.tval = tval;
    ModelDev M;
    RC(M.open(U, d1, V, d2, k, index, item, sorted, dtype, &v));
    TopnDev D;
    return serve_topn(v, D, ncut, cutoffs, threshold, stats, per_user);
    });
}

int pcr_evaluate_ranks_model(const double* U, int64_t d1, const double* V, int64_t d2, int64_t k, const int64_t* index, const int32_t* item,
                             const int64_t* tindex, const int32_t* titem, const double* tval, double threshold, int dtype,
                             pcr_rank_stats* stats, double* per_user, int64_t* ranks, int device) {
    return abi_guard("pcr_evaluate_ranks_model", [&]() -> int {
    bool sorted = true;
    RC(pcr_evaluate_ranks_model_check(U, d1, V, d2, k, index, item, tindex, titem, tval, threshold, dtype, stats, &sorted));
    RC(model_device(device));
    ServeView v;
    v.tptr = tindex; v.titem = titem; v.tval = tval;
    ModelDev M;
    RC(M.open(U, d1, V, d2, k, index, item, sorted, dtype, &v));
    RankDev D;
    return serve_ranks(v, D, threshold, stats, per_user, ranks);
    });
}

int pcr_evaluate_diversity_model(const double* U, int64_t d1, const double* V, int64_t d2, int64_t k, const int64_t* index, const int32_t* item,
                                 int64_t n, const int32_t* users, int ncut, const int* cutoffs, int dtype, pcr_diversity_stats* stats,
                                 double* per_user, int64_t* exposure, int device) {
    return abi_guard("pcr_evaluate_diversity_model", [&]() -> int {
    bool sorted = true;
    RC(pcr_evaluate_diversity_model_check(U, d1, V, d2, k, index, item, n, users, ncut, cutoffs, dtype, stats, &sorted));
    RC(model_device(device));
    ServeView v; ModelDev M;
    RC(M.open(U, d1, V, d2, k, index, item, sorted, dtype, &v));
    DBuf<double> info; int info_mode = 0;
    return serve_diversity(v, info, info_mode, n, users, ncut, cutoffs, stats, per_user, exposure);
    });
}

int pcr_recommend_diverse_model(const double* U, int64_t d1, const double* V, int64_t d2, int64_t k, const int64_t* index, const int32_t* item,
                                int64_t n, const int32_t* users, int topk, int pool, double theta, int dtype, int32_t* items, double* scores,
                                int device) {
    return abi_guard("pcr_recommend_diverse_model", [&]() -> int {
    bool sorted = true;
    RC(pcr_recommend_diverse_model_check(U, d1, V, d2, k, index, item, n, users, topk, pool, theta, dtype, items, scores, &sorted));
    RC(model_device(device));
    if (n == 0) return PCR_OK;
    ServeView v; ModelDev M;
    RC(M.open(U, d1, V, d2, k, index, item, sorted, dtype, &v));
    return serve_recommend_diverse(v, n, users, topk, pool, theta, items, scores);
    });
}

int pcr_evaluate_lists_model(const double* V, int64_t d2, int64_t k, int64_t d1, const int64_t* index, const int32_t* item, const int64_t* tindex,
                             const int32_t* titem, const double* tval, int64_t n, const int32_t* users, int L, const int32_t* lists, int ncut,
                             const int* cutoffs, double threshold, int dtype, pcr_topn_stats* topn, double* per_user_topn,
                             pcr_diversity_stats* div, double* per_user_div, int64_t* exposure, int device) {
    return abi_guard("pcr_evaluate_lists_model", [&]() -> int {
    RC(pcr_evaluate_lists_model_check(V, d2, k, d1, index, item, tindex, titem, tval, n, users, L, lists, ncut, cutoffs, threshold, dtype, topn,
                                      per_user_topn, div));
    RC(model_device(device));
    ServeView v;
    v.tptr = tindex; v.titem = titem; v.tval = tval;
    ModelDev M;                                            // (the training CSR counts popularity alone: its rows need no order)
    RC(M.open(nullptr, d1, V, d2, k, index, item, true, dtype, &v));
    DBuf<double> info; int info_mode = 0;
    RC(div_info_ready("pcr_evaluate_lists_model", v, info, info_mode));
    return by_precision(v, [&](auto zero) -> int {
        return lists_run<decltype(zero)>(v, info.p, n, users, L, lists, ncut, cutoffs, threshold, tindex != nullptr, topn, per_user_topn, div,
                                         per_user_div, exposure);
    });
    });
}

int pcr_evaluate_rerank_model(const double* U, int64_t d1, const double* V, int64_t d2, int64_t k, const int64_t* index, const int32_t* item,
                              const int64_t* tindex, const int32_t* titem, const double* tval, int64_t n, const int32_t* users, int nth,
                              const double* thetas, int pool, int ncut, const int* cutoffs, double threshold, int dtype, pcr_topn_stats* topn,
                              pcr_diversity_stats* div, double* per_user_topn, double* per_user_div, int64_t* exposure, int device) {
    return abi_guard("pcr_evaluate_rerank_model", [&]() -> int {
    bool sorted = true;
    RC(pcr_evaluate_rerank_model_check(U, d1, V, d2, k, index, item, tindex, titem, tval, n, users, nth, thetas, pool, ncut, cutoffs, threshold,
                                       dtype, topn, per_user_topn, div, &sorted));
    RC(model_device(device));
    ServeView v;
    v.tptr = tindex; v.titem = titem; v.tval = tval;
    ModelDev M;
    RC(M.open(U, d1, V, d2, k, index, item, sorted, dtype, &v));
    DBuf<double> info; int info_mode = 0;
    RC(div_info_ready("pcr_evaluate_rerank_model", v, info, info_mode));
    return by_precision(v, [&](auto zero) -> int {
        return tradeoff_run<decltype(zero)>("pcr_evaluate_rerank_model", v, info.p, n, users, nth, thetas, pool, ncut, cutoffs, threshold,
                                            tindex != nullptr, topn, div, per_user_topn, per_user_div, exposure);
    });
    });
}

}  // extern "C"
