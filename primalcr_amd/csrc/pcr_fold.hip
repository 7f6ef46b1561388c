// pcr_fold.hip -- the fold-in families behind the C ABI of include/primalcr.h: rows for users or items the model was not trained
// on, against the fixed other factor.  Four families, each a solver entry and a _model entry over one ServeView (pcr_dev.h):
//   pcr_fold_in          new users of a ranking model     k_foldin (pcr_foldin.h)                    "foldin/newton"
//   pcr_fold_in_ridge    squared loss                     k_ridge_direct, k_ridge_cg (pcr_ridge.h)   "foldin/ridge"
//   pcr_fold_in_nnls     squared loss, row >= 0           k_nnls_direct, k_nnls_cg (pcr_nnls.h)      "foldin/nnls"
//   pcr_fold_in_conf     squared loss, weights / implicit k_ridge_direct_conf, k_ridge_cg_conf,        "foldin/conf", "foldin/conf.gram"
//                                                         k_ridge_catgram (pcr_ridge.h)
//   pcr_fold_in_items    new items of a ranking model     k_rater_scores, k_itemfold (pcr_itemfold.h) "itemfold/scores", "itemfold/newton"
// and, on fold-in's plan and forms, the explanation of listed items by a user's own ratings:
//   pcr_explain          rows of a ranking model          k_explain (pcr_explain.h)                  "explain/contrib"
//   pcr_explain_ridge    squared-loss rows                k_explain_ridge (pcr_explain_ridge.h)      "explain/ridge"
// A run uploads its plan (pcr_host.cpp built and checked it), launches one kernel per workgroup form inside the family's profile
// slot -- workgroups stride over their range, the longest rows first -- and hands the rows, the stats and the per-row records
// back through one FoldOut.  Recommendation and its metrics are pcr_serve.hip, training is pcr_solver.hip.
// There is NO CPU compute path in this file: every [device] entry point fails with PCR_ERR_DEVICE when HIP is unusable.
#include "pcr_dev.h"
#include "pcr_foldin.h"
#include "pcr_explain.h"
#include "pcr_explain_ridge.h"
#include "pcr_itemfold.h"
#include "pcr_ridge.h"
#include "pcr_nnls.h"
#include "pcr_prims.h"

static int device_cus(int* cus) {
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    HIPCHK(hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, dev));
    *cus = std::max(*cus, 1);
    return PCR_OK;
}

// What a run hands back: the n rows in the storage type (ld values each), widened to fp64 for the caller, and the per-row
// records of `fields` doubles the kernels write
template <typename T>
struct FoldOut {
    int64_t n = 0;
    int fields = 0;
    DBuf<T> rows;
    DBuf<double> per, rowsD;
    int alloc(const ServeView& v, int64_t n_, int fields_) {
        n = n_; fields = fields_;
        RC(rows.alloc((size_t)n * v.ld)); RC(per.alloc((size_t)n * fields)); RC(rowsD.alloc((size_t)n * v.r));
        return PCR_OK;
    }
    // the rows to out [n][r], the records to stats(records) and, if asked for, to per_row [n][fields]; synchronises v.st
    template <class Stats>
    int finish(const ServeView& v, double* out, double* per_row, Stats&& stats) {
        hipLaunchKernelGGL((k_mat_out<T>), dim3((unsigned)std::min<int64_t>(1 << 16, cdiv(n * v.r, 256))), dim3(256), 0, v.st, (const T*)rows.p, rowsD.p, n, v.r, v.ld);
        HIPCHK(hipGetLastError());
        std::vector<double> hp((size_t)n * fields);
        HIPCHK(hipMemcpyAsync(out, rowsD.p, (size_t)n * v.r * sizeof(double), hipMemcpyDeviceToHost, v.st));
        HIPCHK(hipMemcpyAsync(hp.data(), per.p, hp.size() * sizeof(double), hipMemcpyDeviceToHost, v.st));
        HIPCHK(hipStreamSynchronize(v.st));
        stats(hp.data());
        if (per_row) std::copy(hp.begin(), hp.end(), per_row);
        return PCR_OK;
    }
};

// The grid of a launch over count rows: at most cap workgroups per CU (fold_wg_cap: the forms' cap by workgroup size) and as many
// as their lds bytes each leave room for
static int fold_wg_cap(int block) { return block == 64 ? 16 : block == 256 ? 4 : 1; }
static int64_t fold_grid(int64_t count, int cus, int cap, size_t lds) {
    const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(cap, PCR_LDS_CU / lds));
    return std::min<int64_t>(count, (int64_t)cus * per_cu);
}
// The scratch form (BIG) of k_foldin / k_itemfold: a slice of arr bytes, in steps of 256, per workgroup and at most FOLD_SCRATCH
// bytes in all, which bounds the grid
static const size_t FOLD_SCRATCH = (size_t)1 << 30;
static int fold_slices(size_t arr, int64_t* grid, size_t* stride, DBuf<char>& scratch) {
    *stride = (arr + 255) & ~(size_t)255;
    *grid = std::max<int64_t>(1, std::min<int64_t>(*grid, (int64_t)(FOLD_SCRATCH / *stride)));
    return scratch.alloc((size_t)*grid * *stride);
}
// kernel<<<grid, block, lds, st>>>(args...) with lds bytes of dynamic LDS allowed
template <class... P, class... A>
static int fold_launch(void (*kernel)(P...), int64_t grid, int block, size_t lds, hipStream_t st, A... args) {
    HIPCHK(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(block), lds, st, static_cast<P>(args)...);
    HIPCHK(hipGetLastError());
    return PCR_OK;
}

// Fold-in (pcr_fold_in, pcr_fold_in_model; k_foldin of pcr_foldin.h) of the plan's users against v's V: the ratings, their
// levels and the users' order go to the device, then one launch per workgroup form -- P.order is by descending length, so the
// forms are ranges of it and the longest users of each start first.  A launch's LDS is sized by its longest user.
struct FoldinParams { int solver_type; double lambda, stepsize; int cg_max; double cg_tol; int steps; };
static FoldinParams foldin_params_of(const pcr_params& p, int steps) { return {p.solver_type, p.lambda, p.stepsize, p.cg_max_iter, p.cg_tol, steps}; }
template <typename T, int BLOCK, bool BIG>
static int foldin_launch(const ServeView& v, const FoldinParams& c, const PcrFoldinPlan& P, const FoldinCsr& X, const Geo& geo, const int32_t* d_order,
                         int64_t first, int64_t count, int cus, const T* dU0, T* dOut, double* dPer, DBuf<char>& scratch) {
    if (count <= 0) return PCR_OK;
    const std::vector<int64_t>& idx = P.X.index;
    const int32_t longest = P.order[(size_t)first];
    const int cap = (int)std::max<int64_t>(1, idx[(size_t)longest + 1] - idx[(size_t)longest]);
    int rs_cap = 1;
    for (int64_t i = first; i < first + count; ++i) {
        const int32_t u = P.order[(size_t)i];
        rs_cap = std::max(rs_cap, (int)(P.lv.run_ofs[(size_t)u + 1] - P.lv.run_ofs[(size_t)u]));
    }
    const size_t li_bytes = BIG ? 8 : 4, arr = foldin_arr_bytes(cap, rs_cap, sizeof(T), li_bytes);
    const size_t lds = fold_small_bytes(geo.ld, BLOCK, sizeof(T)) + (BIG ? 0 : arr);
    if (lds > PCR_LDS_CU) {
        pcr_set_error("fold-in: rank " + std::to_string(geo.r) + " (with " + std::to_string(rs_cap - 1) + " rating levels) is too large for the kernel's LDS");
        return PCR_ERR_UNSUPPORTED;
    }
    int64_t grid = fold_grid(count, cus, fold_wg_cap(BLOCK), lds);
    size_t stride = 0;
    if (BIG) RC(fold_slices(arr, &grid, &stride, scratch));
    const int pcr1 = c.solver_type == PCR_SOLVER_PCR ? 1 : 0;
    return fold_launch(k_foldin<T, BLOCK, BIG>, grid, BLOCK, lds, v.st, X, geo, d_order + first, (int)count, dU0, dOut, serve_V<T>(v), dPer, c.lambda,
                       c.stepsize, c.cg_max, c.cg_tol, c.steps, pcr1, pcr1, cap, rs_cap, scratch.p, stride);
}

template <typename T>
static int foldin_run(const ServeView& v, const FoldinParams& c, const PcrFoldinPlan& P, const double* U0, double* U_out, pcr_foldin_stats* stats,
                      double* per_user) {
    const int64_t n = P.X.d1;
    hipStream_t st = v.st;
    Geo geo;
    geo.r = v.r; geo.ld = v.ld; geo.nchunk = v.ld / VecOf<T>::N; geo.G = std::min(64, host_pow2(geo.nchunk));
    int cus = 0;
    RC(device_cus(&cus));
    DBuf<int64_t> uptr, runofs;
    DBuf<int32_t> item, runstart, order;
    DBuf<uint16_t> lvl;
    DBuf<T> dU0;
    DBuf<char> scratch;
    FoldOut<T> out;
    RC(uptr.upload(P.X.index, st)); RC(item.upload_n(P.X.item.data(), P.X.item.size()));
    RC(lvl.upload(P.lv.level, st)); RC(runofs.upload(P.lv.run_ofs, st)); RC(runstart.upload(P.lv.run_start, st));
    RC(order.upload(P.order, st));
    RC(dU0.alloc((size_t)n * v.ld)); RC(out.alloc(v, n, PCR_FOLDIN_FIELDS));
    if (U0) RC(upload_rows<T>(st, v.r, v.ld, {{U0, n, dU0.p}}));
    else HIPCHK(hipMemsetAsync(dU0.p, 0, (size_t)n * v.ld * sizeof(T), st));
    const FoldinCsr X = {uptr.p, item.p, lvl.p, runofs.p, runstart.p};
    {
        ProfScope ps(v.prof, "foldin/newton", st);
        const int64_t nw = n - P.n_big - P.n_lds;
        RC((foldin_launch<T, 512, true>(v, c, P, X, geo, order.p, 0, P.n_big, cus, dU0.p, out.rows.p, out.per.p, scratch)));
        RC((foldin_launch<T, 256, false>(v, c, P, X, geo, order.p, P.n_big, P.n_lds, cus, dU0.p, out.rows.p, out.per.p, scratch)));
        RC((foldin_launch<T, 64, false>(v, c, P, X, geo, order.p, P.n_big + P.n_lds, nw, cus, dU0.p, out.rows.p, out.per.p, scratch)));
    }
    return out.finish(v, U_out, per_user, [&](const double* hp) { if (stats) pcr_foldin_stats_from(hp, n, stats); });
}

// Ridge fold-in (pcr_fold_in_ridge*; pcr_ridge.h) and non-negative fold-in (pcr_fold_in_nnls*; pcr_nnls.h) of the plan's users
// against v's V are one run over a family: the ratings and the users' order go to the device, then one launch per range of the
// plan -- a (form, workgroup size, tile count) class, its LDS sized by the class (nnls: form and workgroup size follow from the
// rank: one range).  The family names its kernels and their LDS, its slot and messages, the tile counts its direct kernel takes,
// and its records.
struct RidgeFamily {
    typedef pcr_ridge_stats Stats;
    static constexpr int FIELDS = PCR_RIDGE_FIELDS, CG = PCR_RIDGE_CG;
    static constexpr const char *slot = "foldin/ridge", *name = "ridge", *direct_lds = "direct forms'";
    static void stats_from(const double* hp, int64_t n, Stats* s) { pcr_ridge_stats_from(hp, n, s); }
    static size_t cg_bytes(int ld) { return ridge_cg_bytes(ld); }
    static size_t direct_bytes(int mp, int ld, int block) { return ridge_direct_bytes(mp, ld, block); }
    static bool tiles_ok(int mp, int, int block) { return mp >= 16 && mp <= (block == 64 ? 64 : PCR_RIDGE_DIRECT_MAX); }
    template <typename T, class... A>
    int cg(int64_t grid, size_t lds, hipStream_t st, A... args) const { return fold_launch(k_ridge_cg<T>, grid, 256, lds, st, args...); }
    template <typename T, int BLOCK, class... A>
    int direct(int64_t grid, size_t lds, hipStream_t st, int form, int mp, A... args) const {
        return fold_launch(k_ridge_direct<T, BLOCK>, grid, BLOCK, lds, st, args..., form == PCR_RIDGE_DUAL ? 1 : 0, mp);
    }
};
// pcr_fold_in_conf*: the plain family under the conf entries' slot (no weights, alpha == 0: the ridge kernels themselves), and the
// weighted / implicit instantiations with what they read besides (cf: device pointers of the run)
struct ConfPlainFamily : RidgeFamily {
    static constexpr const char *slot = "foldin/conf", *name = "conf";
};
struct ConfFamily : RidgeFamily {
    static constexpr const char *slot = "foldin/conf", *name = "conf";
    RidgeConf cf;
    static size_t direct_bytes(int mp, int ld, int block) { return ridge_direct_conf_bytes(mp, ld, block); }
    template <typename T, class... A>
    int cg(int64_t grid, size_t lds, hipStream_t st, A... args) const { return fold_launch(k_ridge_cg_conf<T>, grid, 256, lds, st, args..., cf); }
    template <typename T, int BLOCK, class... A>
    int direct(int64_t grid, size_t lds, hipStream_t st, int form, int mp, A... args) const {
        return fold_launch(k_ridge_direct_conf<T, BLOCK>, grid, BLOCK, lds, st, args..., form == PCR_RIDGE_DUAL ? 1 : 0, mp, cf);
    }
};
struct NnlsFamily {
    typedef pcr_nnls_stats Stats;
    static constexpr int FIELDS = PCR_NNLS_FIELDS, CG = PCR_NNLS_CG;
    static constexpr const char *slot = "foldin/nnls", *name = "nnls", *direct_lds = "direct form's";
    static void stats_from(const double* hp, int64_t n, Stats* s) { pcr_nnls_stats_from(hp, n, s); }
    static size_t cg_bytes(int ld) { return nnls_cg_bytes(ld); }
    static size_t direct_bytes(int mp, int ld, int block) { return nnls_direct_bytes(mp, ld, block); }
    static bool tiles_ok(int mp, int r, int block) { return mp >= 16 && mp >= r && mp <= (block == 64 ? 64 : PCR_RIDGE_DIRECT_MAX); }
    template <typename T, class... A>
    int cg(int64_t grid, size_t lds, hipStream_t st, A... args) const { return fold_launch(k_nnls_cg<T>, grid, 256, lds, st, args...); }
    template <typename T, int BLOCK, class... A>
    int direct(int64_t grid, size_t lds, hipStream_t st, int, int mp, A... args) const {
        return fold_launch(k_nnls_direct<T, BLOCK>, grid, BLOCK, lds, st, args..., mp);
    }
};
// prepare(fam, st) (conf: the weights, W and the catalogue Gram to the device) runs before the family's slot opens.
template <class Fam, typename T, class Prep>
static int ridge_run(const ServeView& v, double lambda, int weighted, const PcrRidgePlan& P, double* U_out, typename Fam::Stats* stats, double* per_user,
                     Prep&& prepare) {
    const int64_t n = P.X.d1;
    hipStream_t st = v.st;
    int cus = 0;
    RC(device_cus(&cus));
    Fam fam;
    RC(prepare(fam, st));
    DBuf<int64_t> uptr;
    DBuf<int32_t> item, order;
    DBuf<double> val;
    FoldOut<T> out;
    RC(uptr.upload(P.X.index, st)); RC(item.upload_n(P.X.item.data(), P.X.item.size())); RC(val.upload_n(P.X.val.data(), P.X.val.size()));
    RC(order.upload(P.order, st));
    RC(out.alloc(v, n, Fam::FIELDS));
    const RidgeCsr X = {uptr.p, item.p, val.p};
    const T* F = serve_V<T>(v);
    const std::string who = std::string(Fam::name) + " fold-in: ";
    {
        ProfScope ps(v.prof, Fam::slot, st);
        for (const PcrRidgePlan::Range& g : P.ranges) {
            if (g.count <= 0) continue;
            const int32_t* users = order.p + g.first;
            if (g.form == Fam::CG) {
                const size_t lds = Fam::cg_bytes(v.ld);
                if (lds > PCR_LDS_CU) { pcr_set_error(who + "rank " + std::to_string(v.r) + " is too large for the CG form's LDS"); return PCR_ERR_UNSUPPORTED; }
                RC((fam.template cg<T>(fold_grid(g.count, cus, 8, lds), lds, st, X, users, (int)g.count, F, v.r, v.ld, out.rows.p, out.per.p, lambda,
                                       weighted)));
                continue;
            }
            const int mp = g.tiles * 16;
            if (!Fam::tiles_ok(mp, v.r, g.block)) { pcr_set_error(who + "a launch class outside the kernel's tile range"); return PCR_ERR_STATE; }
            const size_t lds = Fam::direct_bytes(mp, v.ld, g.block);
            if (lds > PCR_LDS_CU) {
                pcr_set_error(who + "rank " + std::to_string(v.r) + " is too large for the " + Fam::direct_lds + " LDS");
                return PCR_ERR_UNSUPPORTED;
            }
            const int64_t grid = fold_grid(g.count, cus, fold_wg_cap(g.block), lds);
            if (g.block == 64) RC((fam.template direct<T, 64>(grid, lds, st, g.form, mp, X, users, (int)g.count, F, v.r, v.ld, out.rows.p, out.per.p, lambda, weighted)));
            else RC((fam.template direct<T, 256>(grid, lds, st, g.form, mp, X, users, (int)g.count, F, v.r, v.ld, out.rows.p, out.per.p, lambda, weighted)));
        }
    }
    return out.finish(v, U_out, per_user, [&](const double* hp) { if (stats) Fam::stats_from(hp, n, stats); });
}
template <class Fam, typename T>
static int ridge_run(const ServeView& v, double lambda, int weighted, const PcrRidgePlan& P, double* U_out, typename Fam::Stats* stats, double* per_user) {
    return ridge_run<Fam, T>(v, lambda, weighted, P, U_out, stats, per_user, [](Fam&, hipStream_t) { return PCR_OK; });
}

// Confidence-weighted / implicit fold-in (pcr_fold_in_conf*) of the plan's users against v's V.  Without
// weights and alpha it IS the ridge run.  Else the weights and the per-user W go to the device and, for alpha > 0, the catalogue
// Gram G = F^T F is built once ("foldin/conf.gram": k_ridge_catgram's partials per row block, then their sum in block order);
// the ridge run then launches the family's weighted / implicit instantiations.
template <typename T>
static int conf_run(const ServeView& v, double lambda, int weighted, const PcrConfPlan& P, double* U_out, pcr_ridge_stats* stats, double* per_user) {
    if (P.plain) return ridge_run<ConfPlainFamily, T>(v, lambda, weighted, P, U_out, stats, per_user);
    DBuf<double> wt, W, G, part;
    return ridge_run<ConfFamily, T>(v, lambda, weighted, P, U_out, stats, per_user, [&](ConfFamily& fam, hipStream_t st) -> int {
        RC(wt.upload(P.wt, st)); RC(W.upload(P.W, st));
        fam.cf.wt = wt.p; fam.cf.W = W.p; fam.cf.alpha = P.alpha;
        if (P.alpha > 0.0) {
            const int ldg = (v.r + 15) / 16 * 16, nb = ridge_catgram_blocks(v.d2, v.r), np = ridge_catgram_pairs(v.r);
            RC(G.alloc((size_t)ldg * ldg)); RC(part.alloc((size_t)nb * np * 16 * 256));
            ProfScope ps(v.prof, "foldin/conf.gram", st);
            hipLaunchKernelGGL((k_ridge_catgram<T>), dim3((unsigned)nb, (unsigned)np), dim3(256), 0, st, serve_V<T>(v), v.d2, v.r, v.ld, nb, part.p);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(k_ridge_catgram_sum, dim3((unsigned)np, 16), dim3(256), 0, st, (const double*)part.p, nb, v.r, ldg, G.p);
            HIPCHK(hipGetLastError());
            fam.cf.G = G.p; fam.cf.ldg = ldg;
        }
        return PCR_OK;
    });
}

// Item fold-in (pcr_fold_in_items, pcr_fold_in_items_model; pcr_itemfold.h) of the plan's items against v's U: the slots and
// their pairs go to the device once; the slots are then cut into batches whose unique raters' table (scores + levels) stays within
// the cap -- a batch holds at least one slot -- and each batch uploads its raters' rows and levels, builds the score table
// ("itemfold/scores": one launch per rater form, the longest raters first) and runs its slots ("itemfold/newton": one launch per
// workgroup form).
static const size_t ITEMFOLD_TABLE = (size_t)1 << 30;
struct ItemfoldDev { RaterTab R; ItemfoldCsr X; Geo geo; int cus; };
template <typename T, int BLOCK, bool BIG>
static int itemfold_launch(const ServeView& v, const FoldinParams& c, const PcrItemfoldPlan& P, const ItemfoldDev& D, int64_t first, int64_t end,
                           const T* dV0, T* dOut, const T* tab, double* dPer, DBuf<char>& scratch) {
    const int64_t count = end - first;
    if (count <= 0) return PCR_OK;
    const int cap = (int)std::max<int64_t>(1, P.sptr[(size_t)first + 1] - P.sptr[(size_t)first]);      // slots are by descending count
    const size_t arr = itemfold_arr_bytes(cap, sizeof(T));
    const size_t lds = fold_small_bytes(D.geo.ld, BLOCK, sizeof(T)) + (BIG ? 0 : arr);
    // the refusal is a function of the rank and the item's form alone, never of the items that share its launch: the form's
    // largest item must fit
    const int form_cap = BLOCK == 64 ? PCR_ITEMFOLD_WAVE_MAX : PCR_ITEMFOLD_LDS_MAX;
    if (fold_small_bytes(D.geo.ld, BLOCK, sizeof(T)) + (BIG ? 0 : itemfold_arr_bytes(form_cap, sizeof(T))) > PCR_LDS_CU) {
        pcr_set_error("item fold-in: rank " + std::to_string(D.geo.r) + " is too large for the LDS of the workgroup form of items " +
                      (BIG ? "beyond " + std::to_string(PCR_ITEMFOLD_LDS_MAX) : "of up to " + std::to_string(form_cap)) + " raters");
        return PCR_ERR_UNSUPPORTED;
    }
    if (BIG && ((arr + 255) & ~(size_t)255) > FOLD_SCRATCH) {
        pcr_set_error("item fold-in: an item of " + std::to_string(cap) + " raters needs more than 1 GiB of per-rater scratch");
        return PCR_ERR_UNSUPPORTED;
    }
    int64_t grid = fold_grid(count, D.cus, fold_wg_cap(BLOCK), lds);
    size_t stride = 0;
    if (BIG) RC(fold_slices(arr, &grid, &stride, scratch));
    return fold_launch(k_itemfold<T, BLOCK, BIG>, grid, BLOCK, lds, v.st, D.R, D.X, D.geo, (int)first, (int)count, dV0, dOut, serve_U<T>(v), tab, dPer,
                       c.lambda, c.stepsize, c.cg_max, c.cg_tol, c.steps, c.solver_type == PCR_SOLVER_PCR ? 1 : 0, cap, scratch.p, stride);
}

template <typename T, int BLOCK>
static int rater_scores_launch(const ServeView& v, const ItemfoldDev& D, const int32_t* d_order, int64_t count, T* tab) {
    if (count <= 0) return PCR_OK;
    const int64_t grid = std::min<int64_t>(count, (int64_t)D.cus * (BLOCK == 64 ? 32 : 8));
    hipLaunchKernelGGL((k_rater_scores<T, BLOCK>), dim3((unsigned)grid), dim3(BLOCK), carve_bytes(D.geo.ld, sizeof(T)), v.st, D.R, D.geo, d_order,
                       (int)count, serve_U<T>(v), serve_V<T>(v), tab);
    HIPCHK(hipGetLastError());
    return PCR_OK;
}

template <typename T>
static int itemfold_run(const ServeView& v, const FoldinParams& c, const PcrItemfoldPlan& P, const double* V0, double* V_out, pcr_itemfold_stats* stats,
                        double* per_item) {
    const int64_t n = P.n, nr = (int64_t)P.raters.size();
    hipStream_t st = v.st;
    ItemfoldDev D;
    D.geo.r = v.r; D.geo.ld = v.ld; D.geo.nchunk = v.ld / VecOf<T>::N; D.geo.G = std::min(64, host_pow2(D.geo.nchunk));
    RC(device_cus(&D.cus));
    size_t table_cap = ITEMFOLD_TABLE;
    { std::string knob; if (pcr_tune_get("itemfold_table_bytes", &knob) && atoll(knob.c_str()) > 0) table_cap = (size_t)atoll(knob.c_str()); }
    DBuf<int64_t> sptr;
    DBuf<int32_t> orig, anypair, puser, pq;
    DBuf<T> dV0;
    FoldOut<T> out;
    RC(sptr.upload(P.sptr, st)); RC(orig.upload(P.order, st)); RC(anypair.upload(P.anypair, st)); RC(puser.upload(P.puser, st)); RC(pq.upload(P.pq, st));
    RC(dV0.alloc((size_t)n * v.ld)); RC(out.alloc(v, n, PCR_ITEMFOLD_FIELDS));
    if (V0) RC(upload_rows<T>(st, v.r, v.ld, {{V0, n, dV0.p}}));
    else HIPCHK(hipMemsetAsync(dV0.p, 0, (size_t)n * v.ld * sizeof(T), st));
    std::vector<int32_t> local((size_t)nr, -1), braters, ploc, ruser, rorder;
    std::vector<int64_t> rptr;
    std::vector<int32_t> ritem;
    std::vector<uint16_t> rlvl;
    auto rlen = [&](int32_t r) { return P.R.index[(size_t)r + 1] - P.R.index[(size_t)r]; };
    for (int64_t b0 = 0; b0 < n;) {
        // the batch [b0, b1): slots are added while the table of their unique raters stays within the cap
        for (int32_t r : braters) local[(size_t)r] = -1;
        braters.clear();
        size_t bytes = 0;
        int64_t b1 = b0;
        for (; b1 < n; ++b1) {
            const size_t mark = braters.size();
            size_t add = 0;
            for (int64_t z = P.sptr[(size_t)b1]; z < P.sptr[(size_t)b1 + 1]; ++z) {
                const int32_t r = P.prater[(size_t)z];
                if (local[(size_t)r] < 0) { local[(size_t)r] = (int32_t)braters.size(); braters.push_back(r); add += (size_t)rlen(r) * (sizeof(T) + 2); }
            }
            if (b1 > b0 && bytes + add > table_cap) {
                for (size_t q = mark; q < braters.size(); ++q) local[(size_t)braters[q]] = -1;
                braters.resize(mark);
                break;
            }
            bytes += add;
        }
        const int64_t nb = (int64_t)braters.size(), pair0 = P.sptr[(size_t)b0], pair1 = P.sptr[(size_t)b1];
        rptr.assign((size_t)nb + 1, 0); ruser.resize((size_t)nb); rorder.resize((size_t)nb);
        for (int64_t i = 0; i < nb; ++i) {
            rptr[(size_t)i + 1] = rptr[(size_t)i] + rlen(braters[(size_t)i]);
            ruser[(size_t)i] = P.raters[(size_t)braters[(size_t)i]];
            rorder[(size_t)i] = (int32_t)i;
        }
        const int64_t flat = rptr[(size_t)nb];
        ritem.resize((size_t)flat); rlvl.resize((size_t)flat);
        for (int64_t i = 0; i < nb; ++i) {
            const int64_t a = P.R.index[(size_t)braters[(size_t)i]], len = rlen(braters[(size_t)i]);
            std::copy(P.R.item.begin() + a, P.R.item.begin() + a + len, ritem.begin() + rptr[(size_t)i]);
            std::copy(P.lv.level.begin() + a, P.lv.level.begin() + a + len, rlvl.begin() + rptr[(size_t)i]);
        }
        // raters by descending length (equal lengths in batch order): the wave form is the tail
        std::stable_sort(rorder.begin(), rorder.end(), [&](int32_t x, int32_t y) { return rptr[(size_t)x + 1] - rptr[(size_t)x] > rptr[(size_t)y + 1] - rptr[(size_t)y]; });
        int64_t n_wg = 0;
        while (n_wg < nb && rptr[(size_t)rorder[(size_t)n_wg] + 1] - rptr[(size_t)rorder[(size_t)n_wg]] > PCR_ITEMFOLD_SCORES_WAVE_MAX) ++n_wg;
        ploc.resize((size_t)(pair1 - pair0));
        for (int64_t z = pair0; z < pair1; ++z) ploc[(size_t)(z - pair0)] = local[(size_t)P.prater[(size_t)z]];
        DBuf<int64_t> d_rptr;
        DBuf<int32_t> d_ruser, d_ritem, d_rorder, d_ploc;
        DBuf<uint16_t> d_rlvl;
        DBuf<T> tab;
        DBuf<char> scratch;
        RC(d_rptr.upload(rptr, st)); RC(d_ruser.upload(ruser, st)); RC(d_ritem.upload(ritem, st)); RC(d_rlvl.upload(rlvl, st));
        RC(d_rorder.upload(rorder, st)); RC(d_ploc.upload(ploc, st)); RC(tab.alloc((size_t)flat));
        D.R = {d_rptr.p, d_ruser.p, d_ritem.p, d_rlvl.p};
        D.X = {sptr.p, orig.p, anypair.p, puser.p, pq.p, d_ploc.p, pair0};
        {
            ProfScope ps(v.prof, "itemfold/scores", st);
            RC((rater_scores_launch<T, 256>(v, D, d_rorder.p, n_wg, tab.p)));
            RC((rater_scores_launch<T, 64>(v, D, d_rorder.p + n_wg, nb - n_wg, tab.p)));
        }
        {
            ProfScope ps(v.prof, "itemfold/newton", st);
            const int64_t e_big = std::min(b1, P.n_big), e_lds = std::min(b1, P.n_big + P.n_lds);
            RC((itemfold_launch<T, 512, true>(v, c, P, D, b0, e_big, dV0.p, out.rows.p, tab.p, out.per.p, scratch)));
            RC((itemfold_launch<T, 256, false>(v, c, P, D, std::max(b0, P.n_big), e_lds, dV0.p, out.rows.p, tab.p, out.per.p, scratch)));
            RC((itemfold_launch<T, 64, false>(v, c, P, D, std::max(b0, P.n_big + P.n_lds), b1, dV0.p, out.rows.p, tab.p, out.per.p, scratch)));
        }
        HIPCHK(hipStreamSynchronize(st));        // the batch's buffers go out of scope
        b0 = b1;
    }
    return out.finish(v, V_out, per_item, [&](const double* hp) { if (stats) { stats->unique_raters = nr; pcr_itemfold_stats_from(hp, n, stats); } });
}

// Explanations (pcr_explain, pcr_explain_model; k_explain of pcr_explain.h) of the plan's users: Um holds their rows of U (row
// urow[i] is user i's; NULL: row i), lam their regularisers lambda / c_u.  The ratings, levels and order go to the device as
// fold-in's, then one launch per workgroup form.  A launch's LDS is sized by its longest user; the refusal by the form's largest.
struct ExplainOut { int32_t* item; double* contrib; double* per_pair; double* per_user; pcr_explain_stats* stats; };
template <typename T, int BLOCK, bool BIG>
static int explain_launch(const ServeView& v, int strict, const PcrFoldinPlan& P, const FoldinCsr& X, const Geo& geo, const int32_t* d_order, int64_t first,
                          int64_t count, int cus, const T* Um, const int32_t* urow, const double* lam, const int32_t* lists, int L, int E,
                          int32_t* d_item, double* d_contrib, double* d_pair, double* d_user, DBuf<char>& scratch) {
    if (count <= 0) return PCR_OK;
    const std::vector<int64_t>& idx = P.X.index;
    const int32_t longest = P.order[(size_t)first];
    const int cap = (int)std::max<int64_t>(1, idx[(size_t)longest + 1] - idx[(size_t)longest]);
    int rs_cap = 1;
    for (int64_t i = first; i < first + count; ++i) {
        const int32_t u = P.order[(size_t)i];
        rs_cap = std::max(rs_cap, (int)(P.lv.run_ofs[(size_t)u + 1] - P.lv.run_ofs[(size_t)u]));
    }
    const size_t li_bytes = BIG ? 8 : 4, arr = explain_arr_bytes(cap, rs_cap, sizeof(T), li_bytes);
    const int erows = std::min(cap, EXPLAIN_CHUNK);
    const size_t lds = explain_small_bytes(geo.ld, BLOCK, sizeof(T), erows) + (BIG ? 0 : arr);
    // the refusal is a function of the rank and the user's form alone: the form's largest user (a level per rating) must fit
    const int form_cap = BLOCK == 64 ? PCR_FOLDIN_WAVE_MAX : PCR_FOLDIN_LDS_MAX;
    if (explain_small_bytes(geo.ld, BLOCK, sizeof(T), std::min(form_cap, EXPLAIN_CHUNK)) + (BIG ? 0 : explain_arr_bytes(form_cap, form_cap + 1, sizeof(T), li_bytes)) >
        PCR_LDS_CU) {
        pcr_set_error("explain: rank " + std::to_string(geo.r) + " is too large for the LDS of the workgroup form of users " +
                      (BIG ? "beyond " + std::to_string(PCR_FOLDIN_LDS_MAX) : "of up to " + std::to_string(form_cap)) + " ratings");
        return PCR_ERR_UNSUPPORTED;
    }
    if (BIG && ((arr + 255) & ~(size_t)255) > FOLD_SCRATCH) {
        pcr_set_error("explain: a user of " + std::to_string(cap) + " ratings needs more than 1 GiB of per-rating scratch");
        return PCR_ERR_UNSUPPORTED;
    }
    int64_t grid = fold_grid(count, cus, fold_wg_cap(BLOCK), lds);
    size_t stride = 0;
    if (BIG) RC(fold_slices(arr, &grid, &stride, scratch));
    return fold_launch(k_explain<T, BLOCK, BIG>, grid, BLOCK, lds, v.st, X, geo, d_order + first, (int)count, Um, urow, serve_V<T>(v), lam, lists, L, E,
                       d_item, d_contrib, d_pair, d_user, strict, cap, rs_cap, erows, scratch.p, stride);
}

template <typename T>
static int explain_run(const ServeView& v, int solver_type, double lambda, const PcrFoldinPlan& P, const T* Um, const int32_t* urow_host,
                       const double* weights, int L, const int32_t* lists, int E, const ExplainOut& o) {
    const int64_t n = P.X.d1;
    hipStream_t st = v.st;
    Geo geo;
    geo.r = v.r; geo.ld = v.ld; geo.nchunk = v.ld / VecOf<T>::N; geo.G = std::min(64, host_pow2(geo.nchunk));
    int cus = 0;
    RC(device_cus(&cus));
    std::vector<double> lam((size_t)n);
    for (int64_t i = 0; i < n; ++i) lam[(size_t)i] = weights ? lambda / weights[i] : lambda;
    DBuf<int64_t> uptr, runofs;
    DBuf<int32_t> item, runstart, order, urow, dlists, d_item;
    DBuf<uint16_t> lvl;
    DBuf<double> dlam, d_contrib, d_pair, d_user;
    DBuf<char> scratch;
    const size_t pairs = (size_t)n * L;
    RC(uptr.upload(P.X.index, st)); RC(item.upload_n(P.X.item.data(), P.X.item.size()));
    RC(lvl.upload(P.lv.level, st)); RC(runofs.upload(P.lv.run_ofs, st)); RC(runstart.upload(P.lv.run_start, st));
    RC(order.upload(P.order, st)); RC(dlam.upload(lam, st)); RC(dlists.upload_n(lists, pairs));
    if (urow_host) RC(urow.upload_n(urow_host, (size_t)n));
    RC(d_item.alloc(pairs * E)); RC(d_contrib.alloc(pairs * E)); RC(d_pair.alloc(pairs * PCR_EXPLAIN_PAIR_FIELDS));
    RC(d_user.alloc((size_t)n * PCR_EXPLAIN_USER_FIELDS));
    const FoldinCsr X = {uptr.p, item.p, lvl.p, runofs.p, runstart.p};
    const int strict = solver_type == PCR_SOLVER_PCR ? 1 : 0;
    {
        ProfScope ps(v.prof, "explain/contrib", st);
        const int64_t nw = n - P.n_big - P.n_lds;
        RC((explain_launch<T, 512, true>(v, strict, P, X, geo, order.p, 0, P.n_big, cus, Um, urow_host ? urow.p : nullptr, dlam.p, dlists.p, L, E,
                                         d_item.p, d_contrib.p, d_pair.p, d_user.p, scratch)));
        RC((explain_launch<T, 256, false>(v, strict, P, X, geo, order.p, P.n_big, P.n_lds, cus, Um, urow_host ? urow.p : nullptr, dlam.p, dlists.p, L, E,
                                          d_item.p, d_contrib.p, d_pair.p, d_user.p, scratch)));
        RC((explain_launch<T, 64, false>(v, strict, P, X, geo, order.p, P.n_big + P.n_lds, nw, cus, Um, urow_host ? urow.p : nullptr, dlam.p, dlists.p, L, E,
                                         d_item.p, d_contrib.p, d_pair.p, d_user.p, scratch)));
    }
    std::vector<double> hpair;
    double* pair_out = o.per_pair;
    if (!pair_out && o.stats) { hpair.resize(pairs * PCR_EXPLAIN_PAIR_FIELDS); pair_out = hpair.data(); }
    HIPCHK(hipMemcpyAsync(o.item, d_item.p, pairs * E * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(o.contrib, d_contrib.p, pairs * E * sizeof(double), hipMemcpyDeviceToHost, st));
    if (pair_out) HIPCHK(hipMemcpyAsync(pair_out, d_pair.p, pairs * PCR_EXPLAIN_PAIR_FIELDS * sizeof(double), hipMemcpyDeviceToHost, st));
    if (o.per_user) HIPCHK(hipMemcpyAsync(o.per_user, d_user.p, (size_t)n * PCR_EXPLAIN_USER_FIELDS * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (o.stats) pcr_explain_stats_from(pair_out, o.item, lists, n, L, E, o.stats);
    return PCR_OK;
}

// Explanations of squared-loss rows (pcr_explain_ridge, pcr_explain_ridge_model; k_explain_ridge of pcr_explain_ridge.h) of the
// plan's users against v's V: Um holds their rows of U (row urow[i] is user i's; NULL: row i) or is NULL (the minimiser itself is
// explained).  The ratings and the order go to the device as ridge fold-in's, then ONE launch: the plan has one range, its LDS
// sized by the rank and the longest user's chunk.
struct ExplainRidgeOut { int32_t* item; double* contrib; double* per_pair; double* per_user; pcr_explain_ridge_stats* stats; };
template <typename T>
static int explain_ridge_run(const ServeView& v, double lambda, int weighted, int nonneg, const PcrRidgePlan& P, const T* Um, const int32_t* urow_host,
                             int L, const int32_t* lists, int E, const ExplainRidgeOut& o) {
    const int64_t n = P.X.d1;
    hipStream_t st = v.st;
    Geo geo;
    geo.r = v.r; geo.ld = v.ld; geo.nchunk = v.ld / VecOf<T>::N; geo.G = std::min(64, host_pow2(geo.nchunk));
    int cus = 0;
    RC(device_cus(&cus));
    const PcrRidgePlan::Range& g = P.ranges.at(0);
    const int mp = g.tiles * 16;
    if (g.block != 256 || mp < v.r || mp < 16 || mp > PCR_RIDGE_DIRECT_MAX || g.first != 0 || g.count != n) {
        pcr_set_error("explain (ridge): a launch class outside the kernel's tile range");
        return PCR_ERR_STATE;
    }
    const int32_t longest = P.order[0];
    const int erows = (int)std::max<int64_t>(1, std::min<int64_t>(P.X.index[(size_t)longest + 1] - P.X.index[(size_t)longest], EXPLAIN_CHUNK));
    const size_t lds = explain_ridge_bytes(mp, 256, erows);
    if (lds > PCR_LDS_CU) { pcr_set_error("explain (ridge): rank " + std::to_string(v.r) + " is too large for the kernel's LDS"); return PCR_ERR_UNSUPPORTED; }
    DBuf<int64_t> uptr;
    DBuf<int32_t> item, order, urow, dlists, d_item;
    DBuf<double> val, d_contrib, d_pair, d_user;
    const size_t pairs = (size_t)n * L;
    RC(uptr.upload(P.X.index, st)); RC(item.upload_n(P.X.item.data(), P.X.item.size())); RC(val.upload_n(P.X.val.data(), P.X.val.size()));
    RC(order.upload(P.order, st)); RC(dlists.upload_n(lists, pairs));
    if (urow_host) RC(urow.upload_n(urow_host, (size_t)n));
    RC(d_item.alloc(pairs * E)); RC(d_contrib.alloc(pairs * E)); RC(d_pair.alloc(pairs * PCR_EXPLAIN_PAIR_FIELDS));
    RC(d_user.alloc((size_t)n * PCR_EXPLAIN_RIDGE_USER_FIELDS));
    const RidgeCsr X = {uptr.p, item.p, val.p};
    {
        ProfScope ps(v.prof, "explain/ridge", st);
        RC(fold_launch(k_explain_ridge<T, 256>, fold_grid(n, cus, fold_wg_cap(256), lds), 256, lds, st, X, geo, order.p, (int)n, serve_V<T>(v), Um,
                       urow_host ? urow.p : nullptr, lambda, weighted, nonneg, mp, dlists.p, L, E, d_item.p, d_contrib.p, d_pair.p, d_user.p, erows));
    }
    std::vector<double> hpair, huser;
    double *pair_out = o.per_pair, *user_out = o.per_user;
    if (!pair_out && o.stats) { hpair.resize(pairs * PCR_EXPLAIN_PAIR_FIELDS); pair_out = hpair.data(); }
    if (!user_out && o.stats) { huser.resize((size_t)n * PCR_EXPLAIN_RIDGE_USER_FIELDS); user_out = huser.data(); }
    HIPCHK(hipMemcpyAsync(o.item, d_item.p, pairs * E * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(o.contrib, d_contrib.p, pairs * E * sizeof(double), hipMemcpyDeviceToHost, st));
    if (pair_out) HIPCHK(hipMemcpyAsync(pair_out, d_pair.p, pairs * PCR_EXPLAIN_PAIR_FIELDS * sizeof(double), hipMemcpyDeviceToHost, st));
    if (user_out) HIPCHK(hipMemcpyAsync(user_out, d_user.p, (size_t)n * PCR_EXPLAIN_RIDGE_USER_FIELDS * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (o.stats) pcr_explain_ridge_stats_from(pair_out, user_out, o.item, lists, n, L, E, o.stats);
    return PCR_OK;
}

// The entries' common end: the stats zeroed, nothing more for n == 0, then open() -- a _model entry's upload, nothing on a
// solver -- and run(T()) in the view's precision
template <class Stats, class Open, class Run>
static int fold_serve(Stats* stats, int64_t n, const ServeView& v, Open&& open, Run&& run) {
    if (stats) *stats = Stats{};
    if (n == 0) return PCR_OK;
    RC(open());
    return by_precision(v, run);
}
static int on_solver() { return PCR_OK; }

// What a solver entry that explains its own users (pcr_explain, pcr_explain_ridge) reads of the data set the solver was created
// from: every user must be on the rank (PCR_ERR_STATE otherwise), train is checked by its dimensions and nnz, users[n] are global
// ids (NULL: all of them in order; *n is then the solver's user count).  R: the requested users' rows and their rows of the device U.
struct SolverRows {
    std::vector<int64_t> index;
    std::vector<int32_t> item, urow;
    std::vector<double> val;
};
static int solver_rows(const char* who_, pcr_solver* s, const ServeView& v, const pcr_dataset* train, int64_t* n_, const int32_t* users, SolverRows* R) {
    const std::string who(who_);
    if (s->comm_nranks() > 1 || s->first_user != 0 || s->n_users != v.d1) {
        pcr_set_error(who + ": needs every user on the rank; this solver holds a shard");
        return PCR_ERR_STATE;
    }
    if (!train) { pcr_set_error(who + ": null training data set"); return PCR_ERR_ARG; }
    const PcrCsr& X = train->train;
    if (X.d1 != v.d1 || X.d2 != v.d2 || X.nnz() != v.nnz) {
        pcr_set_error(who + ": the data set is not the one the solver was created from (dimensions or nnz differ)");
        return PCR_ERR_ARG;
    }
    if (!users) *n_ = s->n_users;                                  // (n is ignored without users)
    const int64_t n = *n_;
    if (n < 0 || n >= ((int64_t)1 << 31) - 64) { pcr_set_error(who + ": bad argument"); return PCR_ERR_ARG; }
    R->index.assign((size_t)n + 1, 0);
    R->urow.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t u = users ? users[i] : i;
        if (u < 0 || u >= X.d1) { pcr_set_error(who + ": user id " + std::to_string(u) + " is outside the solver's users"); return PCR_ERR_ARG; }
        R->urow[(size_t)i] = (int32_t)u;
        R->index[(size_t)i + 1] = R->index[(size_t)i] + (X.index[(size_t)u + 1] - X.index[(size_t)u]);
    }
    R->item.resize((size_t)R->index[(size_t)n]);
    R->val.resize((size_t)R->index[(size_t)n]);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t a = X.index[(size_t)R->urow[(size_t)i]], len = R->index[(size_t)i + 1] - R->index[(size_t)i];
        std::copy(X.item.begin() + a, X.item.begin() + a + len, R->item.begin() + R->index[(size_t)i]);
        std::copy(X.val.begin() + a, X.val.begin() + a + len, R->val.begin() + R->index[(size_t)i]);
    }
    return PCR_OK;
}

extern "C" {

int pcr_fold_in_model(const pcr_params* p, const double* V, int64_t d2, int64_t n, const int64_t* index, const int32_t* item, const double* val,
                      const double* U0, int steps, double* U_out, pcr_foldin_stats* stats, double* per_user) {
    return abi_guard("pcr_fold_in_model", [&]() -> int {
    PcrFoldinPlan P;
    RC(pcr_fold_in_model_check(p, V, d2, n, index, item, val, steps, U_out, &P));
    RC(model_device(p->device));
    ServeView v; ModelDev M;
    const FoldinParams c = foldin_params_of(*p, steps);
    return fold_serve(stats, n, v, [&] { return M.open(nullptr, n, V, d2, p->k, nullptr, nullptr, true, p->precision, &v); },
                      [&](auto zero) -> int { return foldin_run<decltype(zero)>(v, c, P, U0, U_out, stats, per_user); });
    });
}

int pcr_fold_in(pcr_solver* s, int64_t n, const int64_t* index, const int32_t* item, const double* val, const double* U0, int steps,
                double* U_out, pcr_foldin_stats* stats, double* per_user) {
    S_OR_ARG;
    return abi_guard("pcr_fold_in", [&]() -> int {
        pcr_params prm;
        RC(s->foldin_params(&prm));
        const ServeView v = solver_view(s, 0);
        PcrFoldinPlan P;
        RC(pcr_fold_in_check("pcr_fold_in", prm.solver_type, v.d2, n, index, item, val, steps, U_out, &P));
        const FoldinParams c = foldin_params_of(prm, steps);
        return fold_serve(stats, n, v, on_solver, [&](auto zero) -> int { return foldin_run<decltype(zero)>(v, c, P, U0, U_out, stats, per_user); });
    });
}

int pcr_fold_in_ridge_model(const double* F, int64_t rows, int64_t k, double lambda, int weighted, int precision, int device, int64_t n,
                            const int64_t* index, const int32_t* item, const double* val, double* U_out, pcr_ridge_stats* stats, double* per_user) {
    return abi_guard("pcr_fold_in_ridge_model", [&]() -> int {
    PcrRidgePlan P;
    RC(pcr_fold_in_ridge_check("pcr_fold_in_ridge_model", true, F, rows, k, lambda, precision, n, index, item, val, U_out, &P));
    RC(model_device(device));
    ServeView v; ModelDev M;
    return fold_serve(stats, n, v, [&] { return M.open(nullptr, n, F, rows, k, nullptr, nullptr, true, precision, &v); }, [&](auto zero) -> int {
        return ridge_run<RidgeFamily, decltype(zero)>(v, lambda, weighted != 0, P, U_out, stats, per_user);
    });
    });
}

int pcr_fold_in_ridge(pcr_solver* s, int weighted, int64_t n, const int64_t* index, const int32_t* item, const double* val, double* U_out,
                      pcr_ridge_stats* stats, double* per_user) {
    S_OR_ARG;
    return abi_guard("pcr_fold_in_ridge", [&]() -> int {
        const ServeView v = solver_view(s, 0);
        const double lambda = s->ridge_lambda();
        PcrRidgePlan P;
        RC(pcr_fold_in_ridge_check("pcr_fold_in_ridge", false, nullptr, v.d2, v.r, lambda, v.dtype, n, index, item, val, U_out, &P));
        return fold_serve(stats, n, v, on_solver, [&](auto zero) -> int {
            return ridge_run<RidgeFamily, decltype(zero)>(v, lambda, weighted != 0, P, U_out, stats, per_user);
        });
    });
}

int pcr_fold_in_conf_model(const double* F, int64_t rows, int64_t k, double lambda, int weighted, double alpha, int precision, int device, int64_t n,
                           const int64_t* index, const int32_t* item, const double* val, const double* weight, double* U_out, pcr_ridge_stats* stats,
                           double* per_user) {
    return abi_guard("pcr_fold_in_conf_model", [&]() -> int {
    PcrConfPlan P;
    RC(pcr_fold_in_conf_check("pcr_fold_in_conf_model", true, F, rows, k, lambda, alpha, precision, n, index, item, val, weight, U_out, &P));
    RC(model_device(device));
    ServeView v; ModelDev M;
    return fold_serve(stats, n, v, [&] { return M.open(nullptr, n, F, rows, k, nullptr, nullptr, true, precision, &v); }, [&](auto zero) -> int {
        return conf_run<decltype(zero)>(v, lambda, weighted != 0, P, U_out, stats, per_user);
    });
    });
}

int pcr_fold_in_conf(pcr_solver* s, int weighted, double alpha, int64_t n, const int64_t* index, const int32_t* item, const double* val,
                     const double* weight, double* U_out, pcr_ridge_stats* stats, double* per_user) {
    S_OR_ARG;
    return abi_guard("pcr_fold_in_conf", [&]() -> int {
        const ServeView v = solver_view(s, 0);
        const double lambda = s->ridge_lambda();
        PcrConfPlan P;
        RC(pcr_fold_in_conf_check("pcr_fold_in_conf", false, nullptr, v.d2, v.r, lambda, alpha, v.dtype, n, index, item, val, weight, U_out, &P));
        return fold_serve(stats, n, v, on_solver, [&](auto zero) -> int {
            return conf_run<decltype(zero)>(v, lambda, weighted != 0, P, U_out, stats, per_user);
        });
    });
}

int pcr_fold_in_nnls_model(const double* F, int64_t rows, int64_t k, double lambda, int weighted, int precision, int device, int64_t n,
                           const int64_t* index, const int32_t* item, const double* val, double* U_out, pcr_nnls_stats* stats, double* per_user) {
    return abi_guard("pcr_fold_in_nnls_model", [&]() -> int {
    PcrRidgePlan P;
    RC(pcr_fold_in_nnls_check("pcr_fold_in_nnls_model", true, F, rows, k, lambda, precision, n, index, item, val, U_out, &P));
    RC(model_device(device));
    ServeView v; ModelDev M;
    return fold_serve(stats, n, v, [&] { return M.open(nullptr, n, F, rows, k, nullptr, nullptr, true, precision, &v); }, [&](auto zero) -> int {
        return ridge_run<NnlsFamily, decltype(zero)>(v, lambda, weighted != 0, P, U_out, stats, per_user);
    });
    });
}

int pcr_fold_in_nnls(pcr_solver* s, int weighted, int64_t n, const int64_t* index, const int32_t* item, const double* val, double* U_out,
                     pcr_nnls_stats* stats, double* per_user) {
    S_OR_ARG;
    return abi_guard("pcr_fold_in_nnls", [&]() -> int {
        const ServeView v = solver_view(s, 0);
        const double lambda = s->ridge_lambda();
        PcrRidgePlan P;
        RC(pcr_fold_in_nnls_check("pcr_fold_in_nnls", false, nullptr, v.d2, v.r, lambda, v.dtype, n, index, item, val, U_out, &P));
        return fold_serve(stats, n, v, on_solver, [&](auto zero) -> int {
            return ridge_run<NnlsFamily, decltype(zero)>(v, lambda, weighted != 0, P, U_out, stats, per_user);
        });
    });
}

int pcr_fold_in_items_model(const pcr_params* p, const double* U, int64_t d1, const double* V, int64_t d2, const int64_t* tr_index,
                            const int32_t* tr_item, const double* tr_val, int64_t n, const int64_t* index, const int32_t* user, const double* val,
                            const double* V0, int steps, double* V_out, pcr_itemfold_stats* stats, double* per_item) {
    return abi_guard("pcr_fold_in_items_model", [&]() -> int {
    PcrItemfoldPlan P;
    RC(pcr_fold_in_items_check("pcr_fold_in_items_model", true, p, U, d1, V, d2, tr_index, tr_item, tr_val, n, index, user, val, steps, V_out, &P));
    RC(model_device(p->device));
    ServeView v; ModelDev M;
    const FoldinParams c = foldin_params_of(*p, steps);
    return fold_serve(stats, n, v, [&] { return M.open(U, d1, V, d2, p->k, nullptr, nullptr, true, p->precision, &v); },
                      [&](auto zero) -> int { return itemfold_run<decltype(zero)>(v, c, P, V0, V_out, stats, per_item); });
    });
}

int pcr_fold_in_items(pcr_solver* s, const pcr_dataset* train, int64_t n, const int64_t* index, const int32_t* user, const double* val,
                      const double* V0, int steps, double* V_out, pcr_itemfold_stats* stats, double* per_item) {
    S_OR_ARG;
    return abi_guard("pcr_fold_in_items", [&]() -> int {
        pcr_params prm;
        if (s->foldin_params(&prm) != PCR_OK) return pcr_solver::pcr_only("pcr_fold_in_items");
        const ServeView v = solver_view(s, 0);
        if (s->comm_nranks() > 1 || s->first_user != 0 || s->n_users != v.d1) {
            pcr_set_error("pcr_fold_in_items: needs every user on the rank; this solver holds a shard");
            return PCR_ERR_STATE;
        }
        if (!train) { pcr_set_error("pcr_fold_in_items: null training data set"); return PCR_ERR_ARG; }
        const PcrCsr& X = train->train;
        if (X.d1 != v.d1 || X.d2 != v.d2 || X.nnz() != v.nnz) {
            pcr_set_error("pcr_fold_in_items: the data set is not the one the solver was created from (dimensions or nnz differ)");
            return PCR_ERR_ARG;
        }
        PcrItemfoldPlan P;
        RC(pcr_fold_in_items_check("pcr_fold_in_items", false, &prm, nullptr, X.d1, nullptr, X.d2, X.index.data(), X.item.data(), X.val.data(), n, index,
                                   user, val, steps, V_out, &P));
        const FoldinParams c = foldin_params_of(prm, steps);
        return fold_serve(stats, n, v, on_solver, [&](auto zero) -> int { return itemfold_run<decltype(zero)>(v, c, P, V0, V_out, stats, per_item); });
    });
}

int pcr_explain_model(const pcr_params* p, const double* V, int64_t d2, int64_t n, const int64_t* index, const int32_t* item, const double* val,
                      const double* U, const double* weights, int L, const int32_t* lists, int E, int32_t* expl_item, double* expl_contrib,
                      double* per_pair, double* per_user, pcr_explain_stats* stats) {
    return abi_guard("pcr_explain_model", [&]() -> int {
    PcrFoldinPlan P;
    RC(pcr_explain_check("pcr_explain_model", true, p, V, d2, n, index, item, val, U, weights, L, lists, E, expl_item, expl_contrib, &P));
    RC(model_device(p->device));
    ServeView v; ModelDev M;
    const ExplainOut o = {expl_item, expl_contrib, per_pair, per_user, stats};
    return fold_serve(stats, n, v, [&] { return M.open(U, n, V, d2, p->k, nullptr, nullptr, true, p->precision, &v); }, [&](auto zero) -> int {
        typedef decltype(zero) T;
        return explain_run<T>(v, p->solver_type, p->lambda, P, serve_U<T>(v), nullptr, weights, L, lists, E, o);
    });
    });
}

int pcr_explain(pcr_solver* s, const pcr_dataset* train, int64_t n, const int32_t* users, const double* weights, int L, const int32_t* lists, int E,
                int32_t* expl_item, double* expl_contrib, double* per_pair, double* per_user, pcr_explain_stats* stats) {
    S_OR_ARG;
    return abi_guard("pcr_explain", [&]() -> int {
        pcr_params prm;
        if (s->foldin_params(&prm) != PCR_OK) return pcr_solver::pcr_only("pcr_explain");
        const ServeView v = solver_view(s, 0);
        SolverRows R;
        RC(solver_rows("pcr_explain", s, v, train, &n, users, &R));
        PcrFoldinPlan P;
        RC(pcr_explain_check("pcr_explain", false, &prm, nullptr, v.d2, n, R.index.data(), R.item.data(), R.val.data(), nullptr, weights, L, lists, E,
                             expl_item, expl_contrib, &P));
        const ExplainOut o = {expl_item, expl_contrib, per_pair, per_user, stats};
        return fold_serve(stats, n, v, on_solver, [&](auto zero) -> int {
            typedef decltype(zero) T;
            return explain_run<T>(v, prm.solver_type, prm.lambda, P, serve_U<T>(v), R.urow.data(), weights, L, lists, E, o);
        });
    });
}

int pcr_explain_ridge_model(const double* F, int64_t rows, int64_t k, double lambda, int weighted, int nonneg, int precision, int device, int64_t n,
                            const int64_t* index, const int32_t* item, const double* val, const double* U, int L, const int32_t* lists, int E,
                            int32_t* expl_item, double* expl_contrib, double* per_pair, double* per_user, pcr_explain_ridge_stats* stats) {
    return abi_guard("pcr_explain_ridge_model", [&]() -> int {
    PcrRidgePlan P;
    RC(pcr_explain_ridge_check("pcr_explain_ridge_model", true, F, rows, k, lambda, nonneg, precision, n, index, item, val, U != nullptr, L, lists, E,
                               expl_item, expl_contrib, &P));
    RC(model_device(device));
    ServeView v; ModelDev M;
    const ExplainRidgeOut o = {expl_item, expl_contrib, per_pair, per_user, stats};
    return fold_serve(stats, n, v, [&] { return M.open(U, n, F, rows, k, nullptr, nullptr, true, precision, &v); }, [&](auto zero) -> int {
        typedef decltype(zero) T;
        return explain_ridge_run<T>(v, lambda, weighted != 0, nonneg != 0, P, U ? serve_U<T>(v) : nullptr, nullptr, L, lists, E, o);
    });
    });
}

int pcr_explain_ridge(pcr_solver* s, const pcr_dataset* train, int64_t n, const int32_t* users, int weighted, int nonneg, int L, const int32_t* lists,
                      int E, int32_t* expl_item, double* expl_contrib, double* per_pair, double* per_user, pcr_explain_ridge_stats* stats) {
    S_OR_ARG;
    return abi_guard("pcr_explain_ridge", [&]() -> int {
        const ServeView v = solver_view(s, 0);
        SolverRows R;
        RC(solver_rows("pcr_explain_ridge", s, v, train, &n, users, &R));
        const double lambda = s->ridge_lambda();
        PcrRidgePlan P;
        RC(pcr_explain_ridge_check("pcr_explain_ridge", false, nullptr, v.d2, v.r, lambda, nonneg, v.dtype, n, R.index.data(), R.item.data(), R.val.data(), true,
                                   L, lists, E, expl_item, expl_contrib, &P));
        const ExplainRidgeOut o = {expl_item, expl_contrib, per_pair, per_user, stats};
        return fold_serve(stats, n, v, on_solver, [&](auto zero) -> int {
            typedef decltype(zero) T;
            return explain_ridge_run<T>(v, lambda, weighted != 0, nonneg != 0, P, serve_U<T>(v), R.urow.data(), L, lists, E, o);
        });
    });
}
}  // extern "C"
