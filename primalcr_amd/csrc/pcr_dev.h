// pcr_dev.h -- host-side device infrastructure shared by the three HIP translation units (pcr_solver.hip: training,
// pcr_serve.hip: recommendation and its metrics, pcr_fold.hip: the fold-in families): error macros, the RAII device buffer, the
// factor upload, the profiler, the solver's base class with the ServeView it hands to the two serving units, what both of them
// need around that view (ModelDev, model_device, solver_view, by_precision), and the C ABI's exception guard.
// Everything here is a template, a class or static inline: no non-template kernel is compiled into two units.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <initializer_list>
#include <map>
#include <memory>
#include <new>
#include <string>
#include <string_view>
#include <vector>

#include "pcr_host.h"
#include "pcr_prims.h"      // k_mat_in

#define HIPCHK(expr)                                                                           \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            pcr_set_error(std::string(#expr) + ": " + hipGetErrorString(e_) + " (" + __FILE__ + ":" + std::to_string(__LINE__) + ")"); \
            return PCR_ERR_DEVICE;                                                             \
        }                                                                                      \
    } while (0)
#define RC(expr) do { int rc_ = (expr); if (rc_ != PCR_OK) return rc_; } while (0)

static inline int host_pow2(int n) { int p = 1; while (p < n) p <<= 1; return p; }
static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
// the LDS of a CU: what a serving kernel's workgroup may ask for, and what the workgroups per CU are counted against
static const size_t PCR_LDS_CU = (size_t)160 * 1024;

// device buffer with RAII
template <typename X>
struct DBuf {
    X* p = nullptr;
    size_t n = 0;
    int alloc(size_t count) {
        free();
        n = count;
        if (count == 0) count = 1;
        HIPCHK(hipMalloc((void**)&p, count * sizeof(X)));
        return PCR_OK;
    }
    int upload(const std::vector<X>& h, hipStream_t st) {
        RC(alloc(h.size()));
        (void)st;
        if (!h.empty()) HIPCHK(hipMemcpy(p, h.data(), h.size() * sizeof(X), hipMemcpyHostToDevice));
        return PCR_OK;
    }
    int upload_n(const X* h, size_t count) {
        RC(alloc(count));
        if (count) HIPCHK(hipMemcpy(p, h, count * sizeof(X), hipMemcpyHostToDevice));
        return PCR_OK;
    }
    void free() { if (p) { (void)hipFree(p); p = nullptr; } n = 0; }
    DBuf() = default;
    DBuf(const DBuf&) = delete;
    DBuf& operator=(const DBuf&) = delete;
    DBuf(DBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DBuf& operator=(DBuf&& o) noexcept { if (this != &o) { free(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; } return *this; }
    ~DBuf() { free(); }
};

// Factor matrices cross the boundary as the reference's fp64 row-major payload (mat_t), k values per row; the device keeps rows
// padded to ld elements of T.  upload_rows converts each {host rows H, row count, device rows D} on the device (k_mat_in) in slabs
// of at most 64 M values, staged straight from the caller's buffer through one device buffer sized for the longest matrix, and
// synchronises st after every slab: no host-side staging copy, no serial conversion loop (48 M values at the Netflix shape).
template <typename T>
struct HostRows { const double* H; int64_t rows; T* D; };
template <typename T>
static int upload_rows(hipStream_t st, int k, int ld, std::initializer_list<HostRows<T>> mats) {
    const int64_t slab_rows = std::max<int64_t>(1, ((int64_t)64 << 20) / k);
    int64_t longest = 0;
    for (const HostRows<T>& m : mats) longest = std::max(longest, m.rows);
    DBuf<double> stage;
    RC(stage.alloc((size_t)std::min(longest, slab_rows) * k));
    for (const HostRows<T>& m : mats)
        for (int64_t r0 = 0; r0 < m.rows; r0 += slab_rows) {
            const int64_t nr = std::min(slab_rows, m.rows - r0);
            HIPCHK(hipMemcpyAsync(stage.p, m.H + r0 * k, (size_t)nr * k * sizeof(double), hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL((k_mat_in<T>), dim3((unsigned)std::min<int64_t>(1 << 16, cdiv(nr * ld, 256))), dim3(256), 0, st, stage.p, m.D + r0 * ld, nr, k, ld);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(st));
        }
    return PCR_OK;
}

// ------------------------------------------------------------------------------ profiling (pcr_profile_*)
struct ProfSlot {
    int64_t ratings = -1, users = -1;      // what one launch covers (-1: the whole shard)
    int64_t seen = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    double ms = 0.0;
    int64_t n = 0;
};
// A solver's named timing slots and the HIP events behind them
struct Profiler {
    bool on = false;
    int period = 1;                       // time every period-th launch of each slot
    std::map<std::string, ProfSlot> slots;
    std::vector<hipEvent_t> pool;         // timing events are recycled: creating one per launch costs more than the launch
    ~Profiler() {
        for (auto& kv : slots)
            for (auto& pr : kv.second.pending) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
        for (hipEvent_t e : pool) (void)hipEventDestroy(e);
    }
    hipEvent_t get() {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        return e;
    }
    void prewarm(int n) {
        while ((int)pool.size() < n) { hipEvent_t e = nullptr; if (hipEventCreate(&e) != hipSuccess) break; pool.push_back(e); }
    }
    // waits for the recorded pairs, adds their times to the slots and returns their events to the pool
    void resolve() {
        for (auto& kv : slots) {
            for (auto& pr : kv.second.pending) {
                float ms = 0.f;
                (void)hipEventSynchronize(pr.second);
                if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) kv.second.ms += ms;
                pool.push_back(pr.first); pool.push_back(pr.second);
            }
            kv.second.pending.clear();
        }
    }
};
// One launch (or group of launches) of slot `name` on stream q, timed by an event pair when it is sampled.  p NULL: not profiled.
struct ProfScope {
    Profiler* p; ProfSlot* slot = nullptr; hipEvent_t a = nullptr, b = nullptr; hipStream_t q;
    ProfScope(Profiler* p_, std::string_view name, hipStream_t q_, int64_t ratings = -1, int64_t users = -1) : p(p_), q(q_) {
        if (!p || !p->on) return;
        ProfSlot* sl = &p->slots[std::string(name)];
        sl->ratings = ratings; sl->users = users;
        // sampled: an event pair costs ~3 us of queue time.  Slots launched once per outer iteration (the U-step classes,
        // the prepares, the fork..join walls) are sampled at least every 4th launch, so that a 20-step run still
        // averages five of them; the per-CG-iteration kernels every period-th
        const bool rare = name.compare(0, 5, "ustep") == 0 || name.compare(0, 5, "wall:") == 0 || name.compare(0, 7, "prepare") == 0;
        const int period = rare ? std::min(p->period, 4) : p->period;
        if ((sl->seen++ % period) != 0) return;
        slot = sl;
        a = p->get(); b = p->get();
        (void)hipEventRecord(a, q);
    }
    ~ProfScope() {
        if (!slot) return;
        (void)hipEventRecord(b, q);
        slot->pending.emplace_back(a, b);
        slot->n += 1;
    }
};

// What the serving layer reads of a trained model: a solver's device state (pcr_solver::serve_view) or the model one call
// uploaded (ModelDev below).  Plain pointers, nothing is owned or written through them.
struct pcr_solver;
enum ServeExchange { SERVE_LOCAL = 0, SERVE_RCCL, SERVE_P2P };     // no exchange step (one shard, or shard-local mode) / which communicator
struct ServeView {
    int dtype = PCR_F64;                       // the type of U and V: PCR_F32 or PCR_F64
    hipStream_t st = nullptr;
    const void *U = nullptr, *V = nullptr;     // device rows of ld values, r of them used
    int r = 0, ld = 0;
    int64_t rows = 0, d1 = 0, d2 = 0;          // rows of U (the shard's users), users of the whole model, items
    // device: the training CSR of the rows (item-ascending per user), for the exclusion and the popularity table
    const int64_t* uptr = nullptr; const int32_t* item = nullptr; int64_t nnz = 0;
    bool exclude = true;                       // this call leaves the training items out
    const int64_t* xptr() const { return exclude ? uptr : nullptr; }
    const int32_t* xitem() const { return exclude ? item : nullptr; }
    // host: the test CSR of the rows
    const int64_t* tptr = nullptr; const int32_t* titem = nullptr; const double* tval = nullptr;
    int select = 1;                            // pcr_tune("recommend_select")
    // device: the packed allow set of a filtered call (bit j & 63 of word j >> 6, cdiv(d2, 64) words; pcr_recommend_filtered):
    // NULL everywhere else, and every item is eligible
    const unsigned long long* allow = nullptr;
    Profiler* prof = nullptr;                  // the "recommend/..." and "ranks/..." slots (NULL: not profiled)
    int exchange = SERVE_LOCAL;
    pcr_solver* owner = nullptr;               // whose communicator sum() and wait() use (NULL: a model, nothing to exchange)
    int sum(double* dev, size_t count) const;  // dev[0..count) summed across the ranks, in place, on st
    int wait() const;                          // synchronises st; a peer-to-peer exchange that missed its deadline is reported here
};
template <typename T> static const T* serve_U(const ServeView& v) { return static_cast<const T*>(v.U); }
template <typename T> static const T* serve_V(const ServeView& v) { return static_cast<const T*>(v.V); }
// run(T()) for the view's precision
template <class F>
static int by_precision(const ServeView& v, F&& run) { return v.dtype == PCR_F64 ? run(0.0) : run(0.0f); }
struct ServeState;                             // the serving layer's cached device tables (pcr_serve.hip)

struct pcr_solver {
    pcr_solver();
    virtual ~pcr_solver();                                         // (both in pcr_serve.hip, where ServeState is complete)
    virtual int set_factors(const double* U, const double* V, bool local) = 0;
    virtual int get_factors(double* U, double* V, bool local) = 0;
    // PrimalCR / PrimalCR++ only (Solver<T>)
    static int pcr_only(const char* what) {
        pcr_set_error(std::string(what) + ": a PrimalCR / PrimalCR++ entry point; this solver is CCDR1 (solver type 0)");
        return PCR_ERR_STATE;
    }
    virtual int comp_m(double*) { return pcr_only("pcr_comp_m"); }
    virtual int objective(double*) { return pcr_only("pcr_objective"); }
    virtual int obtain_g(double*) { return pcr_only("pcr_obtain_g"); }
    virtual int compute_Ha(const double*, double*) { return pcr_only("pcr_compute_Ha"); }
    virtual int solve_delta(const double*, double*, int*) { return pcr_only("pcr_solve_delta"); }
    virtual int update_V(double*, int*) { return pcr_only("pcr_update_V"); }
    virtual int update_U(double*, int64_t*) { return pcr_only("pcr_update_U"); }
    virtual int foldin_params(pcr_params*) { return pcr_only("pcr_fold_in"); }    // the parameters pcr_fold_in runs with
    // per-user loss weights (w: d1 of the job, or this rank's n_users with local; NULL: unweighted)
    virtual int set_user_weights(const double*, bool) {
        pcr_set_error("pcr_solver_set_user_weights: per-user loss weights exist for PrimalCR / PrimalCR++ only; this solver is CCDR1 (solver type 0)");
        return PCR_ERR_UNSUPPORTED;
    }
    virtual double ridge_lambda() = 0;                             // the lambda pcr_fold_in_ridge runs with (every solver type)
    virtual int evaluate(int which, int ndcg_k, double* err, double* ndcg) = 0;
    virtual int train(pcr_log_fn log, void* ctx, pcr_iter_stats* hist) = 0;
    virtual int iterate_abi(int n, pcr_iter_stats* out) = 0;
    virtual int comm_init(const void* id) = 0;
    virtual int comm_init_p2p(const char* shm_name) = 0;
    virtual void comm_abort() = 0;
    virtual int comm_nranks() = 0;
    virtual int sync() = 0;
    virtual std::string ustep_classes() = 0;                       // comma-separated profile slot names of the U-step length classes
    virtual int class_rows(const std::string& slot, double* v) = 0; // rows of V that class has gathered so far (pcr_tune "count_rows")
    int64_t first_user = 0, n_users = 0, nnz_local = 0;
    double ustep_rows = 0.0;      // rows of V gathered by all U steps so far (all ranks); pcr_solver_counter("ustep_row_gathers")
    bool local_only = false;      // nranks > 1 without a communicator: entry points return this shard's partials
    Profiler prof;
    std::vector<std::pair<std::string, double>> setup_ms;   // wall time of the phases of pcr_solver_create, in order (pcr_solver_counter "setup_ms/<i>", pcr_solver_setup_phase)
    // CCDR1 only (pcr_ccd.h): the "ccd_residual_mismatch" counter, pcr_solver_set_ccd_params
    virtual int residual_mismatch(double*) { pcr_set_error("pcr_solver_counter: 'ccd_residual_mismatch' exists on a CCDR1 solver only"); return PCR_ERR_STATE; }
    virtual int set_ccd_params(const pcr_ccd_params*) { pcr_set_error("pcr_solver_set_ccd_params: not a CCDR1 solver (solver type 0)"); return PCR_ERR_STATE; }
    // per-rating confidence weights (w: nnz, training-CSR order; NULL: unweighted) and the "ccd_rating_weights" counter
    virtual int set_rating_weights(const double*) {
        pcr_set_error("pcr_solver_set_rating_weights: per-rating weights exist for CCDR1 (solver type 0) only; PrimalCR / PrimalCR++ take "
                      "per-user loss weights: pcr_solver_set_user_weights");
        return PCR_ERR_UNSUPPORTED;
    }
    virtual int rating_weights_set(double*) { pcr_set_error("pcr_solver_counter: 'ccd_rating_weights' exists on a CCDR1 solver only"); return PCR_ERR_STATE; }
    // implicit feedback (alpha: the weight of every unrated cell; 0: off) and the "ccd_implicit" counter
    virtual int set_implicit(double) {
        pcr_set_error("pcr_solver_set_implicit: implicit feedback exists for CCDR1 (solver type 0) only; the ranking losses of PrimalCR / "
                      "PrimalCR++ compare a user's rated items with each other and have no term for an unrated cell");
        return PCR_ERR_UNSUPPORTED;
    }
    virtual int implicit_alpha(double*) { pcr_set_error("pcr_solver_counter: 'ccd_implicit' exists on a CCDR1 solver only"); return PCR_ERR_STATE; }
    // the serving layer (pcr_serve.hip, pcr_fold.hip): the view of this solver's factors and shard, the exchange behind ServeView::sum (sync()
    // is ServeView::wait), the tables it keeps between calls
    virtual void serve_view(ServeView* v) = 0;
    virtual int allreduce_f64(double*, size_t) { return PCR_OK; }
    std::unique_ptr<ServeState> serve;
};

// s's view for one call: the launches are timed in s's profiler (that of a CCDR1 solver, not of the Solver<T> it holds)
static inline ServeView solver_view(pcr_solver* s, int flags) {
    ServeView v;
    s->serve_view(&v); v.exclude = (flags & PCR_REC_EXCLUDE_TRAIN) != 0;
    return v;
}

// A model in host memory on the device for one call: the exclusion CSR (item-ascending rows: a CSR that is not gets a sorted
// copy, for the kernel's cursor) and both host fp64 factors in the requested type, rows padded to ld: U then V in one buffer.
// open() fills the view: the default stream, nothing profiled, nothing exchanged.
struct ModelDev {
    DBuf<int64_t> dx;
    DBuf<int32_t> di;
    DBuf<char> F;
    int open(const double* U, int64_t d1, const double* V, int64_t d2, int64_t k, const int64_t* index, const int32_t* item, bool sorted,
             int dtype, ServeView* v) {
        if (index) {
            std::vector<int32_t> sitem;
            const int64_t nnz = index[d1];
            if (!sorted) {
                sitem.assign(item, item + nnz);
                pcr_parallel_ranges(d1, pcr_host_threads(), [&](int, int64_t lo, int64_t hi) {
                    for (int64_t u = lo; u < hi; ++u) std::sort(sitem.begin() + index[u], sitem.begin() + index[u + 1]);
                });
            }
            RC(dx.upload_n(index, (size_t)d1 + 1)); RC(di.upload_n(sorted ? item : sitem.data(), (size_t)nnz));
        }
        const int ld = ((int)k + 3) & ~3;
        const size_t row = (size_t)ld * (dtype == PCR_F64 ? sizeof(double) : sizeof(float));
        const int64_t ur = U ? d1 : 0;             // (U NULL: pcr_evaluate_lists_model scores nothing and brings no user factors)
        RC(F.alloc((size_t)(ur + d2) * row));
        char* dV = F.p + (size_t)ur * row;
        if (dtype == PCR_F64) RC(upload_rows<double>(v->st, (int)k, ld, {{U, ur, (double*)F.p}, {V, d2, (double*)dV}}));
        else RC(upload_rows<float>(v->st, (int)k, ld, {{U, ur, (float*)F.p}, {V, d2, (float*)dV}}));
        v->dtype = dtype; v->U = F.p; v->V = dV; v->r = (int)k; v->ld = ld; v->rows = v->d1 = d1; v->d2 = d2;
        v->uptr = dx.p; v->item = di.p; v->nnz = index ? index[d1] : 0;
        return PCR_OK;
    }
};

static inline int model_device(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { pcr_set_error("no HIP device available"); return PCR_ERR_DEVICE; }
    if (device < 0 || device >= ndev) { pcr_set_error("device ordinal out of range"); return PCR_ERR_ARG; }
    HIPCHK(hipSetDevice(device));
    return PCR_OK;
}

// ------------------------------------------------------------------------------------------ C ABI
// No C++ exception may cross the C ABI (a host allocation that fails while a 700 M-rating shard is being set up is an error
// code, not std::terminate).
template <class F>
static int abi_guard(const char* what, F&& body) noexcept {
    try { return body(); }
    catch (const std::bad_alloc&) { try { pcr_set_error(std::string(what) + ": out of host memory"); } catch (...) {} return PCR_ERR_NOMEM; }
    catch (const std::exception& e) { try { pcr_set_error(std::string(what) + ": " + e.what()); } catch (...) {} return PCR_ERR_ARG; }
    catch (...) { return PCR_ERR_ARG; }
}
#define PCR_ABI(name, expr) return abi_guard(name, [&]() -> int { return (expr); })
#define S_OR_ARG if (!s) { pcr_set_error("null solver"); return PCR_ERR_ARG; }
