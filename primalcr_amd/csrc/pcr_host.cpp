// pcr_host.cpp -- host data path of libprimalcr: meta/ratings loader, CSR conversion, level
// ranking, model file I/O, initial(), user partitioning.  No GPU calls in this file.
//
// Mirrors the *formats and semantics* of the reference (file:line cited per function); the
// reference's vector<vector<double>> / smat_t containers are not reproduced.
#include "pcr_host.h"

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <climits>
#include <cstdint>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <functional>
#include <limits>
#include <memory>
#include <mutex>
#include <numeric>
#include <random>
#include <thread>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

static thread_local std::string g_err;
void pcr_set_error(const std::string& msg) { g_err = msg; }

extern "C" const char* pcr_last_error(void) { return g_err.c_str(); }

// No C++ exception may cross the C ABI: a header that promises 2^60 ratings, a meta file with a negative count or a machine
// that is simply out of memory must come back as an error code, not as std::terminate (found by the malformed-input test,
// tests/test_host_abi.py, which also runs under AddressSanitizer).
template <class F>
static int guarded(const char* what, F&& body) noexcept {
    try { return body(); }
    catch (const std::bad_alloc&) { try { pcr_set_error(std::string(what) + ": out of memory"); } catch (...) {} return PCR_ERR_NOMEM; }
    catch (const std::exception& e) { try { pcr_set_error(std::string(what) + ": " + e.what()); } catch (...) {} return PCR_ERR_ARG; }
    catch (...) { return PCR_ERR_ARG; }
}
// Worker threads of the host data path: `n_workers` std::threads run body(worker index); an exception thrown on a worker (a failed
// allocation inside a counting sort, say) must not end the process through std::terminate -- the first one is carried back and
// rethrown on the calling thread, where the entry point's guard turns it into an error code.
template <class Body>
static void run_workers(int n_workers, Body&& body) {
    if (n_workers <= 1) { body(0); return; }
    std::exception_ptr first;
    std::mutex mu;
    auto safe = [&](int w) {
        try { body(w); }
        catch (...) { std::lock_guard<std::mutex> lk(mu); if (!first) first = std::current_exception(); }
    };
    std::vector<std::thread> th;
    th.reserve((size_t)n_workers - 1);
    try {
        for (int w = 1; w < n_workers; ++w) th.emplace_back(safe, w);
    } catch (...) {                                        // (thread creation failed: finish with the threads that exist)
        std::lock_guard<std::mutex> lk(mu);
        if (!first) first = std::current_exception();
    }
    safe(0);
    for (auto& x : th) x.join();
    if (first) std::rethrow_exception(first);
}

static const int64_t kMaxDim = ((int64_t)1 << 31) - 2;             // ids are int32 throughout (the device solver's limit too)
extern "C" const char* pcr_version(void) { return "primalcr-mi355x 0.1 (gfx950)"; }

// pmf.h:27-48
extern "C" void pcr_params_default(pcr_params* p) {
    p->solver_type = PCR_SOLVER_PCRPP;
    p->k = 10;
    p->threads = 4;
    p->maxiter = 10;
    p->lambda = 5000;
    p->do_predict = 1;
    p->verbose = 0;
    p->stepsize = 1.0;
    p->ndcg_k = 10;
    p->precision = PCR_F32;
    p->device = 0;
    p->cg_max_iter = 10;
    p->cg_tol = 0.01;
}

// (initial(): pcr_initial.cpp -- a translation unit of its own, compiled by g++)

// ------------------------------------------------------------------------------------------
// CSR conversion
// ------------------------------------------------------------------------------------------

// fn(t, lo, hi) over T contiguous pieces of [0, n), one std::thread each (T = 1: on the calling thread)
template <class F>
static void run_pieces(int64_t n, int T, F&& fn) {
    T = (int)std::max<int64_t>(1, std::min<int64_t>(T, n));
    if (T == 1) { fn(0, (int64_t)0, n); return; }
    run_workers(T, [&](int t) { fn(t, n * t / T, n * (t + 1) / T); });
}
static int pieces_for(int64_t n, int threads) { return (int)std::max<int64_t>(1, std::min<int64_t>(std::min(threads, 64), n / 65536 + 1)); }

// index[u] = number of entries whose key is below u, for a NON-DECREASING key sequence key[0, n) with values in [0, d1):
// every piece writes the index entries of the keys that first appear in it (each entry is written exactly once).
static void index_of_sorted_keys(const int32_t* key, int64_t n, int64_t d1, int64_t* index, int T) {
    if (n == 0) { std::fill(index, index + d1 + 1, (int64_t)0); return; }
    run_pieces(n, T, [&](int, int64_t lo, int64_t hi) {
        int64_t prev = lo == 0 ? -1 : key[lo - 1];
        for (int64_t z = lo; z < hi; ++z) {
            const int64_t k = key[z];
            if (k != prev) { for (int64_t u = prev + 1; u <= k; ++u) index[u] = z; prev = k; }
        }
        if (hi == n) for (int64_t u = prev + 1; u <= d1; ++u) index[u] = n;
    });
}

// util.h:223-247 sorts entries by (row, col); util.cpp:229-243 walks them user by user: items ascending inside a user.
// `threads` host threads throughout:
//   * the usual case -- the file is already ordered by (user, item), as the reference's own data sets and the generators'
//     are -- is detected piece by piece during the range check and needs no data movement at all: the parsed item / value
//     arrays ARE the CSR (they are adopted when the caller hands them over in X, copied in parallel otherwise) and the row
//     pointers come from the first occurrence of every user;
//   * anything else: entries are scattered into user-range buckets (per piece and bucket counts -> offsets, file order kept
//     inside a bucket), then every bucket -- on its own thread -- does its counting sort by user and, where a user's items are
//     not ascending, a stable sort by item (equal (user, item) pairs keep their file order).
// adopt = item / val point at X.item / X.val (sized nnz) already.
static int build_train_csr(int64_t d1, int64_t d2, int64_t nnz, const int32_t* user, const int32_t* item,
                           const double* val, PcrCsr& X, int threads, bool adopt) {
    X.d1 = d1; X.d2 = d2;
    X.index.resize((size_t)d1 + 1);
    const int T = pieces_for(nnz, threads);
    struct Piece { int64_t bad = -1; bool sorted = true; };
    std::vector<Piece> pc((size_t)T);
    run_pieces(nnz, T, [&](int t, int64_t lo, int64_t hi) {
        Piece& P = pc[(size_t)t];
        int64_t pu = lo > 0 ? user[lo - 1] : -1, pi = lo > 0 ? item[lo - 1] : -1;      // (the pair before the piece: the seam counts too)
        for (int64_t z = lo; z < hi; ++z) {
            const int64_t u = user[z], i = item[z];
            if (u < 0 || u >= d1 || i < 0 || i >= d2) { P.bad = z; return; }
            if (u < pu || (u == pu && i < pi)) P.sorted = false;
            pu = u; pi = i;
        }
    });
    bool sorted = true;
    for (const Piece& P : pc) {
        if (P.bad >= 0) {
            int64_t first_bad = P.bad;
            for (const Piece& Q : pc) if (Q.bad >= 0) first_bad = std::min(first_bad, Q.bad);
            pcr_set_error("rating " + std::to_string(first_bad) + " has user/item id outside the meta dimensions");
            return PCR_ERR_ARG;
        }
        sorted = sorted && P.sorted;
    }
    if (sorted) {
        index_of_sorted_keys(user, nnz, d1, X.index.data(), T);
        if (!adopt) {
            X.item.resize((size_t)nnz); X.val.resize((size_t)nnz);
            run_pieces(nnz, T, [&](int, int64_t lo, int64_t hi) {
                std::copy(item + lo, item + hi, X.item.data() + lo);
                std::copy(val + lo, val + hi, X.val.data() + lo);
            });
        }
        return PCR_OK;
    }
    // ---- general path
    const int64_t NB = std::max<int64_t>(1, std::min<int64_t>(d1, (int64_t)T * 8));   // user-range buckets (more than threads: balance)
    const int64_t bw = (d1 + NB - 1) / NB;
    std::vector<int64_t> cnt((size_t)T * NB, 0);
    run_pieces(nnz, T, [&](int t, int64_t lo, int64_t hi) {
        int64_t* c = cnt.data() + (size_t)t * NB;
        for (int64_t z = lo; z < hi; ++z) c[user[z] / bw]++;
    });
    std::vector<int64_t> bstart((size_t)NB + 1, 0);
    for (int64_t b = 0; b < NB; ++b) {
        int64_t acc = bstart[b];
        for (int t = 0; t < T; ++t) { const int64_t c = cnt[(size_t)t * NB + b]; cnt[(size_t)t * NB + b] = acc; acc += c; }
        bstart[b + 1] = acc;
    }
    pcr_vec<int32_t> bu((size_t)nnz), bi((size_t)nnz);
    pcr_vec<double> bv((size_t)nnz);
    run_pieces(nnz, T, [&](int t, int64_t lo, int64_t hi) {
        int64_t* c = cnt.data() + (size_t)t * NB;
        for (int64_t z = lo; z < hi; ++z) {
            const int64_t q = c[user[z] / bw]++;
            bu[q] = user[z]; bi[q] = item[z]; bv[q] = val[z];
        }
    });
    pcr_vec<int32_t> oi((size_t)nnz);
    pcr_vec<double> ov((size_t)nnz);
    std::atomic<int64_t> next{0};
    auto bucket_work = [&]() {
        std::vector<int64_t> cur;
        std::vector<std::pair<int32_t, double>> tmp;
        for (;;) {
            const int64_t b = next.fetch_add(1);
            if (b >= NB) break;
            const int64_t ulo = b * bw, uhi = std::min(d1, ulo + bw), a = bstart[b], e = bstart[b + 1];
            if (ulo >= uhi) continue;
            cur.assign((size_t)(uhi - ulo) + 1, 0);
            for (int64_t z = a; z < e; ++z) cur[(size_t)(bu[z] - ulo) + 1]++;
            int64_t acc = a;                                             // entries of users below ulo = the bucket's start
            for (int64_t u = ulo; u < uhi; ++u) { const int64_t c = cur[(size_t)(u - ulo) + 1]; X.index[u] = acc; cur[(size_t)(u - ulo)] = acc; acc += c; }
            for (int64_t z = a; z < e; ++z) { const int64_t q = cur[(size_t)(bu[z] - ulo)]++; oi[q] = bi[z]; ov[q] = bv[z]; }
            for (int64_t u = ulo; u < uhi; ++u) {
                const int64_t ua = X.index[u], ub = u + 1 < uhi ? X.index[u + 1] : e;
                bool asc = true;
                for (int64_t q = ua + 1; q < ub && asc; ++q) asc = oi[q - 1] <= oi[q];
                if (asc) continue;
                tmp.resize((size_t)(ub - ua));
                for (int64_t q = ua; q < ub; ++q) tmp[(size_t)(q - ua)] = {oi[q], ov[q]};
                std::stable_sort(tmp.begin(), tmp.end(), [](const std::pair<int32_t, double>& x, const std::pair<int32_t, double>& y) { return x.first < y.first; });
                for (int64_t q = ua; q < ub; ++q) { oi[q] = tmp[(size_t)(q - ua)].first; ov[q] = tmp[(size_t)(q - ua)].second; }
            }
        }
    };
    run_workers(T, [&](int) { bucket_work(); });
    for (int64_t u = NB * bw; u < d1; ++u) X.index[u] = nnz;              // (none: NB * bw >= d1)
    X.index[d1] = nnz;
    X.item.swap(oi); X.val.swap(ov);
    return PCR_OK;
}

// util.cpp:250-274: the test file is assumed user-sorted; the reference's cursor walks the users 0, 1, ... and appends entries
// while their user id is not above the cursor -- so an entry lands in the row of the LARGEST user id seen so far (itself
// included), and the scan ends for good at the first id that is not a user (>= d1): that entry and everything behind it are
// dropped.  Mirrored, in parallel: per-piece maxima -> carried-in running maximum -> row of every entry -> row pointers as for
// sorted keys.  adopt = item / val point at X.item / X.val (sized nnz); they are cut at the end of the scan.
static void build_test_csr(int64_t d1, int64_t d2, int64_t nnz, const int32_t* user, const int32_t* item,
                           const double* val, PcrCsr& X, int threads, bool adopt) {
    X.d1 = d1; X.d2 = d2;
    X.index.resize((size_t)d1 + 1);
    const int T = pieces_for(nnz, threads);
    std::vector<int64_t> pmax((size_t)T + 1, -1);
    run_pieces(nnz, T, [&](int t, int64_t lo, int64_t hi) {
        int64_t m = -1;
        for (int64_t z = lo; z < hi; ++z) m = std::max<int64_t>(m, user[z]);
        pmax[(size_t)t + 1] = m;
    });
    pmax[0] = 0;                                                          // the cursor starts at user 0
    for (int t = 0; t < T; ++t) pmax[(size_t)t + 1] = std::max(pmax[(size_t)t], pmax[(size_t)t + 1]);
    pcr_vec<int32_t> row((size_t)nnz);
    std::vector<int64_t> stop((size_t)T, nnz);
    run_pieces(nnz, T, [&](int t, int64_t lo, int64_t hi) {
        int64_t m = pmax[(size_t)t];
        for (int64_t z = lo; z < hi; ++z) {
            m = std::max<int64_t>(m, user[z]);
            if (m >= d1) { stop[(size_t)t] = z; for (; z < hi; ++z) row[z] = 0; return; }
            row[z] = (int32_t)m;
        }
    });
    int64_t keep = nnz;
    for (int t = 0; t < T; ++t) keep = std::min(keep, stop[(size_t)t]);
    index_of_sorted_keys(row.data(), keep, d1, X.index.data(), T);
    if (!adopt) {
        X.item.resize((size_t)keep); X.val.resize((size_t)keep);
        run_pieces(keep, T, [&](int, int64_t lo, int64_t hi) {
            std::copy(item + lo, item + hi, X.item.data() + lo);
            std::copy(val + lo, val + hi, X.val.data() + lo);
        });
    } else {
        X.item.resize((size_t)keep); X.val.resize((size_t)keep);
    }
}

// pcr_dataset::traw_*: the file's test triplets, kept only when the test CSR cannot stand for them
static void keep_raw_test(pcr_dataset& ds, int64_t d1, int64_t tnnz, const int32_t* tuser, const int32_t* titem, const double* tval) {
    bool as_is = true;
    for (int64_t z = 0; z < tnnz && as_is; ++z) as_is = tuser[z] < d1 && (z == 0 || tuser[z] >= tuser[z - 1]);
    if (as_is) return;
    ds.traw_user.assign(tuser, tuser + tnnz);
    ds.traw_item.assign(titem, titem + tnnz);
    ds.traw_val.assign(tval, tval + tnnz);
}

static int check_test_ids(int64_t d2, int64_t tnnz, const int32_t* tuser, const int32_t* titem, int threads) {
    const int T = pieces_for(tnnz, threads);
    std::vector<int64_t> bad((size_t)T, -1);
    run_pieces(tnnz, T, [&](int t, int64_t lo, int64_t hi) {
        for (int64_t z = lo; z < hi; ++z)
            if (titem[z] < 0 || titem[z] >= d2 || tuser[z] < 0) { bad[(size_t)t] = z; return; }
    });
    for (int64_t b : bad)
        if (b >= 0) {
            pcr_set_error("test rating " + std::to_string(b) + " has user/item id outside the meta dimensions");
            return PCR_ERR_ARG;
        }
    return PCR_OK;
}

extern "C" int pcr_dataset_from_triplets(int64_t d1, int64_t d2, int64_t nnz, const int32_t* user,
                                         const int32_t* item, const double* val, int64_t tnnz,
                                         const int32_t* tuser, const int32_t* titem, const double* tval,
                                         pcr_dataset** out) {
    if (!out || d1 < 0 || d2 < 0 || nnz < 0 || tnnz < 0 || (nnz > 0 && (!user || !item || !val)) ||
        (tnnz > 0 && (!tuser || !titem || !tval))) {
        pcr_set_error("pcr_dataset_from_triplets: bad argument");
        return PCR_ERR_ARG;
    }
    if (d1 > kMaxDim || d2 > kMaxDim) { pcr_set_error("pcr_dataset_from_triplets: more than 2^31 - 2 users or items"); return PCR_ERR_UNSUPPORTED; }
    return guarded("pcr_dataset_from_triplets", [&]() -> int {
        std::unique_ptr<pcr_dataset> ds(new pcr_dataset());
        const int threads = pcr_host_threads();
        int rc = build_train_csr(d1, d2, nnz, user, item, val, ds->train, threads, false);
        if (rc != PCR_OK) return rc;
        rc = check_test_ids(d2, tnnz, tuser, titem, threads);
        if (rc != PCR_OK) return rc;
        keep_raw_test(*ds, d1, tnnz, tuser, titem, tval);
        build_test_csr(d1, d2, tnnz, tuser, titem, tval, ds->test, threads, false);
        ds->tnnz_file = tnnz;
        *out = ds.release();
        return PCR_OK;
    });
}

// The same data set from arrays that already ARE the reference's SparseMat layout (util.h:390-413: what convert() leaves,
// util.cpp:219-274): index[d1+1], item[nnz], val[nnz], items ascending inside a user for the training set (checked; the
// test set is taken as given).  No triplet round trip for callers that hold CSRs (100 M-rating synthetic sets).
extern "C" int pcr_dataset_from_csr(int64_t d1, int64_t d2, const int64_t* index, const int32_t* item, const double* val,
                                    const int64_t* tindex, const int32_t* titem, const double* tval, pcr_dataset** out) {
    if (!out || d1 < 0 || d2 < 0 || !index || index[0] != 0 || (tindex && tindex[0] != 0)) {
        pcr_set_error("pcr_dataset_from_csr: bad argument");
        return PCR_ERR_ARG;
    }
    const int64_t nnz = index[d1], tnnz = tindex ? tindex[d1] : 0;
    if (nnz < 0 || tnnz < 0 || (nnz > 0 && (!item || !val)) || (tnnz > 0 && (!titem || !tval))) {
        pcr_set_error("pcr_dataset_from_csr: bad argument");
        return PCR_ERR_ARG;
    }
    for (int64_t u = 0; u < d1; ++u) {
        if (index[u + 1] < index[u] || (tindex && tindex[u + 1] < tindex[u])) { pcr_set_error("pcr_dataset_from_csr: index not monotone"); return PCR_ERR_ARG; }
        for (int64_t z = index[u]; z < index[u + 1]; ++z)
            if (item[z] < 0 || item[z] >= d2 || (z > index[u] && item[z] <= item[z - 1])) {
                pcr_set_error("pcr_dataset_from_csr: user " + std::to_string(u) + ": item ids must be ascending and inside [0, d2)");
                return PCR_ERR_ARG;
            }
    }
    for (int64_t z = 0; z < tnnz; ++z)
        if (titem[z] < 0 || titem[z] >= d2) { pcr_set_error("pcr_dataset_from_csr: test item id outside [0, d2)"); return PCR_ERR_ARG; }
    if (d1 > kMaxDim || d2 > kMaxDim) { pcr_set_error("pcr_dataset_from_csr: more than 2^31 - 2 users or items"); return PCR_ERR_UNSUPPORTED; }
    return guarded("pcr_dataset_from_csr", [&]() -> int {
        std::unique_ptr<pcr_dataset> ds(new pcr_dataset());
        ds->train.d1 = ds->test.d1 = d1; ds->train.d2 = ds->test.d2 = d2;
        ds->train.index.assign(index, index + d1 + 1);
        ds->train.item.assign(item, item + nnz);
        ds->train.val.assign(val, val + nnz);
        if (tindex) ds->test.index.assign(tindex, tindex + d1 + 1); else ds->test.index.assign(d1 + 1, 0);
        ds->test.item.assign(titem, titem + tnnz);
        ds->test.val.assign(tval, tval + tnnz);
        ds->tnnz_file = tnnz;
        *out = ds.release();
        return PCR_OK;
    });
}

// ------------------------------------------------------------------------------------------
// launch knobs (pcr_tune): a key/value table PER CALLING THREAD, which pcr_solver_create (on that thread) snapshots into the
// solver -- no process-global mutable state: two threads that create solvers with different knobs do not see each other's
// ------------------------------------------------------------------------------------------
#include <map>
static std::map<std::string, std::string>& tune_table() { static thread_local std::map<std::string, std::string> t; return t; }
static const char* const TUNE_KEYS[] = {"ustep_mode", "cluster_k", "cluster_users", "ubins", "ustep_gram", "spmm_tiles", "spmm_chunk", "sddmm_csc",
                                        "lanes", "pipeline", "window_cache", "prepare_merged", "resort_window", "allreduce_chunks", "p2p_ll",
                                        "p2p_timeout_ms", "p2p_queue_budget", "count_rows", "debug", "win16", "ustep_win_lds", "plan_key64", "ustep_newton", "vblock_users", "recommend_select", "ranks_batch_users", "sample_threads", "rerank_lds", "ridge_form", "nnls_form", "itemfold_table_bytes", "fault_cluster_member", "fault_p2p_skip", "fault_p2p_coarse", nullptr};
extern "C" int pcr_tune(const char* key, const char* value) {
    if (!key) { pcr_set_error("pcr_tune: null key"); return PCR_ERR_ARG; }
    bool known = false;
    for (const char* const* k = TUNE_KEYS; *k; ++k) known = known || !strcmp(*k, key);
    if (!known) { pcr_set_error(std::string("pcr_tune: unknown key '") + key + "'"); return PCR_ERR_ARG; }
    if (value) tune_table()[key] = value; else tune_table().erase(key);
    return PCR_OK;
}
bool pcr_tune_get(const char* key, std::string* out) {
    auto it = tune_table().find(key);
    if (it == tune_table().end()) return false;
    if (out) *out = it->second;
    return true;
}
int pcr_tune_int(const char* key, int dflt) {
    std::string v;
    return pcr_tune_get(key, &v) ? atoi(v.c_str()) : dflt;
}

// ------------------------------------------------------------------------------------------
// text loader (util.cpp:6-25, util.h:118-131, util.h:360-371)
// ------------------------------------------------------------------------------------------

// A rating file as one read-only byte range: mmap for regular files (no copy, no zero-filled staging buffer; the parser
// threads fault their own pieces in), a heap buffer for anything that cannot be mapped (pipes, /proc, empty files).
struct TextFile {
    const char* p = nullptr;
    size_t len = 0;
    void* map = nullptr;
    size_t map_len = 0;
    pcr_vec<char> heap;
    ~TextFile() { if (map) munmap(map, map_len); }
    int open(const std::string& path) {
        const int fd = ::open(path.c_str(), O_RDONLY | O_CLOEXEC);
        if (fd < 0) { pcr_set_error("can't open " + path + ": " + strerror(errno)); return PCR_ERR_IO; }
        struct stat sb;
        if (fstat(fd, &sb) == 0 && S_ISREG(sb.st_mode) && sb.st_size > 0) {
            void* m = mmap(nullptr, (size_t)sb.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
            if (m != MAP_FAILED) {
                (void)madvise(m, (size_t)sb.st_size, MADV_WILLNEED);
                map = m; map_len = (size_t)sb.st_size; p = static_cast<const char*>(m); len = map_len;
                ::close(fd);
                return PCR_OK;
            }
        }
        size_t cap = (size_t)1 << 20, got = 0;
        heap.resize(cap);
        for (;;) {
            const ssize_t n = ::read(fd, heap.data() + got, cap - got);
            if (n < 0) { if (errno == EINTR) continue; ::close(fd); pcr_set_error("can't read " + path + ": " + strerror(errno)); return PCR_ERR_IO; }
            if (n == 0) break;
            got += (size_t)n;
            if (got == cap) { cap *= 2; heap.resize(cap); }
        }
        ::close(fd);
        p = heap.data(); len = got;
        return PCR_OK;
    }
};

// strtol / strtod need a terminated string and the mapped file has none: the (rare) libc path parses a bounded copy.
struct SlowCopy {
    char buf[512];
    size_t n;
    SlowCopy(const char* p, const char* end) { n = std::min<size_t>(sizeof(buf) - 1, (size_t)(end - p)); memcpy(buf, p, n); buf[n] = 0; }
};

// One rating "user item value" (util.h:126, util.h:367).  Fast path for the common "digits digits
// [-]digits[.digits]" shape, strtol/strtod for anything else (exponents, inf, ...).
static inline bool parse_one(const char*& p, const char* end, int32_t& u, int32_t& it, double& v) {
    auto skip_ws = [&]() { while (p < end && (*p == ' ' || *p == '\t' || *p == '\n' || *p == '\r')) ++p; };
    auto parse_uint = [&](long& out) -> bool {
        skip_ws();
        const char* s = p;
        long x = 0;
        while (p < end && *p >= '0' && *p <= '9') { if (x < ((long)1 << 40)) x = x * 10 + (*p - '0'); ++p; }     // (saturates: an absurd token is an id out of range, not an overflow)
        if (p == s || (p < end && (*p == '.' || *p == '-' || *p == '+' || *p == 'e' || *p == 'E'))) { p = s; return false; }
        out = x;
        return true;
    };
    const char* save = p;
    long a, b;
    if (parse_uint(a) && parse_uint(b)) {
        skip_ws();
        const char* s = p;
        bool neg = false;
        if (p < end && (*p == '-' || *p == '+')) { neg = *p == '-'; ++p; }
        long ip = 0; int nd = 0;
        while (p < end && *p >= '0' && *p <= '9' && nd < 15) { ip = ip * 10 + (*p - '0'); ++p; ++nd; }
        bool simple = nd > 0 || (p < end && *p == '.');
        double val = (double)ip;
        if (simple && p < end && *p == '.') {
            ++p;
            long fp = 0; int fd = 0;
            while (p < end && *p >= '0' && *p <= '9' && fd < 15) { fp = fp * 10 + (*p - '0'); ++p; ++fd; }
            static const double P10[16] = {1, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15};
            // exact only when the decimal is short; otherwise defer to strtod for correct rounding
            if (nd + fd > 15 || (p < end && *p >= '0' && *p <= '9')) simple = false;
            else if (fd > 0) val = (double)(ip * (long)P10[fd] + fp) / P10[fd];
        }
        // 1-based ids that do not fit int32 are malformed lines, not ids that wrap around into the valid range
        if (a < 1 || b < 1 || a > (long)INT32_MAX || b > (long)INT32_MAX) { p = save; return false; }
        if (simple && (p >= end || *p == ' ' || *p == '\t' || *p == '\n' || *p == '\r' || *p == 0)) {
            u = (int32_t)(a - 1); it = (int32_t)(b - 1); v = neg ? -val : val;
            return true;
        }
        p = s;
        SlowCopy c(p, end);
        char* e;
        double dv = strtod(c.buf, &e);
        if (e == c.buf || (size_t)(e - c.buf) == sizeof(c.buf) - 1) { p = save; return false; }     // (a token that fills the copy is no rating)
        p += e - c.buf;
        u = (int32_t)(a - 1); it = (int32_t)(b - 1); v = dv;
        return true;
    }
    p = save;                                           // signs / odd formats in the ids: the libc path
    SlowCopy c(p, end);
    char* e;
    const char* q = c.buf;
    long i = strtol(q, &e, 10);
    if (e == q) return false;
    q = e;
    long j = strtol(q, &e, 10);
    if (e == q) return false;
    q = e;
    double dv = strtod(q, &e);
    if (e == q || (size_t)(e - c.buf) == sizeof(c.buf) - 1) return false;
    p += e - c.buf;
    if (i < INT32_MIN + 1 || j < INT32_MIN + 1 || i > (long)INT32_MAX || j > (long)INT32_MAX) return false;
    u = (int32_t)(i - 1); it = (int32_t)(j - 1); v = dv;
    return true;
}

// "%d %d %lf" per entry, 1-based ids (util.h:126,131; util.h:367-368); exactly nnz entries are read.
// Parsed by `threads` host threads: the file is cut at line boundaries, the non-blank lines of every piece are counted
// (one vectorisable pass; a piece that contains a line ending in white space is recounted exactly), then every piece parses
// into its slice of the (uninitialised) output arrays.
static int64_t nonblank_lines(const char* base, size_t a, size_t b) {
    // fast count: newlines, + 1 for an unterminated last line; exact unless some newline follows white space or another
    // newline (blank lines, "\r\n", trailing blanks) -- `odd` counts those, and any of them sends the piece to the exact loop
    int64_t nl = 0, odd = 0;
    if (b > a) { nl = base[a] == '\n'; odd = nl; }                        // (a newline at the start of a piece: a blank line)
    for (size_t q0 = a + 1; q0 < b; q0 += 1 << 15) {                      // (blocks with 32-bit counters and no loop-carried state: vectorises)
        const size_t q1 = std::min(b, q0 + ((size_t)1 << 15));
        const unsigned char* s = reinterpret_cast<const unsigned char*>(base);
        unsigned bn = 0, bo = 0;
        for (size_t q = q0; q < q1; ++q) {
            const unsigned isnl = s[q] == '\n', pws = (s[q - 1] == '\n') | (s[q - 1] == ' ') | (s[q - 1] == '\t') | (s[q - 1] == '\r');
            bn += isnl;
            bo += isnl & pws;
        }
        nl += bn; odd += bo;
    }
    if (odd == 0) {
        // an unterminated last line counts only if it has content ("1 2 3\n  " holds one entry, not two)
        bool tail = false;
        for (size_t q = b; q > a && base[q - 1] != '\n' && !tail; --q) tail = base[q - 1] != ' ' && base[q - 1] != '\t' && base[q - 1] != '\r';
        return nl + (tail ? 1 : 0);
    }
    int64_t n = 0; bool content = false;
    for (size_t q = a; q < b; ++q) {
        if (base[q] == '\n') { n += content; content = false; }
        else if (base[q] != ' ' && base[q] != '\t' && base[q] != '\r') content = true;
    }
    return n + (content ? 1 : 0);
}

// a rating file opened, cut into pieces at line boundaries, the entries before every piece counted
struct ScannedFile {
    TextFile tf;
    int T = 1;
    std::vector<size_t> cut;
    std::vector<int64_t> first;                            // first[t] = entries before piece t; first[T] = entries of the file
};
static int scan_ratings(const std::string& path, int threads, ScannedFile& sf) {
    int rc = sf.tf.open(path);
    if (rc != PCR_OK) return rc;
    const char* base = sf.tf.p;
    const size_t len = sf.tf.len;
    int T = std::max(1, std::min(threads, 64));
    if (len < (size_t)1 << 20) T = 1;
    sf.T = T;
    sf.cut.assign((size_t)T + 1, len);
    sf.cut[0] = 0;
    for (int t = 1; t < T; ++t) {
        size_t c = std::max(sf.cut[t - 1], len * t / T);
        while (c < len && base[c] != '\n') ++c;
        sf.cut[t] = c < len ? c + 1 : len;
    }
    sf.first.assign((size_t)T + 1, 0);
    std::vector<int64_t> cnt(T, 0);
    run_pieces(T, T, [&](int, int64_t lo, int64_t hi) { for (int64_t t = lo; t < hi; ++t) cnt[t] = nonblank_lines(base, sf.cut[t], sf.cut[t + 1]); });
    for (int t = 0; t < T; ++t) sf.first[t + 1] = sf.first[t] + cnt[t];
    return PCR_OK;
}
// entries [0, n) of a scanned file into user / item / val (val may be null); returns the index of the first malformed entry, or -1
static int64_t parse_scanned(const ScannedFile& sf, int64_t n, int32_t* user, int32_t* item, double* val) {
    const int T = sf.T;
    const char* base = sf.tf.p;
    std::vector<int64_t> bad(T, -1);
    run_pieces(T, T, [&](int, int64_t lo, int64_t hi) {
        for (int64_t t = lo; t < hi; ++t) {
            const char* p = base + sf.cut[t];
            const char* end = base + sf.cut[t + 1];
            double dummy;
            for (int64_t z = sf.first[t]; z < sf.first[t + 1] && z < n; ++z)
                if (!parse_one(p, end, user[z], item[z], val ? val[z] : dummy)) { bad[t] = z; break; }
        }
    });
    for (int t = 0; t < T; ++t) if (bad[t] >= 0) return bad[t];
    return -1;
}

static int parse_ratings(const std::string& path, int64_t nnz, pcr_vec<int32_t>& user,
                         pcr_vec<int32_t>& item, pcr_vec<double>& val, int threads) {
    if (nnz < 0) { pcr_set_error(path + ": a negative rating count in meta"); return PCR_ERR_IO; }
    ScannedFile sf;
    int rc = scan_ratings(path, threads, sf);
    if (rc != PCR_OK) return rc;
    if (sf.first[sf.T] < nnz) {
        pcr_set_error(path + ": expected " + std::to_string(nnz) + " ratings, found " + std::to_string(sf.first[sf.T]));
        return PCR_ERR_IO;
    }
    user.resize((size_t)nnz); item.resize((size_t)nnz); val.resize((size_t)nnz);          // (only now: meta may promise any number)
    const int64_t bad = parse_scanned(sf, nnz, user.data(), item.data(), val.data());
    if (bad >= 0) { pcr_set_error(path + ": malformed rating line " + std::to_string(bad + 1)); return PCR_ERR_IO; }
    return PCR_OK;
}

// A rating file without a meta file beside it (pmf-predict.cpp:52-55 reads "user item rating" triples until fscanf fails):
// count = the file's non-blank lines; read = at most n entries by `threads` host threads, 0-based ids, ending at the first malformed
// entry (*n_read entries stand before it; the reference's `!= EOF` loop never ends there).
extern "C" int pcr_rating_file_count(const char* path, int64_t* n) {
    if (!path || !n) { pcr_set_error("pcr_rating_file_count: bad argument"); return PCR_ERR_ARG; }
    return guarded("pcr_rating_file_count", [&]() -> int {
        ScannedFile sf;
        int rc = scan_ratings(path, pcr_host_threads(), sf);
        if (rc != PCR_OK) return rc;
        *n = sf.first[sf.T];
        return PCR_OK;
    });
}
extern "C" int pcr_rating_file_read(const char* path, int threads, int64_t n, int32_t* user, int32_t* item, double* val, int64_t* n_read) {
    if (!path || n < 0 || !n_read || (n > 0 && (!user || !item))) { pcr_set_error("pcr_rating_file_read: bad argument"); return PCR_ERR_ARG; }
    if (threads <= 0) threads = pcr_host_threads();
    return guarded("pcr_rating_file_read", [&]() -> int {
        ScannedFile sf;
        int rc = scan_ratings(path, threads, sf);
        if (rc != PCR_OK) return rc;
        const int64_t m = std::min(n, sf.first[sf.T]);
        const int64_t bad = parse_scanned(sf, m, user, item, val);
        *n_read = bad >= 0 ? bad : m;
        return PCR_OK;
    });
}

extern "C" int pcr_dataset_load(const char* dir, pcr_dataset** out) { return pcr_dataset_load_mt(dir, 0, out); }

extern "C" int pcr_dataset_load_mt(const char* dir, int threads, pcr_dataset** out) {
    if (!dir || !out) { pcr_set_error("pcr_dataset_load: bad argument"); return PCR_ERR_ARG; }
    if (threads <= 0) threads = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    std::string d(dir);
    std::string metap = d + "/meta";
    FILE* fp = fopen(metap.c_str(), "r");
    if (!fp) { pcr_set_error("can't open " + metap + ": " + strerror(errno)); return PCR_ERR_IO; }
    long m = 0, n = 0, nnz = 0, tnnz = 0;
    char name[1024], tname[1024];
    bool have_test = false;
    if (fscanf(fp, "%ld %ld", &m, &n) != 2 || fscanf(fp, "%ld %1023s", &nnz, name) != 2) {
        fclose(fp);
        pcr_set_error(metap + ": expected 'm n' then 'nnz training_file'");
        return PCR_ERR_IO;
    }
    if (fscanf(fp, "%ld %1023s", &tnnz, tname) == 2) have_test = true;   // third line optional (util.cpp:18)
    fclose(fp);
    if (m < 0 || n < 0 || m > kMaxDim || n > kMaxDim) { pcr_set_error(metap + ": user / item counts must lie in [0, 2^31 - 2]"); return PCR_ERR_IO; }
    return guarded("pcr_dataset_load", [&]() -> int {
        // item / value arrays are parsed straight into the data set's CSR storage: for a file ordered by (user, item) they are
        // the CSR as they stand (build_train_csr adopts them)
        std::unique_ptr<pcr_dataset> ds(new pcr_dataset());
        pcr_vec<int32_t> u, tu;
        int rc = parse_ratings(d + "/" + name, nnz, u, ds->train.item, ds->train.val, threads);
        if (rc != PCR_OK) return rc;
        rc = build_train_csr(m, n, nnz, u.data(), ds->train.item.data(), ds->train.val.data(), ds->train, threads, true);
        if (rc != PCR_OK) return rc;
        pcr_vec<int32_t>().swap(u);
        if (have_test) {
            rc = parse_ratings(d + "/" + tname, tnnz, tu, ds->test.item, ds->test.val, threads);
            if (rc != PCR_OK) return rc;
            rc = check_test_ids(n, tnnz, tu.data(), ds->test.item.data(), threads);
            if (rc != PCR_OK) return rc;
            keep_raw_test(*ds, m, tnnz, tu.data(), ds->test.item.data(), ds->test.val.data());
        } else {
            tnnz = 0;
        }
        build_test_csr(m, n, tnnz, tu.data(), ds->test.item.data(), ds->test.val.data(), ds->test, threads, true);
        ds->tnnz_file = tnnz;
        *out = ds.release();
        return PCR_OK;
    });
}

// ---- binary side-car cache of the converted data set
namespace {
struct CacheHeader {
    char magic[8];                 // "PCRCACH2"
    int64_t d1, d2, nnz, tnnz, tnnz_file;
    int64_t traw;                  // raw test triplets kept (pcr_dataset::traw_*), 0 for a user-sorted test file
    int64_t stamp[6];              // size, mtime (ns) of meta, training file, test file at the time of the parse (0: not recorded)
};
const char kCacheMagic[8] = {'P', 'C', 'R', 'C', 'A', 'C', 'H', '2'};

bool file_stamp(const std::string& p, int64_t* size, int64_t* mtime) {
    struct stat sb;
    if (stat(p.c_str(), &sb) != 0) return false;
    *size = (int64_t)sb.st_size;
    *mtime = (int64_t)sb.st_mtim.tv_sec * 1000000000LL + (int64_t)sb.st_mtim.tv_nsec;
    return true;
}
// stamps of <dir>/meta and the rating files it names; false if meta is unreadable
bool dir_stamps(const std::string& d, int64_t stamp[6]) {
    for (int i = 0; i < 6; ++i) stamp[i] = 0;
    FILE* fp = fopen((d + "/meta").c_str(), "r");
    if (!fp) return false;
    long m = 0, n = 0, nnz = 0, tnnz = 0;
    char name[1024], tname[1024];
    const bool ok = fscanf(fp, "%ld %ld", &m, &n) == 2 && fscanf(fp, "%ld %1023s", &nnz, name) == 2;
    const bool have_test = ok && fscanf(fp, "%ld %1023s", &tnnz, tname) == 2;
    fclose(fp);
    if (!ok || !file_stamp(d + "/meta", &stamp[0], &stamp[1]) || !file_stamp(d + "/" + name, &stamp[2], &stamp[3])) return false;
    if (have_test && !file_stamp(d + "/" + tname, &stamp[4], &stamp[5])) return false;
    return true;
}

// n bytes between a file and memory by the host threads: pread / pwrite of disjoint pieces (both are thread-safe on one descriptor)
bool par_io(int fd, off_t off, void* mem, size_t n, bool write, int threads) {
    const int T = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::min(threads, 64), n / ((size_t)8 << 20) + 1));
    std::vector<char> ok((size_t)T, 1);
    run_pieces((int64_t)n, T, [&](int t, int64_t lo, int64_t hi) {
        char* p = static_cast<char*>(mem);
        while (lo < hi) {
            const ssize_t g = write ? pwrite(fd, p + lo, (size_t)(hi - lo), off + lo) : pread(fd, p + lo, (size_t)(hi - lo), off + lo);
            if (g < 0 && errno == EINTR) continue;
            if (g <= 0) { ok[(size_t)t] = 0; return; }
            lo += g;
        }
    });
    for (char c : ok) if (!c) return false;
    return true;
}

// Layout: header | train.index | train.item | train.val | test.index | test.item | test.val | traw_user | traw_item | traw_val.  Written and read by the host
// threads in disjoint pieces (a 1.2 GB cache through one fread / fwrite was SLOWER than parsing the text it caches).
int save_cache(const pcr_dataset* ds, const char* path, const int64_t stamp[6]) {
    if (!ds || !path) { pcr_set_error("pcr_dataset_save_cache: bad argument"); return PCR_ERR_ARG; }
    const std::string tmp = std::string(path) + ".tmp";
    const int fd = ::open(tmp.c_str(), O_CREAT | O_TRUNC | O_WRONLY | O_CLOEXEC, 0644);
    if (fd < 0) { pcr_set_error("can't open " + tmp + ": " + strerror(errno)); return PCR_ERR_IO; }
    CacheHeader h;
    memcpy(h.magic, kCacheMagic, 8);
    h.d1 = ds->train.d1; h.d2 = ds->train.d2; h.nnz = ds->train.nnz(); h.tnnz = ds->test.nnz(); h.tnnz_file = ds->tnnz_file;
    h.traw = (int64_t)ds->traw_val.size();
    for (int i = 0; i < 6; ++i) h.stamp[i] = stamp ? stamp[i] : 0;
    const int threads = pcr_host_threads();
    off_t off = 0;
    bool ok = par_io(fd, off, &h, sizeof(h), true, 1);
    off += sizeof(h);
    auto put = [&](const void* p, size_t bytes) { if (ok && bytes) ok = par_io(fd, off, const_cast<void*>(p), bytes, true, threads); off += (off_t)bytes; };
    put(ds->train.index.data(), ds->train.index.size() * 8); put(ds->train.item.data(), ds->train.item.size() * 4); put(ds->train.val.data(), ds->train.val.size() * 8);
    put(ds->test.index.data(), ds->test.index.size() * 8); put(ds->test.item.data(), ds->test.item.size() * 4); put(ds->test.val.data(), ds->test.val.size() * 8);
    put(ds->traw_user.data(), ds->traw_user.size() * 4); put(ds->traw_item.data(), ds->traw_item.size() * 4); put(ds->traw_val.data(), ds->traw_val.size() * 8);
    ok = (::close(fd) == 0) && ok;
    if (!ok || rename(tmp.c_str(), path) != 0) { remove(tmp.c_str()); pcr_set_error(std::string("can't write ") + path); return PCR_ERR_IO; }
    return PCR_OK;
}
int load_cache(const char* path, const int64_t want[6], pcr_dataset** out) {
    const int fd = ::open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) { pcr_set_error(std::string("can't open ") + path + ": " + strerror(errno)); return PCR_ERR_IO; }
    struct Closer { int fd; ~Closer() { ::close(fd); } } closer{fd};
    CacheHeader h;
    auto fail = [&](const char* why) { pcr_set_error(std::string(path) + ": " + why); return PCR_ERR_IO; };
    struct stat sb;
    if (fstat(fd, &sb) != 0 || (size_t)sb.st_size < sizeof(h) || !par_io(fd, 0, &h, sizeof(h), false, 1) || memcmp(h.magic, kCacheMagic, 8) != 0)
        return fail("not a data set cache of this version");
    if (h.d1 < 0 || h.d2 < 0 || h.nnz < 0 || h.tnnz < 0 || h.traw < 0 || h.d1 > kMaxDim || h.d2 > kMaxDim) return fail("corrupt header");
    {   // the header must describe exactly this file before anything is allocated from it
        const __int128 want_bytes = (__int128)sizeof(h) + 2 * (__int128)(h.d1 + 1) * 8 + (__int128)(h.nnz + h.tnnz) * 12 + (__int128)h.traw * 16;
        if ((__int128)sb.st_size != want_bytes) return fail("truncated or corrupt (size does not match the header)");
    }
    if (want) for (int i = 0; i < 6; ++i) if (h.stamp[i] != want[i]) return fail("stale (the text files changed)");
    const int threads = pcr_host_threads();
    std::unique_ptr<pcr_dataset> ds(new pcr_dataset);
    ds->train.d1 = ds->test.d1 = h.d1; ds->train.d2 = ds->test.d2 = h.d2; ds->tnnz_file = h.tnnz_file;
    ds->train.index.resize((size_t)h.d1 + 1); ds->train.item.resize((size_t)h.nnz); ds->train.val.resize((size_t)h.nnz);
    ds->test.index.resize((size_t)h.d1 + 1); ds->test.item.resize((size_t)h.tnnz); ds->test.val.resize((size_t)h.tnnz);
    off_t off = sizeof(h);
    bool ok = true;
    auto get = [&](void* p, size_t bytes) { if (ok && bytes) ok = par_io(fd, off, p, bytes, false, threads); off += (off_t)bytes; };
    get(ds->train.index.data(), ds->train.index.size() * 8); get(ds->train.item.data(), ds->train.item.size() * 4); get(ds->train.val.data(), ds->train.val.size() * 8);
    get(ds->test.index.data(), ds->test.index.size() * 8); get(ds->test.item.data(), ds->test.item.size() * 4); get(ds->test.val.data(), ds->test.val.size() * 8);
    ds->traw_user.resize((size_t)h.traw); ds->traw_item.resize((size_t)h.traw); ds->traw_val.resize((size_t)h.traw);
    get(ds->traw_user.data(), ds->traw_user.size() * 4); get(ds->traw_item.data(), ds->traw_item.size() * 4); get(ds->traw_val.data(), ds->traw_val.size() * 8);
    if (!ok) return fail("truncated");
    for (int64_t z = 0; z < h.traw; ++z)
        if (ds->traw_user[(size_t)z] < 0 || ds->traw_item[(size_t)z] < 0 || ds->traw_item[(size_t)z] >= h.d2) return fail("raw test id out of range");
    const std::vector<int64_t>&ti = ds->train.index, &xi = ds->test.index;
    if (ti.front() != 0 || ti.back() != h.nnz || xi.front() != 0 || xi.back() != h.tnnz) return fail("corrupt row pointers");
    // consistency of everything an index will be taken from, user ranges side by side: 0 = fine, else the first kind of damage
    const int T = pieces_for(h.nnz + h.d1, threads);
    std::vector<int> bad((size_t)T, 0);
    run_pieces(h.d1, T, [&](int t, int64_t lo, int64_t hi) {
        for (int64_t u = lo; u < hi; ++u) {
            if (ti[u + 1] < ti[u] || xi[u + 1] < xi[u] || ti[u + 1] > h.nnz || xi[u + 1] > h.tnnz || ti[u] < 0 || xi[u] < 0) { bad[(size_t)t] = 1; return; }
            for (int64_t z = ti[u]; z < ti[u + 1]; ++z) {
                const int32_t j = ds->train.item[(size_t)z];
                if (j < 0 || j >= h.d2) { bad[(size_t)t] = 2; return; }
                if (z > ti[u] && j <= ds->train.item[(size_t)z - 1]) { bad[(size_t)t] = 3; return; }
            }
            for (int64_t z = xi[u]; z < xi[u + 1]; ++z)
                if (ds->test.item[(size_t)z] < 0 || ds->test.item[(size_t)z] >= h.d2) { bad[(size_t)t] = 2; return; }
        }
    });
    for (int b : bad)
        if (b) return fail(b == 1 ? "corrupt row pointers" : b == 2 ? "item id out of range" : "items of a user not ascending");
    *out = ds.release();
    return PCR_OK;
}
}  // namespace

extern "C" int pcr_dataset_save_cache(const pcr_dataset* ds, const char* path) { return save_cache(ds, path, nullptr); }
extern "C" int pcr_dataset_load_cache(const char* path, pcr_dataset** out) {
    if (!path || !out) { pcr_set_error("pcr_dataset_load_cache: bad argument"); return PCR_ERR_ARG; }
    return guarded("pcr_dataset_load_cache", [&]() -> int { return load_cache(path, nullptr, out); });
}
extern "C" int pcr_dataset_load_cached(const char* dir, int threads, const char* cache, pcr_dataset** out) {
    if (!dir || !cache || !out) { pcr_set_error("pcr_dataset_load_cached: bad argument"); return PCR_ERR_ARG; }
    int64_t stamp[6];
    const bool have = dir_stamps(dir, stamp);
    if (have && guarded("pcr_dataset_load_cached", [&]() -> int { return load_cache(cache, stamp, out); }) == PCR_OK) return PCR_OK;
    int rc = pcr_dataset_load_mt(dir, threads, out);
    if (rc != PCR_OK) return rc;
    if (have) (void)save_cache(*out, cache, stamp);      // best effort: a read-only data directory is not an error
    return PCR_OK;
}

extern "C" void pcr_dataset_free(pcr_dataset* ds) { delete ds; }

extern "C" int pcr_dataset_dims(const pcr_dataset* ds, int64_t* d1, int64_t* d2, int64_t* nnz, int64_t* tnnz) {
    if (!ds) { pcr_set_error("null dataset"); return PCR_ERR_ARG; }
    if (d1) *d1 = ds->train.d1;
    if (d2) *d2 = ds->train.d2;
    if (nnz) *nnz = ds->train.nnz();
    if (tnnz) *tnnz = ds->test.nnz();
    return PCR_OK;
}

extern "C" int pcr_dataset_csr(const pcr_dataset* ds, int which, int64_t* index, int64_t* item, double* val) {
    if (!ds || (which != 0 && which != 1)) { pcr_set_error("pcr_dataset_csr: bad argument"); return PCR_ERR_ARG; }
    const PcrCsr& X = which == 0 ? ds->train : ds->test;
    if (index) std::copy(X.index.begin(), X.index.end(), index);
    if (item) for (size_t z = 0; z < X.item.size(); ++z) item[z] = X.item[z];
    if (val) std::copy(X.val.begin(), X.val.end(), val);
    return PCR_OK;
}

// ------------------------------------------------------------------------------------------
// levels
// ------------------------------------------------------------------------------------------

// run fn(t, lo, hi) for nthreads contiguous pieces of [0, n) (host set-up work: levels, tile-major CSC)
void pcr_parallel_ranges(int64_t n, int nthreads, const std::function<void(int, int64_t, int64_t)>& fn) {
    nthreads = (int)std::max<int64_t>(1, std::min<int64_t>(nthreads, n / 4096 + 1));
    if (nthreads == 1) { fn(0, 0, n); return; }
    run_workers(nthreads, [&](int t) { fn(t, n * t / nthreads, n * (t + 1) / nthreads); });
}
// fn(task) for task = 0 .. ntasks - 1, handed out one by one to nthreads workers (uneven tasks); exceptions are carried back
void pcr_parallel_tasks(int ntasks, int nthreads, const std::function<void(int)>& fn) {
    std::atomic<int> next{0};
    run_workers(std::max(1, std::min(nthreads, ntasks)), [&](int) { for (;;) { const int t = next.fetch_add(1); if (t >= ntasks) break; fn(t); } });
}
int pcr_host_threads() {
    // (the cgroup quota of a container is not visible through hardware_concurrency: cap at 16, the loader's default too)
    return (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
}

// Three passes, the outer two over user ranges in parallel: (1) per user the sorted distinct keys and each rating's level;
// (2) prefix sums of the per-user level counts; (3) the cumulative per-level counts and the level keys.
// Pass 1 per user: rating sets have a handful of integer levels, so when the rounded keys of a user span fewer than 64 integers
// (and, for PrimalCR's raw keys, every rating IS an integer) the level of a rating is a popcount in a 64-bit presence mask -- two
// streaming passes over the ratings, no searching; otherwise insertion into a small sorted vector (<= 64 distinct values), else
// sort + unique.
// lround() without the libm call: truncate, then step away from zero when the (exactly representable) remainder is at least a half
static inline long fast_lround(double v) {
    if (!(v > -4.0e15 && v < 4.0e15)) return lround(v);
    const long t = (long)v;
    const double f = v - (double)t;
    return f >= 0.5 ? t + 1 : f <= -0.5 ? t - 1 : t;
}

int pcr_build_levels(const PcrCsr& X, int64_t u0, int64_t u1, int solver_type, PcrLevels& out, std::string& err) {
    const int64_t z0 = X.index[u0], z1 = X.index[u1], nu = u1 - u0;
    out.level.resize((size_t)(z1 - z0));
    out.run_ofs.assign((size_t)(nu + 1), 0);
    out.run_start.clear();
    out.lev_val.clear();
    out.max_levels = 0;
    const int nth = pcr_host_threads();
    std::vector<int64_t> bad(nth, -1);
    std::vector<int> maxlev(nth, 0);
    std::vector<char> allint(nth, 1);
    const bool pp = solver_type == PCR_SOLVER_PCRPP;
    // per user: the presence mask + its base (fast path) or nothing (mask 0: general path, redone in pass 3 for the keys)
    std::vector<uint64_t> umask((size_t)nu, 0);
    std::vector<int64_t> ubase((size_t)nu, 0);
    const double* val = X.val.data();
    pcr_parallel_ranges(nu, nth, [&](int t, int64_t lo, int64_t hi) {
        std::vector<double> uniq, keys;
        std::vector<long> ikey;
        for (int64_t ui = lo; ui < hi; ++ui) {
            const int64_t a = X.index[u0 + ui], b = X.index[u0 + ui + 1];
            if (b == a) { out.run_ofs[ui + 1] = 1; continue; }
            long kmin = LONG_MAX, kmax = LONG_MIN;
            bool ints = true;
            ikey.resize((size_t)(b - a));                          // the rounded keys once (the user's ratings stay in cache)
            for (int64_t z = a; z < b; ++z) {
                const double v = val[z];
                const long k = fast_lround(v);
                ikey[(size_t)(z - a)] = k;
                kmin = std::min(kmin, k); kmax = std::max(kmax, k);
                ints = ints && (double)k == v;
            }
            if (!ints) allint[t] = 0;
            if ((pp || ints) && kmax - kmin < 64 && kmin > LONG_MIN / 2 && kmax < LONG_MAX / 2) {
                uint64_t m = 0;
                for (int64_t z = a; z < b; ++z) m |= (uint64_t)1 << (ikey[(size_t)(z - a)] - kmin);
                for (int64_t z = a; z < b; ++z) {
                    const int sh = (int)(ikey[(size_t)(z - a)] - kmin);
                    out.level[z - z0] = (uint16_t)__builtin_popcountll(m & (((uint64_t)1 << sh) - 1));
                }
                const int T = __builtin_popcountll(m);
                umask[ui] = m; ubase[ui] = kmin;
                maxlev[t] = std::max(maxlev[t], T);
                out.run_ofs[ui + 1] = T + 1;
                continue;
            }
            uniq.clear();
            bool small = true;
            for (int64_t z = a; z < b && small; ++z) {
                const double k = pp ? (double)fast_lround(val[z]) : val[z];
                auto it = std::lower_bound(uniq.begin(), uniq.end(), k);
                if (it == uniq.end() || *it != k) { if (uniq.size() >= 64) small = false; else uniq.insert(it, k); }
            }
            if (!small) {
                keys.resize((size_t)(b - a));
                for (int64_t z = a; z < b; ++z) keys[z - a] = pp ? (double)fast_lround(val[z]) : val[z];
                uniq = keys;
                std::sort(uniq.begin(), uniq.end());
                uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
            }
            const int T = (int)uniq.size();
            if (T > 65535) { if (bad[t] < 0) bad[t] = u0 + ui; continue; }
            maxlev[t] = std::max(maxlev[t], T);
            out.run_ofs[ui + 1] = T + 1;
            for (int64_t z = a; z < b; ++z) {
                const double k = pp ? (double)fast_lround(val[z]) : val[z];
                out.level[z - z0] = (uint16_t)(std::lower_bound(uniq.begin(), uniq.end(), k) - uniq.begin());
            }
        }
    });
    out.integer_valued = true;
    for (int t = 0; t < nth; ++t) {
        if (bad[t] >= 0) { err = "user " + std::to_string(bad[t]) + " has more than 65535 distinct rating levels"; return PCR_ERR_UNSUPPORTED; }
        out.max_levels = std::max(out.max_levels, maxlev[t]);
        out.integer_valued = out.integer_valued && allint[t];
    }
    for (int64_t ui = 0; ui < nu; ++ui) out.run_ofs[ui + 1] += out.run_ofs[ui];
    out.run_start.assign((size_t)out.run_ofs[nu], 0);
    out.lev_val.assign((size_t)out.run_ofs[nu], 0.0);
    pcr_parallel_ranges(nu, nth, [&](int, int64_t lo, int64_t hi) {
        for (int64_t ui = lo; ui < hi; ++ui) {
            const int64_t a = X.index[u0 + ui], b = X.index[u0 + ui + 1];
            int32_t* rs = out.run_start.data() + out.run_ofs[ui];
            double* lvv = out.lev_val.data() + out.run_ofs[ui];
            const int T = (int)(out.run_ofs[ui + 1] - out.run_ofs[ui]) - 1;
            for (int64_t z = a; z < b; ++z) rs[out.level[z - z0] + 1]++;
            for (int l = 0; l < T; ++l) rs[l + 1] += rs[l];
            if (umask[ui]) {
                int l = 0;
                for (uint64_t m = umask[ui]; m; m &= m - 1) lvv[l++] = (double)(ubase[ui] + __builtin_ctzll(m));
            } else {
                for (int64_t z = a; z < b; ++z) lvv[out.level[z - z0]] = pp ? (double)fast_lround(val[z]) : val[z];
            }
        }
    });
    return PCR_OK;
}

// |Omega_u| per user under the solver's level bucketing: the pairs of ratings at different levels
static int pcr_user_pairs(const pcr_dataset* ds, int solver_type, std::vector<int64_t>& pairs) {
    const PcrCsr& X = ds->train;
    PcrLevels lv;
    std::string err;
    const int rc = pcr_build_levels(X, 0, X.d1, solver_type, lv, err);
    if (rc != PCR_OK) { pcr_set_error(err); return rc; }
    pairs.assign((size_t)X.d1, 0);
    for (int64_t u = 0; u < X.d1; ++u) {
        int64_t n = X.index[u + 1] - X.index[u], same = 0;
        for (int64_t q = lv.run_ofs[u]; q + 1 < lv.run_ofs[u + 1]; ++q) {
            int64_t c = lv.run_start[q + 1] - lv.run_start[q];
            same += c * c;
        }
        pairs[(size_t)u] = (n * n - same) / 2;
    }
    return PCR_OK;
}

extern "C" int64_t pcr_dataset_count_pairs(const pcr_dataset* ds, int solver_type) {
    if (!ds) return -1;
    std::vector<int64_t> pairs;
    if (pcr_user_pairs(ds, solver_type, pairs) != PCR_OK) return -1;
    int64_t total = 0;
    for (int64_t c : pairs) total += c;
    return total;
}

extern "C" int pcr_dataset_user_pairs(const pcr_dataset* ds, int solver_type, int64_t* pairs) {
    if (!ds || (!pairs && ds->train.d1 > 0)) { pcr_set_error("pcr_dataset_user_pairs: bad argument"); return PCR_ERR_ARG; }
    if (solver_type != PCR_SOLVER_PCR && solver_type != PCR_SOLVER_PCRPP) { pcr_set_error("pcr_dataset_user_pairs: solver type must be 1 (PrimalCR) or 2 (PrimalCR++)"); return PCR_ERR_ARG; }
    std::vector<int64_t> v;
    const int rc = pcr_user_pairs(ds, solver_type, v);
    if (rc != PCR_OK) return rc;
    std::copy(v.begin(), v.end(), pairs);
    return PCR_OK;
}

// per-user loss weights by scheme (primalcr.h): both normalising schemes keep the unweighted problem's total mass
extern "C" int pcr_user_weights(const pcr_dataset* ds, int solver_type, int scheme, double* w) {
    if (!ds || (!w && ds->train.d1 > 0)) { pcr_set_error("pcr_user_weights: bad argument"); return PCR_ERR_ARG; }
    if (solver_type != PCR_SOLVER_PCR && solver_type != PCR_SOLVER_PCRPP) { pcr_set_error("pcr_user_weights: solver type must be 1 (PrimalCR) or 2 (PrimalCR++)"); return PCR_ERR_ARG; }
    if (scheme != PCR_WEIGHT_UNIFORM && scheme != PCR_WEIGHT_PAIRS && scheme != PCR_WEIGHT_RATINGS) {
        pcr_set_error("pcr_user_weights: unknown scheme " + std::to_string(scheme) + " (0 = uniform, 1 = pairs, 2 = ratings)");
        return PCR_ERR_ARG;
    }
    const PcrCsr& X = ds->train;
    std::vector<int64_t> cnt((size_t)X.d1, 0);               // the user's mass: |Omega_u| or n_u
    if (scheme == PCR_WEIGHT_PAIRS) { const int rc = pcr_user_pairs(ds, solver_type, cnt); if (rc != PCR_OK) return rc; }
    else if (scheme == PCR_WEIGHT_RATINGS) for (int64_t u = 0; u < X.d1; ++u) cnt[(size_t)u] = X.index[u + 1] - X.index[u];
    int64_t total = 0, active = 0;
    for (int64_t c : cnt) { total += c; active += c > 0 ? 1 : 0; }
    const double mean = active > 0 ? (double)total / (double)active : 1.0;
    for (int64_t u = 0; u < X.d1; ++u) w[u] = cnt[(size_t)u] > 0 ? mean / (double)cnt[(size_t)u] : 1.0;
    return PCR_OK;
}

// per-rating weights for CCDR1 (primalcr.h): (user, item, weight) triplets into the training CSR's order.  A user's items
// ascend, so a triplet finds its rating by binary search.
extern "C" int pcr_dataset_match_weights(const pcr_dataset* ds, int64_t n, const int32_t* user, const int32_t* item, const double* w, double* w_csr) {
    if (!ds || n < 0 || (n > 0 && (!user || !item || !w)) || (!w_csr && ds->train.nnz() > 0)) {
        pcr_set_error("pcr_dataset_match_weights: bad argument");
        return PCR_ERR_ARG;
    }
    const PcrCsr& X = ds->train;
    const int64_t nnz = X.nnz();
    std::vector<char> seen((size_t)nnz, 0);
    for (int64_t q = 0; q < n; ++q) {
        const int64_t u = user[q], j = item[q];
        const std::string who = "triplet " + std::to_string(q) + " (user " + std::to_string(u) + ", item " + std::to_string(j) + ")";
        int64_t z = -1;
        if (u >= 0 && u < X.d1 && j >= 0 && j < X.d2) {
            const int32_t* lo = X.item.data() + X.index[(size_t)u];
            const int32_t* hi = X.item.data() + X.index[(size_t)u + 1];
            const int32_t* at = std::lower_bound(lo, hi, (int32_t)j);
            if (at != hi && *at == (int32_t)j) z = at - X.item.data();
        }
        if (z < 0) { pcr_set_error("pcr_dataset_match_weights: " + who + " is not a training rating"); return PCR_ERR_ARG; }
        if (seen[(size_t)z]) { pcr_set_error("pcr_dataset_match_weights: " + who + " names a training rating a second time"); return PCR_ERR_ARG; }
        seen[(size_t)z] = 1;
        w_csr[z] = w[q];
    }
    if (n < nnz) {
        for (int64_t u = 0; u < X.d1; ++u)
            for (int64_t z = X.index[(size_t)u]; z < X.index[(size_t)u + 1]; ++z)
                if (!seen[(size_t)z]) {
                    pcr_set_error("pcr_dataset_match_weights: the training rating (user " + std::to_string(u) + ", item " +
                                  std::to_string(X.item[(size_t)z]) + ") is left without a weight");
                    return PCR_ERR_ARG;
                }
    }
    return PCR_OK;
}

// w_z = (n_max / n_item(z))^gamma: the inverse of a power-law propensity in the item's popularity; not normalised
extern "C" int pcr_rating_weights_popularity(const pcr_dataset* ds, double gamma, double* w_csr) {
    if (!ds || (!w_csr && ds->train.nnz() > 0)) { pcr_set_error("pcr_rating_weights_popularity: bad argument"); return PCR_ERR_ARG; }
    if (!std::isfinite(gamma)) { pcr_set_error("pcr_rating_weights_popularity: gamma must be a finite number"); return PCR_ERR_ARG; }
    const PcrCsr& X = ds->train;
    const int64_t nnz = X.nnz();
    std::vector<int64_t> cnt((size_t)X.d2, 0);
    for (int64_t z = 0; z < nnz; ++z) cnt[(size_t)X.item[(size_t)z]]++;
    int64_t nmax = 0;
    for (int64_t c : cnt) nmax = std::max(nmax, c);
    std::vector<double> wi((size_t)X.d2, 1.0);
    for (int64_t j = 0; j < X.d2; ++j)
        if (cnt[(size_t)j] > 0) wi[(size_t)j] = gamma == 0.0 ? 1.0 : std::pow((double)nmax / (double)cnt[(size_t)j], gamma);
    for (int64_t z = 0; z < nnz; ++z) w_csr[z] = wi[(size_t)X.item[(size_t)z]];
    return PCR_OK;
}

// ------------------------------------------------------------------------------------------
// model file (pmf-train.cpp:297-310, util.cpp:30-79)
// ------------------------------------------------------------------------------------------

extern "C" int pcr_model_save(const char* path, const double* U, int64_t d1, const double* V, int64_t d2, int64_t k) {
    FILE* fp = fopen(path, "wb");
    if (!fp) { pcr_set_error(std::string("can't open output file ") + path); return PCR_ERR_IO; }
    long hdr[2];
    bool ok = true;
    hdr[0] = (long)d1; hdr[1] = (long)k;
    ok &= fwrite(hdr, sizeof(long), 2, fp) == 2;
    ok &= fwrite(U, sizeof(double), (size_t)(d1 * k), fp) == (size_t)(d1 * k);
    hdr[0] = (long)d2; hdr[1] = (long)k;
    ok &= fwrite(hdr, sizeof(long), 2, fp) == 2;
    ok &= fwrite(V, sizeof(double), (size_t)(d2 * k), fp) == (size_t)(d2 * k);
    ok &= fclose(fp) == 0;
    if (!ok) { pcr_set_error(std::string("short write to ") + path); return PCR_ERR_IO; }
    return PCR_OK;
}

extern "C" int pcr_model_load(const char* path, int64_t* d1, int64_t* d2, int64_t* k, double* U, double* V) {
    FILE* fp = fopen(path, "rb");
    if (!fp) { pcr_set_error(std::string("can't open model file ") + path); return PCR_ERR_IO; }
    long hdr[2];
    int rc = PCR_OK;
    struct stat sb;
    const bool have_size = fstat(fileno(fp), &sb) == 0;
    do {
        if (fread(hdr, sizeof(long), 2, fp) != 2 || hdr[0] < 0 || hdr[1] < 0) { rc = PCR_ERR_IO; break; }
        long m1 = hdr[0], kk = hdr[1];
        // (a corrupt header must not turn into a 2^60-element read or, in a caller that sizes its buffers from the query call, an
        // allocation of that size: the first matrix has to fit the file)
        if (!have_size || (__int128)m1 * kk * 8 + 32 > (__int128)sb.st_size) { rc = PCR_ERR_IO; break; }
        if (U) { if (fread(U, sizeof(double), (size_t)(m1 * kk), fp) != (size_t)(m1 * kk)) { rc = PCR_ERR_IO; break; } }
        else fseek(fp, (long)sizeof(double) * m1 * kk, SEEK_CUR);
        if (fread(hdr, sizeof(long), 2, fp) != 2 || hdr[1] != kk || hdr[0] < 0) { rc = PCR_ERR_IO; break; }
        long m2 = hdr[0];
        if ((__int128)(m1 + m2) * kk * 8 + 32 != (__int128)sb.st_size) { rc = PCR_ERR_IO; break; }
        if (V && fread(V, sizeof(double), (size_t)(m2 * kk), fp) != (size_t)(m2 * kk)) { rc = PCR_ERR_IO; break; }
        if (d1) *d1 = m1;
        if (d2) *d2 = m2;
        if (k) *k = kk;
    } while (0);
    fclose(fp);
    if (rc != PCR_OK) pcr_set_error(std::string("malformed model file ") + path);
    return rc;
}

// ------------------------------------------------------------------------------------------
// multi-GPU partition: contiguous user ranges balanced by nnz
// ------------------------------------------------------------------------------------------

extern "C" int pcr_partition_users(const int64_t* index, int64_t d1, int nparts, int64_t* bounds) {
    if (!index || !bounds || nparts < 1 || d1 < 0) { pcr_set_error("pcr_partition_users: bad argument"); return PCR_ERR_ARG; }
    int64_t nnz = index[d1];
    bounds[0] = 0;
    for (int p = 1; p < nparts; ++p) {
        // first user boundary whose prefix nnz reaches p/nparts of the total
        double target = (double)nnz * p / nparts;
        int64_t lo = bounds[p - 1], hi = d1;
        while (lo < hi) {
            int64_t mid = (lo + hi) / 2;
            if ((double)index[mid] < target) lo = mid + 1; else hi = mid;
        }
        if (nnz == 0) lo = d1 * p / nparts;
        bounds[p] = std::max(lo, bounds[p - 1]);
    }
    bounds[nparts] = d1;
    return PCR_OK;
}

int pcr_recommend_model_check(const double* U, int64_t d1, const double* V, int64_t d2, int64_t k, const int64_t* index,
                              const int32_t* item, int64_t n, const int32_t* users, int topk, int dtype, const int32_t* items,
                              const double* scores, bool* sorted, const char* who) {
    auto bad = [who](const std::string& why) { pcr_set_error(std::string(who) + ": " + why); return PCR_ERR_ARG; };
    if (sorted) *sorted = true;
    if (!U || !V || d1 < 1 || d2 < 1 || k < 1 || n < 0) return bad("bad argument");
    if (d2 >= ((int64_t)1 << 31) - 64) return bad("more than 2^31 items");
    if (topk < 1 || topk > PCR_RECOMMEND_MAX_K) return bad("K = " + std::to_string(topk) + " outside [1, " + std::to_string(PCR_RECOMMEND_MAX_K) + "]");
    if (dtype != PCR_F32 && dtype != PCR_F64) return bad("dtype must be PCR_F32 or PCR_F64");
    if (n > 0 && (!items || !scores)) return bad("null output");
    if ((index == nullptr) != (item == nullptr)) return bad("index and item go together");
    if (!users && n > d1) return bad("n > d1 without a user list");
    const int nth = pcr_host_threads();
    if (users) {
        std::vector<int64_t> first((size_t)nth, -1);
        pcr_parallel_ranges(n, nth, [&](int t, int64_t lo, int64_t hi) {
            for (int64_t z = lo; z < hi; ++z)
                if (users[z] < 0 || users[z] >= d1) { first[(size_t)t] = z; return; }
        });
        for (int64_t x : first) if (x >= 0) return bad("user " + std::to_string(users[x]) + " (entry " + std::to_string(x) + ") outside the model");
    }
    if (index) {
        if (index[0] != 0) return bad("index[0] must be 0");
        for (int64_t u = 0; u < d1; ++u) if (index[u + 1] < index[u]) return bad("index not monotone at user " + std::to_string(u));
        std::vector<int> st((size_t)nth, 0);   // bit 0: an item outside [0, d2); bit 1: a row that is not item-ascending
        pcr_parallel_ranges(d1, nth, [&](int t, int64_t lo, int64_t hi) {
            for (int64_t u = lo; u < hi; ++u)
                for (int64_t z = index[u]; z < index[u + 1]; ++z) {
                    if (item[z] < 0 || item[z] >= d2) { st[(size_t)t] |= 1; return; }
                    if (z > index[u] && item[z] < item[z - 1]) st[(size_t)t] |= 2;
                }
        });
        int all = 0;
        for (int x : st) all |= x;
        if (all & 1) return bad("an item id of the exclusion CSR is outside [0, d2)");
        if (sorted) *sorted = !(all & 2);
    }
    return PCR_OK;
}

int pcr_item_filter_check(const char* who, int64_t d2, int64_t n, const int32_t* users, const pcr_item_filter* f) {
    auto bad = [who](const std::string& why) { pcr_set_error(std::string(who) + ": " + why); return PCR_ERR_ARG; };
    if (!f) return bad("null filter (pcr_recommend is the entry without one)");
    if (!f->allow && !f->cand_ptr) return bad("a filter without an allow set and without candidate lists (pcr_recommend is the entry without one)");
    if (!f->cand_ptr) return PCR_OK;
    auto user_of = [&](int64_t i) { return "user " + std::to_string(users ? (int64_t)users[i] : i) + " (row " + std::to_string(i) + ")"; };
    const int64_t* cp = f->cand_ptr;
    if (cp[0] != 0) return bad("cand_ptr[0] must be 0");
    for (int64_t i = 0; i < n; ++i) if (cp[i + 1] < cp[i]) return bad("cand_ptr not monotone at " + user_of(i));
    if (!f->cand_item) return bad("cand_ptr without cand_item");
    const int nth = pcr_host_threads();
    std::vector<int64_t> first((size_t)nth, -1);       // the first bad row of each thread's range
    std::vector<int32_t> what((size_t)nth, 0);         // ... and its id; kind 0: outside [0, d2), 1: twice in the row
    std::vector<char> kind((size_t)nth, 0);
    pcr_parallel_ranges(n, nth, [&](int t, int64_t lo, int64_t hi) {
        std::vector<int32_t> row;
        for (int64_t i = lo; i < hi; ++i) {
            const int32_t* c = f->cand_item + cp[i];
            const int64_t len = cp[i + 1] - cp[i];
            for (int64_t z = 0; z < len; ++z)
                if (c[z] < 0 || c[z] >= d2) { first[(size_t)t] = i; what[(size_t)t] = c[z]; kind[(size_t)t] = 0; return; }
            row.assign(c, c + len);
            std::sort(row.begin(), row.end());
            for (int64_t z = 1; z < len; ++z)
                if (row[(size_t)z] == row[(size_t)z - 1]) { first[(size_t)t] = i; what[(size_t)t] = row[(size_t)z]; kind[(size_t)t] = 1; return; }
        }
    });
    for (int t = 0; t < nth; ++t) {
        if (first[(size_t)t] < 0) continue;
        const std::string id = "candidate id " + std::to_string(what[(size_t)t]);
        return bad(kind[(size_t)t] ? id + " twice in the row of " + user_of(first[(size_t)t])
                                   : id + " of " + user_of(first[(size_t)t]) + " outside [0, " + std::to_string(d2) + ")");
    }
    return PCR_OK;
}

int pcr_recommend_filtered_model_check(const double* U, int64_t d1, const double* V, int64_t d2, int64_t k, const int64_t* index,
                                       const int32_t* item, int64_t n, const int32_t* users, int topk, int dtype, const pcr_item_filter* f,
                                       const int32_t* items, const double* scores, bool* sorted) {
    const int rc = pcr_recommend_model_check(U, d1, V, d2, k, index, item, n, users, topk, dtype, items, scores, sorted, "pcr_recommend_filtered_model");
    return rc != PCR_OK ? rc : pcr_item_filter_check("pcr_recommend_filtered_model", d2, n, users, f);
}

int pcr_cutoffs_check(const char* who, int ncut, const int* cutoffs) {
    auto bad = [who](const std::string& why) { pcr_set_error(std::string(who) + ": " + why); return PCR_ERR_ARG; };
    if (ncut < 1 || ncut > PCR_TOPN_MAX_CUTOFFS || !cutoffs)
        return bad("ncut = " + std::to_string(ncut) + " outside [1, " + std::to_string(PCR_TOPN_MAX_CUTOFFS) + "] (or no cutoffs)");
    for (int c = 0; c < ncut; ++c) {
        if (cutoffs[c] < 1 || cutoffs[c] > PCR_RECOMMEND_MAX_K)
            return bad("cutoff " + std::to_string(cutoffs[c]) + " outside [1, " + std::to_string(PCR_RECOMMEND_MAX_K) + "]");
        if (c > 0 && cutoffs[c] <= cutoffs[c - 1]) return bad("cutoffs must be strictly ascending");
    }
    return PCR_OK;
}

int pcr_topn_check(const char* who, int ncut, const int* cutoffs, double threshold, const pcr_topn_stats* stats) {
    auto bad = [who](const std::string& why) { pcr_set_error(std::string(who) + ": " + why); return PCR_ERR_ARG; };
    const int rc = pcr_cutoffs_check(who, ncut, cutoffs);
    if (rc != PCR_OK) return rc;
    if (std::isnan(threshold)) return bad("threshold is NaN");
    if (!stats) return bad("null stats");
    return PCR_OK;
}

// the test CSR of a model entry: present, tindex[0] = 0, monotone, items inside [0, d2)
static int test_csr_check(const char* who, int64_t d1, int64_t d2, const int64_t* tindex, const int32_t* titem, const double* tval) {
    auto bad = [who](const std::string& why) { pcr_set_error(std::string(who) + ": " + why); return PCR_ERR_ARG; };
    if (!tindex || !titem || !tval) return bad("null test CSR");
    if (tindex[0] != 0) return bad("tindex[0] must be 0");
    for (int64_t u = 0; u < d1; ++u) if (tindex[u + 1] < tindex[u]) return bad("tindex not monotone at user " + std::to_string(u));
    const int nth = pcr_host_threads();
    std::vector<char> out_of_range((size_t)nth, 0);
    pcr_parallel_ranges(tindex[d1], nth, [&](int t, int64_t lo, int64_t hi) {
        for (int64_t z = lo; z < hi; ++z) if (titem[z] < 0 || titem[z] >= d2) { out_of_range[(size_t)t] = 1; return; }
    });
    for (char x : out_of_range) if (x) return bad("an item id of the test CSR is outside [0, d2)");
    return PCR_OK;
}

int pcr_evaluate_topn_model_check(const double* U, int64_t d1, const double* V, int64_t d2, int64_t k, const int64_t* index,
                                  const int32_t* item, const int64_t* tindex, const int32_t* titem, const double* tval, int ncut,
                                  const int* cutoffs, double threshold, int dtype, const pcr_topn_stats* stats, bool* sorted,
                                  const char* who) {
    int rc = pcr_topn_check(who, ncut, cutoffs, threshold, stats);
    if (rc != PCR_OK) return rc;
    rc = pcr_recommend_model_check(U, d1, V, d2, k, index, item, 0, nullptr, cutoffs[ncut - 1], dtype, nullptr, nullptr, sorted, who);
    if (rc != PCR_OK) return rc;
    return test_csr_check(who, d1, d2, tindex, titem, tval);
}

int pcr_evaluate_ranks_model_check(const double* U, int64_t d1, const double* V, int64_t d2, int64_t k, const int64_t* index,
                                   const int32_t* item, const int64_t* tindex, const int32_t* titem, const double* tval,
                                   double threshold, int dtype, const pcr_rank_stats* stats, bool* sorted, const char* who) {
    auto bad = [who](const std::string& why) { pcr_set_error(std::string(who) + ": " + why); return PCR_ERR_ARG; };
    if (std::isnan(threshold)) return bad("threshold is NaN");
    if (!stats) return bad("null stats");
    const int rc = pcr_recommend_model_check(U, d1, V, d2, k, index, item, 0, nullptr, 1, dtype, nullptr, nullptr, sorted, who);
    if (rc != PCR_OK) return rc;
    return test_csr_check(who, d1, d2, tindex, titem, tval);
}

void pcr_topn_relevance(int64_t rows, const int64_t* tptr, const int32_t* titem, const double* tval, double threshold, int ncut,
                        const int* cutoffs, PcrTopnRel& out) {
    const int K = cutoffs[ncut - 1];
    out.disc.resize((size_t)K);
    for (int i = 0; i < K; ++i) out.disc[(size_t)i] = 1.0 / log2((double)(i + 2));
    // contiguous user ranges per host thread, concatenated in order: the counted users stay ascending
    const int nth = pcr_host_threads();
    struct Part { std::vector<int32_t> users; std::vector<int64_t> len; std::vector<int32_t> item; std::vector<double> gain, idcg; };
    std::vector<Part> parts((size_t)nth);
    pcr_parallel_ranges(rows, nth, [&](int t, int64_t lo, int64_t hi) {
        Part& P = parts[(size_t)t];
        std::vector<std::pair<int32_t, double>> row;
        std::vector<double> g;
        for (int64_t u = lo; u < hi; ++u) {
            row.clear();
            for (int64_t z = tptr[u]; z < tptr[u + 1]; ++z) if (tval[z] >= threshold) row.emplace_back(titem[z], tval[z]);
            if (row.empty()) continue;
            std::sort(row.begin(), row.end());
            g.clear();
            for (size_t e = 0; e < row.size(); ++e) {
                if (e + 1 < row.size() && row[e + 1].first == row[e].first) continue;      // the largest rating of a duplicated item
                P.item.push_back(row[e].first);
                g.push_back(pow(2.0, row[e].second) - 1.0);
                P.gain.push_back(g.back());
            }
            P.users.push_back((int32_t)u);
            P.len.push_back((int64_t)g.size());
            std::sort(g.begin(), g.end(), [](double a, double b) { return a > b; });
            const int64_t nr = (int64_t)g.size();
            for (int c = 0; c < ncut; ++c) {
                const int64_t m = std::min<int64_t>(cutoffs[c], nr);
                double b = 0.0, w = 0.0;
                for (int64_t i = 0; i < m; ++i) { b += out.disc[(size_t)i]; w += g[(size_t)i] * out.disc[(size_t)i]; }
                P.idcg.push_back(b); P.idcg.push_back(w);
            }
        }
    });
    out.users.clear(); out.ritem.clear(); out.rgain.clear(); out.idcg.clear();
    out.rptr.assign(1, 0);
    for (const Part& P : parts) {
        out.users.insert(out.users.end(), P.users.begin(), P.users.end());
        for (int64_t l : P.len) out.rptr.push_back(out.rptr.back() + l);
        out.ritem.insert(out.ritem.end(), P.item.begin(), P.item.end());
        out.rgain.insert(out.rgain.end(), P.gain.begin(), P.gain.end());
        out.idcg.insert(out.idcg.end(), P.idcg.begin(), P.idcg.end());
    }
}

void pcr_topn_stats_from(const double* sums, int ncut, const int* cutoffs, pcr_topn_stats* stats) {
    const double users = sums[8 * ncut];
    auto mean = [](double s, double n) { return n > 0.0 ? s / n : 0.0; };
    for (int c = 0; c < ncut; ++c) {
        const double* x = sums + 8 * c;
        pcr_topn_stats& o = stats[c];
        o.cutoff = cutoffs[c];
        o.users = (int64_t)users;
        o.users_graded = (int64_t)x[7];
        o.hits = (int64_t)x[0];
        o.precision = mean(x[1], users);
        o.recall = mean(x[2], users);
        o.hit_rate = mean(x[3], users);
        o.map = mean(x[4], users);
        o.ndcg = mean(x[5], users);
        o.ndcg_graded = mean(x[6], x[7]);
    }
}

void pcr_rank_stats_from(const double* sums, pcr_rank_stats* stats) {
    const double users = sums[8];
    auto mean = [](double s, double n) { return n > 0.0 ? s / n : 0.0; };
    stats->users = (int64_t)users;
    stats->users_auc = (int64_t)sums[7];
    stats->relevant = (int64_t)sums[0];
    stats->mrr = mean(sums[1], users);
    stats->mean_rank = mean(sums[2], users);
    stats->auc = mean(sums[6], sums[7]);
    stats->mpr = mean(sums[4], users);
}

void pcr_rank_scatter(int64_t rows, const int64_t* tptr, const int32_t* titem, const double* tval, double threshold,
                      const PcrTopnRel& rel, const int64_t* rrank, int64_t* ranks) {
    std::fill(ranks, ranks + tptr[rows], (int64_t)0);
    pcr_parallel_ranges((int64_t)rel.users.size(), pcr_host_threads(), [&](int, int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; ++i) {
            const int64_t u = rel.users[(size_t)i];
            const int32_t* rb = rel.ritem.data() + rel.rptr[(size_t)i];
            const int32_t* re = rel.ritem.data() + rel.rptr[(size_t)i + 1];
            for (int64_t z = tptr[u]; z < tptr[u + 1]; ++z)
                if (tval[z] >= threshold) ranks[z] = rrank[std::lower_bound(rb, re, titem[z]) - rel.ritem.data()];
        }
    });
}

// ------------------------------------------------------------------------------ filtered evaluation (include/primalcr.h)
int pcr_eval_filter_check(const char* who, const char* unfiltered, int64_t d2, int64_t rows, const pcr_item_filter* f) {
    auto bad = [who](const std::string& why) { pcr_set_error(std::string(who) + ": " + why); return PCR_ERR_ARG; };
    if (!f) return bad(std::string("null filter (") + unfiltered + " is the entry without one)");
    if (!f->allow && !f->cand_ptr)
        return bad(std::string("a filter without an allow set and without candidate lists (") + unfiltered + " is the entry without one)");
    return pcr_item_filter_check(who, d2, rows, nullptr, f);
}

void pcr_filter_test_rows(int64_t rows, const int64_t* tptr, const int32_t* titem, const double* tval, const pcr_item_filter& f,
                          PcrFilteredTest& out) {
    const int nth = pcr_host_threads();
    std::vector<PcrFilteredTest> parts((size_t)nth);
    std::vector<int64_t> len((size_t)rows, 0);
    pcr_parallel_ranges(rows, nth, [&](int t, int64_t lo, int64_t hi) {
        PcrFilteredTest& P = parts[(size_t)t];
        std::vector<int32_t> row;
        for (int64_t u = lo; u < hi; ++u) {
            if (tptr[u + 1] == tptr[u]) continue;
            if (f.cand_ptr) {
                row.assign(f.cand_item + f.cand_ptr[u], f.cand_item + f.cand_ptr[u + 1]);
                std::sort(row.begin(), row.end());
            }
            for (int64_t z = tptr[u]; z < tptr[u + 1]; ++z) {
                const int32_t j = titem[z];
                if (f.allow && !f.allow[j]) continue;
                if (f.cand_ptr && !std::binary_search(row.begin(), row.end(), j)) continue;
                P.item.push_back(j); P.val.push_back(tval[z]); P.pos.push_back(z);
                ++len[(size_t)u];
            }
        }
    });
    out.ptr.assign((size_t)rows + 1, 0);
    for (int64_t u = 0; u < rows; ++u) out.ptr[(size_t)u + 1] = out.ptr[(size_t)u] + len[(size_t)u];
    out.item.clear(); out.val.clear(); out.pos.clear();
    for (const PcrFilteredTest& P : parts) {           // (contiguous user ranges, concatenated in order)
        out.item.insert(out.item.end(), P.item.begin(), P.item.end());
        out.val.insert(out.val.end(), P.val.begin(), P.val.end());
        out.pos.insert(out.pos.end(), P.pos.begin(), P.pos.end());
    }
}

static inline uint64_t sample_mix(uint64_t x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
    return x;
}
// The row of one user (include/primalcr.h, pcr_sample_negatives): its length, and with dst != NULL the row itself, ascending, at
// dst.  The length needs no draw -- min(n_neg, |P_u|) negatives and, with include_test, the distinct test items -- so a call that
// only sizes the rows samples nothing.  `ex`, `test` and `drawn` are scratch.
static int64_t sample_row(int64_t d2, const int32_t* tr, int64_t ntr, const int32_t* te, int64_t nte, uint64_t user, int64_t n_neg, uint64_t seed,
                          bool include_test, std::vector<int32_t>& ex, std::vector<int32_t>& test, std::vector<int32_t>& drawn, int32_t* dst) {
    if (nte == 0) return 0;
    test.assign(te, te + nte);
    std::sort(test.begin(), test.end());
    test.erase(std::unique(test.begin(), test.end()), test.end());
    ex.assign(tr, tr + ntr);
    ex.insert(ex.end(), test.begin(), test.end());
    std::sort(ex.begin(), ex.end());
    ex.erase(std::unique(ex.begin(), ex.end()), ex.end());          // the items outside the pool, ascending
    const int64_t pool = d2 - (int64_t)ex.size(), m = std::min(n_neg, pool);
    const int64_t len = m + (include_test ? (int64_t)test.size() : 0);
    if (!dst) return len;
    const bool whole = m == pool, keep = 2 * m <= pool;
    const int64_t want = whole ? 0 : keep ? m : pool - m;           // distinct draws inside the pool
    drawn.clear();
    const uint64_t golden = 0x9E3779B97F4A7C15ull, key = sample_mix(seed + golden * (user + 1));
    for (uint64_t t = 0; (int64_t)drawn.size() < want; ++t) {
        const int32_t j = (int32_t)(sample_mix(key + golden * (t + 1)) % (uint64_t)d2);
        if (std::binary_search(ex.begin(), ex.end(), j)) continue;
        const auto it = std::lower_bound(drawn.begin(), drawn.end(), j);
        if (it != drawn.end() && *it == j) continue;
        drawn.insert(it, j);
    }
    if (whole || !keep) {                                           // the pool, without the draws that are left out
        size_t e = 0, d = 0;
        for (int64_t j = 0; j < d2; ++j) {
            while (e < ex.size() && ex[e] < j) ++e;
            while (d < drawn.size() && drawn[d] < j) ++d;
            const bool is_ex = e < ex.size() && ex[e] == j, is_dr = d < drawn.size() && drawn[d] == j;
            if (!is_ex && !is_dr) *dst++ = (int32_t)j;
            else if (is_ex && include_test && std::binary_search(test.begin(), test.end(), (int32_t)j)) *dst++ = (int32_t)j;
        }
        return len;
    }
    if (include_test) std::merge(drawn.begin(), drawn.end(), test.begin(), test.end(), dst);
    else std::copy(drawn.begin(), drawn.end(), dst);
    return len;
}

extern "C" int pcr_sample_negatives(int64_t rows, int64_t d2, const int64_t* index, const int32_t* item, const int64_t* tindex,
                                    const int32_t* titem, int64_t first_user, int64_t n_neg, uint64_t seed, int include_test,
                                    int64_t* cand_ptr, int32_t* cand_item) {
    auto bad = [](const std::string& why) { pcr_set_error("pcr_sample_negatives: " + why); return PCR_ERR_ARG; };
    try {
        if (rows < 0 || d2 < 1 || first_user < 0 || n_neg < 0 || !cand_ptr) return bad("bad argument");
        if (d2 >= ((int64_t)1 << 31) - 64) return bad("more than 2^31 items");
        if ((index == nullptr) != (item == nullptr)) return bad("index and item go together");
        if (!tindex || (tindex[rows] > 0 && !titem)) return bad("null test CSR");
        if (tindex[0] != 0 || (index && index[0] != 0)) return bad("index[0] and tindex[0] must be 0");
        for (int64_t u = 0; u < rows; ++u) {
            if (tindex[u + 1] < tindex[u]) return bad("tindex not monotone at row " + std::to_string(u));
            if (index && index[u + 1] < index[u]) return bad("index not monotone at row " + std::to_string(u));
        }
        for (int64_t z = 0; z < tindex[rows]; ++z) if (titem[z] < 0 || titem[z] >= d2) return bad("an item id of the test CSR is outside [0, d2)");
        if (index) for (int64_t z = 0; z < index[rows]; ++z) if (item[z] < 0 || item[z] >= d2) return bad("an item id of the training CSR is outside [0, d2)");
        const int knob = pcr_tune_int("sample_threads", 0), nth = knob > 0 ? knob : pcr_host_threads();
        // a row is a function of its own user alone.  Pass 1 sizes the rows without a draw and makes the pointer; pass 2 (with
        // cand_item) writes each row where the pointer puts it
        auto pass = [&](int32_t* out) {
            pcr_parallel_ranges(rows, nth, [&](int, int64_t lo, int64_t hi) {
                std::vector<int32_t> ex, test, drawn;
                for (int64_t u = lo; u < hi; ++u) {
                    const int64_t len = sample_row(d2, index ? item + index[u] : nullptr, index ? index[u + 1] - index[u] : 0, titem + tindex[u],
                                                   tindex[u + 1] - tindex[u], (uint64_t)(first_user + u), n_neg, seed, include_test != 0, ex, test,
                                                   drawn, out ? out + cand_ptr[u] : nullptr);
                    if (!out) cand_ptr[u + 1] = len;
                }
            });
        };
        pass(nullptr);
        cand_ptr[0] = 0;
        for (int64_t u = 0; u < rows; ++u) cand_ptr[u + 1] += cand_ptr[u];
        if (cand_item) pass(cand_item);
        return PCR_OK;
    } catch (const std::bad_alloc&) { pcr_set_error("pcr_sample_negatives: out of host memory"); return PCR_ERR_NOMEM; }
}

// ------------------------------------------------------------------------------ beyond-accuracy metrics (include/primalcr.h)
int pcr_evaluate_diversity_model_check(const double* U, int64_t d1, const double* V, int64_t d2, int64_t k, const int64_t* index,
                                       const int32_t* item, int64_t n, const int32_t* users, int ncut, const int* cutoffs, int dtype,
                                       const pcr_diversity_stats* stats, bool* sorted) {
    static const char* who = "pcr_evaluate_diversity_model";
    const int rc = pcr_cutoffs_check(who, ncut, cutoffs);
    if (rc != PCR_OK) return rc;
    if (!stats) { pcr_set_error(std::string(who) + ": null stats"); return PCR_ERR_ARG; }
    static const int32_t no_items = 0;         // (the lists stay on the device: nothing for the output check to find missing)
    static const double no_scores = 0.0;
    return pcr_recommend_model_check(U, d1, V, d2, k, index, item, n, users, cutoffs[ncut - 1], dtype, &no_items, &no_scores, sorted, who);
}

// ------------------------------------------------------------------------------ MMR re-ranking (include/primalcr.h)
int pcr_rerank_check(const char* who, int topk, int pool, double theta) {
    auto bad = [who](const std::string& why) { pcr_set_error(std::string(who) + ": " + why); return PCR_ERR_ARG; };
    if (topk < 1) return bad("topk = " + std::to_string(topk) + " below 1");
    if (pool < topk) return bad("pool = " + std::to_string(pool) + " below topk = " + std::to_string(topk));
    if (pool > PCR_RECOMMEND_MAX_K) return bad("pool = " + std::to_string(pool) + " above " + std::to_string(PCR_RECOMMEND_MAX_K));
    if (!(theta >= 0.0 && theta <= 1.0)) return bad("theta must be in [0, 1]");       // (a NaN fails both compares)
    return PCR_OK;
}

int pcr_recommend_diverse_model_check(const double* U, int64_t d1, const double* V, int64_t d2, int64_t k, const int64_t* index,
                                      const int32_t* item, int64_t n, const int32_t* users, int topk, int pool, double theta, int dtype,
                                      const int32_t* items, const double* scores, bool* sorted) {
    static const char* who = "pcr_recommend_diverse_model";
    const int rc = pcr_rerank_check(who, topk, pool, theta);
    if (rc != PCR_OK) return rc;
    return pcr_recommend_model_check(U, d1, V, d2, k, index, item, n, users, pool, dtype, items, scores, sorted, who);
}

// ------------------------------------------------------------------------------ group-capped lists (include/primalcr.h)
int pcr_cap_check(const char* who, int topk, int pool, const int32_t* group, int cap) {
    auto bad = [who](const std::string& why) { pcr_set_error(std::string(who) + ": " + why); return PCR_ERR_ARG; };
    if (!group) return bad("null group");
    if (cap < 1) return bad("cap = " + std::to_string(cap) + " below 1");
    if (topk < 1) return bad("topk = " + std::to_string(topk) + " below 1");
    if (pool < topk) return bad("pool = " + std::to_string(pool) + " below topk = " + std::to_string(topk));
    if (pool > PCR_RECOMMEND_MAX_K) return bad("pool = " + std::to_string(pool) + " above " + std::to_string(PCR_RECOMMEND_MAX_K));
    return PCR_OK;
}

int pcr_cap_filter_check(const char* who, const pcr_item_filter* f) {
    if (!f) return PCR_OK;
    if (f->cand_ptr) { pcr_set_error(std::string(who) + ": candidate rows do not go with a group cap (an allow set does)"); return PCR_ERR_UNSUPPORTED; }
    if (!f->allow) { pcr_set_error(std::string(who) + ": a filter without an allow set (NULL is the filter that allows everything)"); return PCR_ERR_ARG; }
    return PCR_OK;
}

int pcr_recommend_capped_model_check(const double* U, int64_t d1, const double* V, int64_t d2, int64_t k, const int64_t* index,
                                     const int32_t* item, int64_t n, const int32_t* users, int topk, int pool, const int32_t* group, int cap,
                                     int dtype, const pcr_item_filter* f, const int32_t* items, const double* scores, bool* sorted) {
    static const char* who = "pcr_recommend_capped_model";
    int rc = pcr_cap_check(who, topk, pool, group, cap);
    if (rc == PCR_OK) rc = pcr_recommend_model_check(U, d1, V, d2, k, index, item, n, users, pool, dtype, items, scores, sorted, who);
    return rc != PCR_OK ? rc : pcr_cap_filter_check(who, f);
}

void pcr_cap_stats_from(int64_t n, int topk, const uint8_t* status, const int32_t* items, pcr_cap_stats* stats) {
    pcr_cap_stats t = {n, 0, 0, 0, 0};
    for (int64_t i = 0; i < n; ++i) {
        const int32_t* row = items + i * topk;
        int len = 0;
        while (len < topk && row[len] >= 0) ++len;
        (status[i] == PCR_CAP_EXACT ? t.exact : t.exhausted) += 1;
        t.short_rows += len < topk ? 1 : 0;
        t.kept += len;
    }
    *stats = t;
}

int pcr_exposure_stats(const int64_t* exposure, int64_t d2, int64_t* recs, int64_t* items_covered, double* coverage, double* gini) {
    if (!exposure || d2 < 1) { pcr_set_error("pcr_exposure_stats: bad argument"); return PCR_ERR_ARG; }
    std::vector<int64_t> x(exposure, exposure + d2);
    for (int64_t v : x) if (v < 0) { pcr_set_error("pcr_exposure_stats: a negative exposure count"); return PCR_ERR_ARG; }
    std::sort(x.begin(), x.end());
    __int128 num = 0, tot = 0;
    int64_t cov = 0;
    for (int64_t i = 0; i < d2; ++i) {
        num += (__int128)(2 * (i + 1) - d2 - 1) * (__int128)x[(size_t)i];
        tot += x[(size_t)i];
        cov += x[(size_t)i] > 0 ? 1 : 0;
    }
    if (tot > (__int128)INT64_MAX) { pcr_set_error("pcr_exposure_stats: the exposure counts sum to more than an int64 holds"); return PCR_ERR_ARG; }
    const __int128 den = (__int128)d2 * tot;
    if (recs) *recs = (int64_t)tot;
    if (items_covered) *items_covered = cov;
    if (coverage) *coverage = (double)cov / (double)d2;
    if (gini) *gini = tot > 0 ? (double)num / (double)den : 0.0;
    return PCR_OK;
}

void pcr_diversity_info(int64_t d1, const double* pop, int64_t d2, double* info) {
    for (int64_t j = 0; j < d2; ++j) info[j] = log2((double)(d1 + 1) / (pop[j] + 1.0));
}

int pcr_diversity_stats_from(const double* sums, int ncut, const int* cutoffs, const double* expo, int64_t d2,
                             pcr_diversity_stats* stats, int64_t* exposure) {
    auto mean = [](double s, double n) { return n > 0.0 ? s / n : 0.0; };
    std::vector<int64_t> row((size_t)d2);
    for (int c = 0; c < ncut; ++c) {
        const double* x = sums + 8 * c;
        pcr_diversity_stats& o = stats[c];
        for (int64_t j = 0; j < d2; ++j) row[(size_t)j] = (int64_t)expo[(size_t)c * d2 + j];
        o.cutoff = cutoffs[c];
        o.users = (int64_t)sums[8 * ncut];
        o.users_ild = (int64_t)x[7];
        const int rc = pcr_exposure_stats(row.data(), d2, &o.recs, &o.items_covered, &o.coverage, &o.gini);
        if (rc != PCR_OK) return rc;
        o.novelty = mean(x[1], x[3]);
        o.ild = mean(x[6], x[7]);
        if (exposure) std::copy(row.begin(), row.end(), exposure + (size_t)c * d2);
    }
    return PCR_OK;
}

// ------------------------------------------------------------------------------ metrics of given and re-ranked lists (include/primalcr.h)
int pcr_lists_check(const char* who, int64_t d2, int64_t n, int L, const int32_t* lists) {
    const int nth = pcr_host_threads();
    struct Bad { int64_t row = -1; int pos = 0, kind = 0; };   // kind 1: outside [0, d2); 2: an entry after -1; 3: an id twice
    std::vector<Bad> first((size_t)nth);
    pcr_parallel_ranges(n, nth, [&](int t, int64_t lo, int64_t hi) {
        std::vector<int32_t> row;
        for (int64_t i = lo; i < hi; ++i) {
            const int32_t* l = lists + (size_t)i * (size_t)L;
            int len = 0;
            while (len < L && l[len] != -1) ++len;
            for (int p = 0; p < L; ++p) {
                if (l[p] == -1) continue;
                if (l[p] < 0 || l[p] >= d2) { first[(size_t)t] = Bad{i, p, 1}; return; }
                if (p > len) { first[(size_t)t] = Bad{i, p, 2}; return; }
            }
            row.assign(l, l + len);
            std::sort(row.begin(), row.end());
            for (int p = 1; p < len; ++p)
                if (row[(size_t)p] == row[(size_t)p - 1]) {
                    int at = 0, seen = 0;
                    for (int e = 0; e < len; ++e) if (l[e] == row[(size_t)p] && ++seen == 2) { at = e; break; }
                    first[(size_t)t] = Bad{i, at, 3};
                    return;
                }
        }
    });
    for (const Bad& b : first) {
        if (b.row < 0) continue;
        const std::string at = "list " + std::to_string(b.row) + ", position " + std::to_string(b.pos);
        const int32_t id = lists[(size_t)b.row * (size_t)L + (size_t)b.pos];
        pcr_set_error(std::string(who) + ": " + (b.kind == 1 ? at + ": item " + std::to_string(id) + " outside [0, d2) and not -1"
                                                 : b.kind == 2 ? at + ": item " + std::to_string(id) + " follows the -1 padding"
                                                               : at + ": item " + std::to_string(id) + " is in the list twice"));
        return PCR_ERR_ARG;
    }
    return PCR_OK;
}

// the optional test CSR and the accuracy outputs of the list entries: *has = a test CSR is given
static int list_outputs_check(const char* who, int64_t d1, int64_t d2, const int64_t* tindex, const int32_t* titem, const double* tval,
                              const pcr_topn_stats* topn, const double* per_user_topn, bool* has) {
    auto bad = [who](const std::string& why) { pcr_set_error(std::string(who) + ": " + why); return PCR_ERR_ARG; };
    *has = tindex || titem || tval;
    if (!*has) {
        if (topn || per_user_topn) return bad("topn and per_user_topn must be NULL without a test CSR");
        return PCR_OK;
    }
    if (!topn) return bad("null topn stats with a test CSR");
    return test_csr_check(who, d1, d2, tindex, titem, tval);
}

int pcr_evaluate_lists_model_check(const double* V, int64_t d2, int64_t k, int64_t d1, const int64_t* index, const int32_t* item,
                                   const int64_t* tindex, const int32_t* titem, const double* tval, int64_t n, const int32_t* users, int L,
                                   const int32_t* lists, int ncut, const int* cutoffs, double threshold, int dtype,
                                   const pcr_topn_stats* topn, const double* per_user_topn, const pcr_diversity_stats* div) {
    static const char* who = "pcr_evaluate_lists_model";
    auto bad = [](const std::string& why) { pcr_set_error(std::string(who) + ": " + why); return PCR_ERR_ARG; };
    if (L < 1 || L > PCR_RECOMMEND_MAX_K) return bad("L = " + std::to_string(L) + " outside [1, " + std::to_string(PCR_RECOMMEND_MAX_K) + "]");
    int rc = pcr_cutoffs_check(who, ncut, cutoffs);
    if (rc != PCR_OK) return rc;
    if (cutoffs[ncut - 1] > L) return bad("cutoff " + std::to_string(cutoffs[ncut - 1]) + " above the list length L = " + std::to_string(L));
    if (std::isnan(threshold)) return bad("threshold is NaN");
    if (!div) return bad("null diversity stats");
    if (!users && n != d1) return bad("n must be d1 without a user list");
    static const int32_t no_items = 0;         // (nothing is written through these: the output check has nothing to find missing)
    static const double no_scores = 0.0;
    rc = pcr_recommend_model_check(V, d1, V, d2, k, index, item, n, users, L, dtype, &no_items, &no_scores, nullptr, who);
    if (rc != PCR_OK) return rc;
    bool has = false;
    rc = list_outputs_check(who, d1, d2, tindex, titem, tval, topn, per_user_topn, &has);
    if (rc != PCR_OK) return rc;
    if (n > 0 && !lists) return bad("null lists");
    return pcr_lists_check(who, d2, n, L, lists);
}

int pcr_tradeoff_check(const char* who, int nth, const double* thetas, int pool, int ncut, const int* cutoffs, double threshold,
                       const pcr_diversity_stats* div) {
    auto bad = [who](const std::string& why) { pcr_set_error(std::string(who) + ": " + why); return PCR_ERR_ARG; };
    int rc = pcr_cutoffs_check(who, ncut, cutoffs);
    if (rc != PCR_OK) return rc;
    if (nth < 1 || nth > PCR_RERANK_MAX_THETAS || !thetas)
        return bad("nth = " + std::to_string(nth) + " outside [1, " + std::to_string(PCR_RERANK_MAX_THETAS) + "] (or no thetas)");
    for (int t = 0; t < nth; ++t) {
        rc = pcr_rerank_check(who, cutoffs[ncut - 1], pool, thetas[t]);
        if (rc != PCR_OK) return rc;
    }
    if (std::isnan(threshold)) return bad("threshold is NaN");
    if (!div) return bad("null diversity stats");
    return PCR_OK;
}

int pcr_evaluate_rerank_model_check(const double* U, int64_t d1, const double* V, int64_t d2, int64_t k, const int64_t* index,
                                    const int32_t* item, const int64_t* tindex, const int32_t* titem, const double* tval, int64_t n,
                                    const int32_t* users, int nth, const double* thetas, int pool, int ncut, const int* cutoffs,
                                    double threshold, int dtype, const pcr_topn_stats* topn, const double* per_user_topn,
                                    const pcr_diversity_stats* div, bool* sorted) {
    static const char* who = "pcr_evaluate_rerank_model";
    int rc = pcr_tradeoff_check(who, nth, thetas, pool, ncut, cutoffs, threshold, div);
    if (rc != PCR_OK) return rc;
    static const int32_t no_items = 0;
    static const double no_scores = 0.0;
    rc = pcr_recommend_model_check(U, d1, V, d2, k, index, item, n, users, pool, dtype, &no_items, &no_scores, sorted, who);
    if (rc != PCR_OK) return rc;
    bool has = false;
    return list_outputs_check(who, d1, d2, tindex, titem, tval, topn, per_user_topn, &has);
}

int64_t pcr_list_relevance(int64_t rows, const int64_t* tptr, const int32_t* titem, const double* tval, double threshold, int ncut,
                           const int* cutoffs, int64_t n, const int32_t* users, int L, PcrTopnRel& out) {
    PcrTopnRel rel;
    if (tptr) pcr_topn_relevance(rows, tptr, titem, tval, threshold, ncut, cutoffs, rel);
    std::vector<int64_t> slot((size_t)rows, -1);       // user -> its row in the compact tables
    for (size_t i = 0; i < rel.users.size(); ++i) slot[(size_t)rel.users[i]] = (int64_t)i;
    out.users.clear();
    out.disc.resize((size_t)L);
    for (int i = 0; i < L; ++i) out.disc[(size_t)i] = 1.0 / log2((double)(i + 2));
    out.rptr.assign((size_t)n + 1, 0);
    int64_t counted = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t s = slot[(size_t)(users ? users[i] : i)];
        out.rptr[(size_t)i + 1] = out.rptr[(size_t)i] + (s < 0 ? 0 : rel.rptr[(size_t)s + 1] - rel.rptr[(size_t)s]);
        counted += s >= 0 ? 1 : 0;
    }
    out.ritem.resize((size_t)out.rptr[(size_t)n]);
    out.rgain.resize((size_t)out.rptr[(size_t)n]);
    out.idcg.assign((size_t)n * (size_t)ncut * 2, 0.0);
    pcr_parallel_ranges(n, pcr_host_threads(), [&](int, int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; ++i) {
            const int64_t s = slot[(size_t)(users ? users[i] : i)];
            if (s < 0) continue;
            const int64_t b = rel.rptr[(size_t)s], e = rel.rptr[(size_t)s + 1];
            std::copy(rel.ritem.begin() + b, rel.ritem.begin() + e, out.ritem.begin() + out.rptr[(size_t)i]);
            std::copy(rel.rgain.begin() + b, rel.rgain.begin() + e, out.rgain.begin() + out.rptr[(size_t)i]);
            std::copy(rel.idcg.begin() + s * ncut * 2, rel.idcg.begin() + (s + 1) * ncut * 2, out.idcg.begin() + i * ncut * 2);
        }
    });
    return counted;
}

// ------------------------------------------------------------------------------------------
// fold-in (include/primalcr.h, "fold-in"): argument checks and the host-side plan
// ------------------------------------------------------------------------------------------
// What both fold-in plans (pcr_fold_in_check, pcr_fold_in_ridge_check) share.  The scan of n CSR rows over d2 columns, by the host
// threads: bit 0 = an id outside [0, d2), bit 1 = a rating that is not finite, bit 2 = a row that is not item-ascending
int pcr_csr_rows_scan(int64_t d2, int64_t n, const int64_t* index, const int32_t* item, const double* val) {
    const int nth = pcr_host_threads();
    std::vector<int> st((size_t)nth, 0);
    pcr_parallel_ranges(n, nth, [&](int t, int64_t lo, int64_t hi) {
        for (int64_t u = lo; u < hi; ++u)
            for (int64_t z = index[u]; z < index[u + 1]; ++z) {
                if (item[z] < 0 || item[z] >= d2) st[(size_t)t] |= 1;
                if (!std::isfinite(val[z])) st[(size_t)t] |= 2;
                if (z > index[u] && item[z] < item[z - 1]) st[(size_t)t] |= 4;
            }
    });
    int all = 0;
    for (int x : st) all |= x;
    return all;
}
// ... and the copy X of the rows; sort: rows in ascending item order (equal items keep their order), the ratings with them
void pcr_csr_sorted_copy(int64_t d2, int64_t n, const int64_t* index, const int32_t* item, const double* val, bool sort, PcrCsr& X) {
    const int64_t nnz = index[n];
    X.d1 = n; X.d2 = d2;
    X.index.assign(index, index + n + 1);
    X.item.assign(item, item + nnz);
    X.val.assign(val, val + nnz);
    if (sort)
        pcr_parallel_ranges(n, pcr_host_threads(), [&](int, int64_t lo, int64_t hi) {
            std::vector<int64_t> perm;
            for (int64_t u = lo; u < hi; ++u) {
                const int64_t a = index[u], len = index[u + 1] - a;
                perm.resize((size_t)len);
                for (int64_t q = 0; q < len; ++q) perm[(size_t)q] = a + q;
                std::stable_sort(perm.begin(), perm.end(), [&](int64_t x, int64_t y) { return item[x] < item[y]; });
                for (int64_t q = 0; q < len; ++q) { X.item[(size_t)(a + q)] = item[perm[(size_t)q]]; X.val[(size_t)(a + q)] = val[perm[(size_t)q]]; }
            }
        });
}

// with_out: the fold-in entries' own arguments (steps, the output) are checked in their place; pcr_fold_in_rows_check leaves them out
static int fold_in_check_impl(const char* who, int solver_type, int64_t d2, int64_t n, const int64_t* index, const int32_t* item, const double* val,
                              bool with_out, int steps, const double* U_out, PcrFoldinPlan* plan) {
    auto bad = [who](const std::string& why) { pcr_set_error(std::string(who) + ": " + why); return PCR_ERR_ARG; };
    if (solver_type == PCR_SOLVER_CCDR1) {
        pcr_set_error(std::string(who) + ": solver type 0 (CCDR1) is not supported: its squared-loss fold-in is a ridge solve");
        return PCR_ERR_UNSUPPORTED;
    }
    if (solver_type != PCR_SOLVER_PCR && solver_type != PCR_SOLVER_PCRPP) return bad("wrong solver type (" + std::to_string(solver_type) + "): 1 = PrimalCR, 2 = PrimalCR++");
    if (n < 0 || d2 < 1 || !index) return bad("bad argument");
    if (d2 >= ((int64_t)1 << 31) - 64) return bad("more than 2^31 items");
    if (n >= ((int64_t)1 << 31) - 64) return bad("more than 2^31 users in one call");
    if (with_out && steps < 1) return bad("steps = " + std::to_string(steps) + " must be at least 1");
    if (with_out && n > 0 && !U_out) return bad("null output");
    if (index[0] != 0) return bad("index[0] must be 0");
    for (int64_t u = 0; u < n; ++u) {
        if (index[u + 1] < index[u]) return bad("index not monotone at user " + std::to_string(u));
        if (index[u + 1] - index[u] > ((int64_t)1 << 30)) return bad("user " + std::to_string(u) + " has more than 2^30 ratings");
    }
    const int64_t nnz = index[n];
    if (nnz > 0 && (!item || !val)) return bad("null item / val");
    const int all = pcr_csr_rows_scan(d2, n, index, item, val);
    if (all & 1) return bad("an item id is outside [0, d2)");
    if (all & 2) return bad("a rating is not finite");
    PcrFoldinPlan local;
    PcrFoldinPlan& P = plan ? *plan : local;
    pcr_csr_sorted_copy(d2, n, index, item, val, (all & 4) != 0, P.X);
    std::string err;
    const int rc = pcr_build_levels(P.X, 0, n, solver_type, P.lv, err);
    if (rc != PCR_OK) { pcr_set_error(std::string(who) + ": " + err); return rc; }
    // users by descending length (equal lengths by ascending id): the longest start first; the three workgroup forms are ranges
    P.order.resize((size_t)n);
    for (int64_t u = 0; u < n; ++u) P.order[(size_t)u] = (int32_t)u;
    std::stable_sort(P.order.begin(), P.order.end(), [&](int32_t x, int32_t y) { return index[x + 1] - index[x] > index[y + 1] - index[y]; });
    P.n_big = P.n_lds = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t len = index[P.order[(size_t)i] + 1] - index[P.order[(size_t)i]];
        if (len > PCR_FOLDIN_LDS_MAX) P.n_big += 1;
        else if (len > PCR_FOLDIN_WAVE_MAX) P.n_lds += 1;
    }
    return PCR_OK;
}

int pcr_fold_in_check(const char* who, int solver_type, int64_t d2, int64_t n, const int64_t* index, const int32_t* item, const double* val,
                      int steps, const double* U_out, PcrFoldinPlan* plan) {
    return fold_in_check_impl(who, solver_type, d2, n, index, item, val, true, steps, U_out, plan);
}
int pcr_fold_in_rows_check(const char* who, int solver_type, int64_t d2, int64_t n, const int64_t* index, const int32_t* item, const double* val,
                           PcrFoldinPlan* plan) {
    return fold_in_check_impl(who, solver_type, d2, n, index, item, val, false, 0, nullptr, plan);
}

int pcr_fold_in_model_check(const pcr_params* p, const double* V, int64_t d2, int64_t n, const int64_t* index, const int32_t* item,
                            const double* val, int steps, const double* U_out, PcrFoldinPlan* plan) {
    auto bad = [](const std::string& why) { pcr_set_error("pcr_fold_in_model: " + why); return PCR_ERR_ARG; };
    if (!p) return bad("null parameters");
    if (!V) return bad("null V");
    if (p->k < 1) return bad("rank k must be >= 1");
    if (p->precision != PCR_F32 && p->precision != PCR_F64) return bad("precision must be PCR_F32 or PCR_F64");
    if (!std::isfinite(p->lambda) || !std::isfinite(p->stepsize) || !std::isfinite(p->cg_tol)) return bad("lambda, stepsize and cg_tol must be finite");
    if (p->cg_max_iter < 0) return bad("cg_max_iter must not be negative");
    return pcr_fold_in_check("pcr_fold_in_model", p->solver_type, d2, n, index, item, val, steps, U_out, plan);
}

void pcr_foldin_stats_from(const double* per_user, int64_t n, pcr_foldin_stats* stats) {
    pcr_foldin_stats s = {};
    s.users = n;
    for (int64_t u = 0; u < n; ++u) {
        const double* o = per_user + (size_t)u * PCR_FOLDIN_FIELDS;
        s.steps += (int64_t)o[0]; s.cg += (int64_t)o[1]; s.ls += (int64_t)o[2];
        s.obj += o[3];
        const int status = (int)o[5];
        if (status == PCR_FOLDIN_CONVERGED) s.converged += 1; else if (status == PCR_FOLDIN_STEP_CAP) s.step_cap += 1; else s.stalled += 1;
    }
    *stats = s;
}

// ------------------------------------------------------------------------------------------
// explanations (include/primalcr.h, "explaining recommendations"): argument checks; the plan is fold-in's
// ------------------------------------------------------------------------------------------
// what both explanation families check of the lists and the outputs: lists [n][L] over d2 items (named `dim` in the messages),
// the contributor tables, L and E
static int explain_lists_check(const char* who, int64_t d2, const char* dim, int64_t n, int L, const int32_t* lists, int E, const int32_t* expl_item,
                               const double* expl_contrib) {
    auto bad = [who](const std::string& why) { pcr_set_error(std::string(who) + ": " + why); return PCR_ERR_ARG; };
    if (n > 0 && !lists) return bad("null lists");
    if (n > 0 && (!expl_item || !expl_contrib)) return bad("null expl_item / expl_contrib");
    if (L < 1 || L > PCR_EXPLAIN_MAX_L) return bad("L = " + std::to_string(L) + " must be inside [1, " + std::to_string(PCR_EXPLAIN_MAX_L) + "]");
    if (E < 1 || E > PCR_EXPLAIN_MAX_E) return bad("E = " + std::to_string(E) + " must be inside [1, " + std::to_string(PCR_EXPLAIN_MAX_E) + "]");
    const int nth = pcr_host_threads();
    std::vector<int> st((size_t)nth, 0);
    pcr_parallel_ranges(n, nth, [&](int t, int64_t lo, int64_t hi) {
        for (int64_t u = lo; u < hi; ++u) {
            bool pad = false;
            for (int l = 0; l < L; ++l) {
                const int32_t j = lists[(size_t)u * L + l];
                if (j == -1) { pad = true; continue; }
                if (j < 0 || j >= d2) st[(size_t)t] |= 1;
                else if (pad) st[(size_t)t] |= 2;
            }
        }
    });
    int all = 0;
    for (int x : st) all |= x;
    if (all & 1) return bad(std::string("a list id is outside [0, ") + dim + ") and not -1");
    if (all & 2) return bad("a list holds an id after a -1");
    return PCR_OK;
}

static int fold_in_ls_args(const char* who, bool need_F, const double* F, int64_t rows, int64_t k, double lambda, int precision, int64_t n,
                           const int64_t* index, const int32_t* item, const double* val, bool with_out, const double* U_out, PcrCsr& X);

int pcr_explain_ridge_check(const char* who, bool need_F, const double* F, int64_t rows, int64_t k, double lambda, int nonneg, int precision,
                            int64_t n, const int64_t* index, const int32_t* item, const double* val, bool has_U, int L, const int32_t* lists, int E,
                            const int32_t* expl_item, const double* expl_contrib, PcrRidgePlan* plan) {
    auto bad = [who](const std::string& why) { pcr_set_error(std::string(who) + ": " + why); return PCR_ERR_ARG; };
    PcrRidgePlan local;
    PcrRidgePlan& P = plan ? *plan : local;
    const int rc = fold_in_ls_args(who, need_F, F, rows, k, lambda, precision, n, index, item, val, false, nullptr, P.X);
    if (rc != PCR_OK) return rc;
    if (!(lambda > 0.0)) return bad("lambda must be finite and > 0");
    if (!has_U && nonneg) return bad("nonneg needs the rows U: the free set is read from them");
    const int lrc = explain_lists_check(who, rows, "rows", n, L, lists, E, expl_item, expl_contrib);
    if (lrc != PCR_OK) return lrc;
    if ((k + 15) / 16 * 16 > PCR_RIDGE_DIRECT_MAX) {
        pcr_set_error(std::string(who) + ": rank " + std::to_string(k) + " padded to 16 is beyond " + std::to_string(PCR_RIDGE_DIRECT_MAX) +
                      ": the user's k x k system would not fit the kernel's LDS");
        return PCR_ERR_UNSUPPORTED;
    }
    // one launch class: the longest users start first (equal lengths by ascending id)
    PcrRidgePlan::Range g;
    g.form = PCR_RIDGE_PRIMAL; g.block = 256; g.tiles = (int)((k + 15) / 16);
    g.first = 0; g.count = n;
    P.order.resize((size_t)n);
    for (int64_t u = 0; u < n; ++u) P.order[(size_t)u] = (int32_t)u;
    std::stable_sort(P.order.begin(), P.order.end(), [&](int32_t x, int32_t y) { return index[x + 1] - index[x] > index[y + 1] - index[y]; });
    P.ranges.assign(1, g);
    return PCR_OK;
}

void pcr_explain_ridge_stats_from(const double* per_pair, const double* per_user, const int32_t* expl_item, const int32_t* lists, int64_t n, int L,
                                  int E, pcr_explain_ridge_stats* stats) {
    pcr_explain_ridge_stats s = {};
    s.users = n;
    for (int64_t z = 0; z < n * L; ++z) {
        if (lists[z] < 0) continue;                                         // padding
        s.pairs += 1;
        const double r = std::fabs(per_pair[(size_t)z * PCR_EXPLAIN_PAIR_FIELDS + 3]);
        if (r > s.residual_abs_max) s.residual_abs_max = r;
    }
    for (int64_t z = 0; z < n * L * E; ++z) s.contributors += expl_item[z] >= 0 ? 1 : 0;
    for (int64_t u = 0; u < n; ++u) s.singular += (int)per_user[(size_t)u * PCR_EXPLAIN_RIDGE_USER_FIELDS + 4] == PCR_RIDGE_SINGULAR ? 1 : 0;
    *stats = s;
}

int pcr_explain_check(const char* who, bool need_factors, const pcr_params* p, const double* V, int64_t d2, int64_t n, const int64_t* index,
                      const int32_t* item, const double* val, const double* U, const double* weights, int L, const int32_t* lists, int E,
                      const int32_t* expl_item, const double* expl_contrib, PcrFoldinPlan* plan) {
    auto bad = [who](const std::string& why) { pcr_set_error(std::string(who) + ": " + why); return PCR_ERR_ARG; };
    if (!p) return bad("null parameters");
    if (need_factors) {
        if (!V) return bad("null V");
        if (p->k < 1) return bad("rank k must be >= 1");
        if (p->precision != PCR_F32 && p->precision != PCR_F64) return bad("precision must be PCR_F32 or PCR_F64");
    }
    if (!std::isfinite(p->lambda) || !(p->lambda > 0.0)) return bad("lambda must be finite and > 0");
    if (p->solver_type == PCR_SOLVER_CCDR1) {
        pcr_set_error(std::string(who) + ": solver type 0 (CCDR1) is not supported: a squared-loss row decomposes through its residuals, not through sweep coefficients");
        return PCR_ERR_UNSUPPORTED;
    }
    const int rc = pcr_fold_in_rows_check(who, p->solver_type, d2, n, index, item, val, plan);
    if (rc != PCR_OK) return rc;
    if (n > 0 && need_factors && !U) return bad("null U");
    const int lrc = explain_lists_check(who, d2, "d2", n, L, lists, E, expl_item, expl_contrib);
    if (lrc != PCR_OK) return lrc;
    if (weights)
        for (int64_t u = 0; u < n; ++u)
            if (!std::isfinite(weights[u]) || !(weights[u] > 0.0)) return bad("the weight of user " + std::to_string(u) + " must be finite and > 0");
    return PCR_OK;
}

void pcr_explain_stats_from(const double* per_pair, const int32_t* expl_item, const int32_t* lists, int64_t n, int L, int E, pcr_explain_stats* stats) {
    pcr_explain_stats s = {};
    s.users = n;
    for (int64_t z = 0; z < n * L; ++z) {
        const double* o = per_pair + (size_t)z * PCR_EXPLAIN_PAIR_FIELDS;
        if (lists[z] < 0) continue;                                         // padding
        s.pairs += 1;
        const double r = std::fabs(o[3]);
        if (r > s.residual_abs_max) s.residual_abs_max = r;
    }
    for (int64_t z = 0; z < n * L * E; ++z) s.contributors += expl_item[z] >= 0 ? 1 : 0;
    *stats = s;
}

// ------------------------------------------------------------------------------------------
// item fold-in (include/primalcr.h, "item fold-in"): argument checks and the host-side plan
// ------------------------------------------------------------------------------------------
int pcr_fold_in_items_check(const char* who, bool need_factors, const pcr_params* p, const double* U, int64_t d1, const double* V, int64_t d2,
                            const int64_t* tr_index, const int32_t* tr_item, const double* tr_val, int64_t n, const int64_t* index,
                            const int32_t* user, const double* val, int steps, const double* V_out, PcrItemfoldPlan* plan) {
    auto bad = [who](const std::string& why) { pcr_set_error(std::string(who) + ": " + why); return PCR_ERR_ARG; };
    if (!p) return bad("null parameters");
    const int solver_type = p->solver_type;
    if (solver_type == PCR_SOLVER_CCDR1) {
        pcr_set_error(std::string(who) + ": solver type 0 (CCDR1) is not supported: its item fold-in is the ridge solve with F = U");
        return PCR_ERR_UNSUPPORTED;
    }
    if (solver_type != PCR_SOLVER_PCR && solver_type != PCR_SOLVER_PCRPP) return bad("wrong solver type (" + std::to_string(solver_type) + "): 1 = PrimalCR, 2 = PrimalCR++");
    if (need_factors) {
        if (!U) return bad("null U");
        if (!V) return bad("null V");
        if (p->k < 1) return bad("rank k must be >= 1");
        if (p->precision != PCR_F32 && p->precision != PCR_F64) return bad("precision must be PCR_F32 or PCR_F64");
        if (!std::isfinite(p->lambda) || !std::isfinite(p->stepsize) || !std::isfinite(p->cg_tol)) return bad("lambda, stepsize and cg_tol must be finite");
        if (p->cg_max_iter < 0) return bad("cg_max_iter must not be negative");
    }
    if (n < 0 || d1 < 1 || d2 < 1 || !index) return bad("bad argument");
    if (d1 >= ((int64_t)1 << 31) - 64) return bad("more than 2^31 users");
    if (d2 >= ((int64_t)1 << 31) - 64) return bad("more than 2^31 items");
    if (n >= ((int64_t)1 << 31) - 64) return bad("more than 2^31 items in one call");
    if (steps < 1) return bad("steps = " + std::to_string(steps) + " must be at least 1");
    if (n > 0 && !V_out) return bad("null output");
    if (!tr_index) return bad("null training index");
    if (index[0] != 0) return bad("index[0] must be 0");
    for (int64_t j = 0; j < n; ++j) {
        if (index[j + 1] < index[j]) return bad("index not monotone at item " + std::to_string(j));
        if (index[j + 1] - index[j] > ((int64_t)1 << 30)) return bad("item " + std::to_string(j) + " has more than 2^30 ratings");
    }
    const int64_t np = index[n];
    if (np > 0 && (!user || !val)) return bad("null user / val");
    if (tr_index[0] != 0) return bad("training index[0] must be 0");
    for (int64_t u = 0; u < d1; ++u) {
        if (tr_index[u + 1] < tr_index[u]) return bad("training index not monotone at user " + std::to_string(u));
        if (tr_index[u + 1] - tr_index[u] > ((int64_t)1 << 30)) return bad("user " + std::to_string(u) + " has more than 2^30 training ratings");
    }
    if (tr_index[d1] > 0 && (!tr_item || !tr_val)) return bad("null training item / val");
    const int all = pcr_csr_rows_scan(d1, n, index, user, val);
    if (all & 1) return bad("a user id is outside [0, d1)");
    if (all & 2) return bad("a rating is not finite");

    PcrItemfoldPlan local;
    PcrItemfoldPlan& P = plan ? *plan : local;
    P.n = n;
    // the unique raters, ascending, and a copy of their training rows
    std::vector<int32_t> rpos((size_t)d1, -1);
    for (int64_t z = 0; z < np; ++z) rpos[(size_t)user[z]] = 0;
    P.raters.clear();
    for (int64_t u = 0; u < d1; ++u)
        if (rpos[(size_t)u] == 0) { rpos[(size_t)u] = (int32_t)P.raters.size(); P.raters.push_back((int32_t)u); }
    const int64_t nr = (int64_t)P.raters.size();
    P.R.d1 = nr; P.R.d2 = d2;
    P.R.index.assign((size_t)nr + 1, 0);
    for (int64_t i = 0; i < nr; ++i) P.R.index[(size_t)i + 1] = P.R.index[(size_t)i] + (tr_index[P.raters[(size_t)i] + 1] - tr_index[P.raters[(size_t)i]]);
    P.R.item.resize((size_t)P.R.index[(size_t)nr]);
    P.R.val.resize((size_t)P.R.index[(size_t)nr]);
    const int nth = pcr_host_threads();
    std::vector<int> st((size_t)nth, 0);
    pcr_parallel_ranges(nr, nth, [&](int t, int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; ++i) {
            const int64_t a = tr_index[P.raters[(size_t)i]], len = tr_index[P.raters[(size_t)i] + 1] - a, o = P.R.index[(size_t)i];
            for (int64_t q = 0; q < len; ++q) {
                if (tr_item[a + q] < 0 || tr_item[a + q] >= d2) st[(size_t)t] |= 1;
                if (!std::isfinite(tr_val[a + q])) st[(size_t)t] |= 2;
                P.R.item[(size_t)(o + q)] = tr_item[a + q];
                P.R.val[(size_t)(o + q)] = tr_val[a + q];
            }
        }
    });
    int trall = 0;
    for (int x : st) trall |= x;
    if (trall & 1) return bad("a training item id of a rater is outside [0, d2)");
    if (trall & 2) return bad("a training rating of a rater is not finite");
    std::string err;
    const int rc = pcr_build_levels(P.R, 0, nr, solver_type, P.lv, err);
    if (rc != PCR_OK) { pcr_set_error(std::string(who) + ": training row of a rater (numbered among the call's raters in ascending user order): " + err); return rc; }
    // slots: items by descending rater count (equal counts by ascending id); the three workgroup forms are ranges
    P.order.resize((size_t)n);
    for (int64_t j = 0; j < n; ++j) P.order[(size_t)j] = (int32_t)j;
    std::stable_sort(P.order.begin(), P.order.end(), [&](int32_t x, int32_t y) { return index[x + 1] - index[x] > index[y + 1] - index[y]; });
    P.n_big = P.n_lds = 0;
    P.sptr.assign((size_t)n + 1, 0);
    for (int64_t t = 0; t < n; ++t) {
        const int64_t len = index[P.order[(size_t)t] + 1] - index[P.order[(size_t)t]];
        P.sptr[(size_t)t + 1] = P.sptr[(size_t)t] + len;
        if (len > PCR_ITEMFOLD_LDS_MAX) P.n_big += 1;
        else if (len > PCR_ITEMFOLD_WAVE_MAX) P.n_lds += 1;
    }
    P.puser.resize((size_t)np); P.prater.resize((size_t)np); P.pq.resize((size_t)np);
    P.anypair.assign((size_t)n, 0);
    const bool pp = solver_type == PCR_SOLVER_PCRPP;
    pcr_parallel_ranges(n, nth, [&](int, int64_t lo, int64_t hi) {
        std::vector<int64_t> perm;
        for (int64_t t = lo; t < hi; ++t) {
            const int64_t a = index[P.order[(size_t)t]], len = index[P.order[(size_t)t] + 1] - a, o = P.sptr[(size_t)t];
            perm.resize((size_t)len);
            for (int64_t q = 0; q < len; ++q) perm[(size_t)q] = a + q;
            std::stable_sort(perm.begin(), perm.end(), [&](int64_t x, int64_t y) { return user[x] < user[y]; });
            int any = 0;
            for (int64_t q = 0; q < len; ++q) {
                const int64_t z = perm[(size_t)q];
                const int32_t r = rpos[(size_t)user[z]];
                const double key = pp ? (double)fast_lround(val[z]) : val[z];
                const double* lvv = P.lv.lev_val.data() + P.lv.run_ofs[(size_t)r];
                const int T = (int)(P.lv.run_ofs[(size_t)r + 1] - P.lv.run_ofs[(size_t)r]) - 1;
                const int lb = (int)(std::lower_bound(lvv, lvv + T, key) - lvv);
                const int code = (lb < T && lvv[lb] == key) ? 2 * lb : 2 * lb - 1;
                P.puser[(size_t)(o + q)] = user[z];
                P.prater[(size_t)(o + q)] = r;
                P.pq[(size_t)(o + q)] = code;
                if (T >= 2 || (T == 1 && code != 0)) any = 1;
            }
            P.anypair[(size_t)t] = any;
        }
    });
    return PCR_OK;
}

void pcr_itemfold_stats_from(const double* per_item, int64_t n, pcr_itemfold_stats* stats) {
    pcr_itemfold_stats s = {};
    s.items = n;
    s.unique_raters = stats->unique_raters;
    for (int64_t j = 0; j < n; ++j) {
        const double* o = per_item + (size_t)j * PCR_ITEMFOLD_FIELDS;
        s.raters += (int64_t)o[0]; s.steps += (int64_t)o[1]; s.cg += (int64_t)o[2]; s.ls += (int64_t)o[3];
        s.obj += o[5];
        const int status = (int)o[7];
        if (status == PCR_FOLDIN_CONVERGED) s.converged += 1; else if (status == PCR_FOLDIN_STEP_CAP) s.step_cap += 1; else s.stalled += 1;
    }
    *stats = s;
}

// ------------------------------------------------------------------------------------------
// ridge fold-in (include/primalcr.h, "ridge fold-in"): the form rule, argument checks and the host-side plan
// ------------------------------------------------------------------------------------------
int pcr_ridge_form(int64_t len, int64_t k) {
    if (len <= k && len <= PCR_RIDGE_DIRECT_MAX) return PCR_RIDGE_DUAL;
    if (len > k && (k + 15) / 16 * 16 <= PCR_RIDGE_DIRECT_MAX) return PCR_RIDGE_PRIMAL;
    return PCR_RIDGE_CG;
}

// the argument checks of the ridge and the non-negative entries, and the copy X of the ratings with item-ascending rows
// (with_out: the fold-in entries' output is checked in its place; pcr_explain_ridge_check has other outputs)
static int fold_in_ls_args(const char* who, bool need_F, const double* F, int64_t rows, int64_t k, double lambda, int precision, int64_t n,
                           const int64_t* index, const int32_t* item, const double* val, bool with_out, const double* U_out, PcrCsr& X) {
    auto bad = [who](const std::string& why) { pcr_set_error(std::string(who) + ": " + why); return PCR_ERR_ARG; };
    if (need_F && !F) return bad("null F");
    if (k < 1) return bad("rank k must be >= 1");
    if (rows < 1) return bad("rows must be >= 1");
    if (rows >= ((int64_t)1 << 31) - 64) return bad("more than 2^31 rows");
    if (k >= ((int64_t)1 << 24)) return bad("rank k is too large");
    if (precision != PCR_F32 && precision != PCR_F64) return bad("precision must be PCR_F32 or PCR_F64");
    if (!std::isfinite(lambda) || lambda < 0.0) return bad("lambda must be finite and not negative");
    if (n < 0 || !index) return bad("bad argument");
    if (n >= ((int64_t)1 << 31) - 64) return bad("more than 2^31 users in one call");
    if (with_out && n > 0 && !U_out) return bad("null output");
    if (index[0] != 0) return bad("index[0] must be 0");
    for (int64_t u = 0; u < n; ++u) {
        if (index[u + 1] < index[u]) return bad("index not monotone at user " + std::to_string(u));
        if (index[u + 1] - index[u] > ((int64_t)1 << 30)) return bad("user " + std::to_string(u) + " has more than 2^30 ratings");
    }
    const int64_t nnz = index[n];
    if (nnz > 0 && (!item || !val)) return bad("null item / val");
    const int all = pcr_csr_rows_scan(rows, n, index, item, val);
    if (all & 1) return bad("an item id is outside [0, rows)");
    if (all & 2) return bad("a rating is not finite");
    pcr_csr_sorted_copy(rows, n, index, item, val, (all & 4) != 0, X);
    return PCR_OK;
}

// the launch ranges of a ridge / conf plan (implicit == 0: the ridge rule itself) from the user lengths
static void ridge_plan_ranges(PcrRidgePlan& P, int64_t k, int64_t n, const int64_t* index, int implicit) {
    std::string knob;
    P.force_cg = pcr_tune_get("ridge_form", &knob) && knob == "cg";
    // a user's launch class: the CG form first, then primal and dual, 256 threads before one wave, more tiles before fewer; inside
    // a class the longest users start first (equal lengths by ascending id)
    auto len_of = [&](int32_t u) { return index[u + 1] - index[u]; };
    auto cls_of = [&](int32_t u, PcrRidgePlan::Range* r) {
        const int64_t len = len_of(u);
        const int form = P.force_cg ? PCR_RIDGE_CG : pcr_conf_form(len, k, implicit);
        const int64_t m = form == PCR_RIDGE_DUAL ? std::max<int64_t>(len, 1) : k;
        r->form = form;
        r->block = form == PCR_RIDGE_CG ? 256 : pcr_conf_block(len, k, implicit);
        r->tiles = form == PCR_RIDGE_CG ? 0 : (int)((m + 15) / 16);
        return (int64_t)form * -1000 - (r->block == 256 ? 100 : 0) - r->tiles;
    };
    P.order.resize((size_t)n);
    std::vector<int64_t> key((size_t)n);
    PcrRidgePlan::Range tmp;
    for (int64_t u = 0; u < n; ++u) { P.order[(size_t)u] = (int32_t)u; key[(size_t)u] = cls_of((int32_t)u, &tmp); }
    std::stable_sort(P.order.begin(), P.order.end(), [&](int32_t x, int32_t y) {
        return key[(size_t)x] != key[(size_t)y] ? key[(size_t)x] < key[(size_t)y] : len_of(x) > len_of(y);
    });
    P.ranges.clear();
    for (int64_t i = 0; i < n; ++i) {
        PcrRidgePlan::Range r;
        cls_of(P.order[(size_t)i], &r);
        if (P.ranges.empty() || key[(size_t)P.order[(size_t)i]] != key[(size_t)P.order[(size_t)(i - 1)]]) { r.first = i; r.count = 0; P.ranges.push_back(r); }
        P.ranges.back().count += 1;
    }
}

int pcr_fold_in_ridge_check(const char* who, bool need_F, const double* F, int64_t rows, int64_t k, double lambda, int precision, int64_t n,
                            const int64_t* index, const int32_t* item, const double* val, const double* U_out, PcrRidgePlan* plan) {
    PcrRidgePlan local;
    PcrRidgePlan& P = plan ? *plan : local;
    const int rc = fold_in_ls_args(who, need_F, F, rows, k, lambda, precision, n, index, item, val, true, U_out, P.X);
    if (rc != PCR_OK) return rc;
    ridge_plan_ranges(P, k, n, index, 0);
    return PCR_OK;
}

// ------------------------------------------------------------------------------------------
// confidence-weighted / implicit fold-in (include/primalcr.h): the form rule, argument checks and the host-side plan
// ------------------------------------------------------------------------------------------
int pcr_conf_form(int64_t len, int64_t k, int implicit) {
    if (!implicit) return pcr_ridge_form(len, k);
    return (k + 15) / 16 * 16 <= PCR_RIDGE_DIRECT_MAX ? PCR_RIDGE_PRIMAL : PCR_RIDGE_CG;
}
int pcr_conf_block(int64_t len, int64_t k, int implicit) {
    if (pcr_conf_form(len, k, implicit) == PCR_RIDGE_CG || len > PCR_RIDGE_WAVE_MAX) return 256;
    return implicit && (k + 15) / 16 * 16 > 64 ? 256 : 64;
}

int pcr_fold_in_conf_check(const char* who, bool need_F, const double* F, int64_t rows, int64_t k, double lambda, double alpha, int precision, int64_t n,
                           const int64_t* index, const int32_t* item, const double* val, const double* weight, const double* U_out, PcrConfPlan* plan) {
    PcrConfPlan local;
    PcrConfPlan& P = plan ? *plan : local;
    auto bad = [who](const std::string& why) { pcr_set_error(std::string(who) + ": " + why); return PCR_ERR_ARG; };
    if (!std::isfinite(alpha) || alpha < 0.0) return bad("alpha must be finite and not negative");
    const int rc = fold_in_ls_args(who, need_F, F, rows, k, lambda, precision, n, index, item, val, true, U_out, P.X);
    if (rc != PCR_OK) return rc;
    const int64_t nnz = index[n];
    if (weight)
        for (int64_t z = 0; z < nnz; ++z)
            if (!std::isfinite(weight[z]) || weight[z] <= 0.0) return bad("a weight is not finite or not positive");
    P.alpha = alpha;
    P.plain = !weight && alpha == 0.0;
    ridge_plan_ranges(P, k, n, index, alpha > 0.0 ? 1 : 0);
    if (P.plain) return PCR_OK;
    // the weights through the permutation of pcr_csr_sorted_copy: ascending items, equal items in the caller's order
    P.wt.assign((size_t)nnz, 1.0);
    P.W.assign((size_t)n, 0.0);
    pcr_parallel_ranges(n, pcr_host_threads(), [&](int, int64_t lo, int64_t hi) {
        std::vector<int64_t> perm;
        for (int64_t u = lo; u < hi; ++u) {
            const int64_t a = index[u], len = index[u + 1] - a;
            if (weight) {
                bool asc = true;
                for (int64_t q = 1; q < len; ++q) asc = asc && item[a + q] >= item[a + q - 1];
                if (asc) std::copy(weight + a, weight + a + len, P.wt.begin() + a);
                else {
                    perm.resize((size_t)len);
                    for (int64_t q = 0; q < len; ++q) perm[(size_t)q] = a + q;
                    std::stable_sort(perm.begin(), perm.end(), [&](int64_t x, int64_t y) { return item[x] < item[y]; });
                    for (int64_t q = 0; q < len; ++q) P.wt[(size_t)(a + q)] = weight[perm[(size_t)q]];
                }
            }
            double w = 0.0;
            for (int64_t q = 0; q < len; ++q) w += P.wt[(size_t)(a + q)];
            P.W[(size_t)u] = w + alpha * (double)(rows - len);
        }
    });
    return PCR_OK;
}

void pcr_ridge_stats_from(const double* per_user, int64_t n, pcr_ridge_stats* stats) {
    pcr_ridge_stats s = {};
    s.users = n;
    for (int64_t u = 0; u < n; ++u) {
        const double* o = per_user + (size_t)u * PCR_RIDGE_FIELDS;
        const int form = (int)o[1], status = (int)o[5];
        if (form == PCR_RIDGE_DUAL) s.dual += 1; else if (form == PCR_RIDGE_PRIMAL) s.primal += 1; else s.cg += 1;
        s.iters += (int64_t)o[2];
        s.loss += o[3]; s.obj += o[4];
        if (status == PCR_RIDGE_SINGULAR) s.singular += 1; else if (status == PCR_RIDGE_CG_CAP) s.cg_cap += 1;
    }
    *stats = s;
}

// ------------------------------------------------------------------------------------------
// non-negative fold-in (include/primalcr.h, "non-negative fold-in"): the form rule, argument checks and the host-side plan
// ------------------------------------------------------------------------------------------
int pcr_nnls_form(int64_t k) { return (k + 15) / 16 * 16 <= PCR_RIDGE_DIRECT_MAX ? PCR_NNLS_DIRECT : PCR_NNLS_CG; }

int pcr_fold_in_nnls_check(const char* who, bool need_F, const double* F, int64_t rows, int64_t k, double lambda, int precision, int64_t n,
                           const int64_t* index, const int32_t* item, const double* val, const double* U_out, PcrRidgePlan* plan) {
    PcrRidgePlan local;
    PcrRidgePlan& P = plan ? *plan : local;
    const int rc = fold_in_ls_args(who, need_F, F, rows, k, lambda, precision, n, index, item, val, true, U_out, P.X);
    if (rc != PCR_OK) return rc;
    std::string knob;
    P.force_cg = pcr_tune_get("nnls_form", &knob) && knob == "cg";
    // (form, workgroup size) are functions of the rank, so the users of a call are one launch class: the longest start first
    // (equal lengths by ascending id)
    PcrRidgePlan::Range g;
    g.form = P.force_cg ? PCR_NNLS_CG : pcr_nnls_form(k);
    g.tiles = g.form == PCR_NNLS_CG ? 0 : (int)((k + 15) / 16);
    g.block = (g.form == PCR_NNLS_CG || g.tiles * 16 > 64) ? 256 : 64;
    g.first = 0; g.count = n;
    P.order.resize((size_t)n);
    for (int64_t u = 0; u < n; ++u) P.order[(size_t)u] = (int32_t)u;
    std::stable_sort(P.order.begin(), P.order.end(), [&](int32_t x, int32_t y) { return index[x + 1] - index[x] > index[y + 1] - index[y]; });
    P.ranges.assign(1, g);
    return PCR_OK;
}

void pcr_nnls_stats_from(const double* per_user, int64_t n, pcr_nnls_stats* stats) {
    pcr_nnls_stats s = {};
    s.users = n;
    for (int64_t u = 0; u < n; ++u) {
        const double* o = per_user + (size_t)u * PCR_NNLS_FIELDS;
        const int form = (int)o[1], status = (int)o[6];
        if (form == PCR_NNLS_DIRECT) s.direct += 1; else s.cg += 1;
        s.pivots += (int64_t)o[2]; s.zeros += (int64_t)o[3];
        s.loss += o[4]; s.obj += o[5];
        if (status == PCR_NNLS_SINGULAR) s.singular += 1; else if (status == PCR_NNLS_CAP) s.cap += 1;
    }
    *stats = s;
}
