// pcr_classes.h -- the length classes of pcr_solver.hip's per-user kernels, laid out on the host: users grouped by rating count
// (make_bins), the cut of the V-side sweeps (pick_sweep_wave_cap) and the whole U-step class layout (ustep_class_layout).
// No GPU calls here, and nothing but a return value and an error text: plain arithmetic on row lengths, level counts, ld, the
// CU count and the launch knobs, so check/classes_dump.hip runs it on a machine without a device (tests/test_classes.py).
// The LDS size functions it calls stay with the kernels whose carving they describe (pcr_ustep.h, pcr_gram.h, pcr_prims.h).
// Bin keeps its one device-side member, the uploaded user list the launches read: pcr_dev.h's DBuf, empty until the solver fills it.
#pragma once
#include <cstdio>
#include <cstring>

#include "pcr_dev.h"
#include "pcr_kernels.h"
#include "pcr_gram.h"

// users of one CSR grouped by length class; each class has its own workgroup size
struct Bin {
    int block = 64;
    bool big = false;
    int K = 1;           // workgroups per user (k_ustep clusters)
    int ugrid = 0;       // k_ustep grid of this bin
    int scratch_ofs = 0; // first global-scratch slice of this bin (big bins that run concurrently must not share slices)
    int cap = 0;         // longest user in the bin
    int limit = 0;       // upper length bound of the class (0: none)
    int rcap = 0;        // k_ustep: rows of V a workgroup keeps resident in LDS
    int unr = 4;         // k_ustep: rows in flight per lane group (8: latency-bound class, one workgroup per CU)
    bool gram = false;   // k_ustep_gram: the dual (Gram-matrix, MFMA) form for users with few ratings
    int wcap = 0;        // k_ustep: 16-bit window entries cached in LDS (cap * ws, or 0)
    int sym = 0;         // k_ustep: symbol id (template parameter CLS) among the classes that run the same workgroup form
    int max_lev = 0;
    int64_t nnz = 0;     // ratings of the users in the bin
    std::vector<int32_t> users;
    DBuf<int32_t> d_users;
};
// length classes: one wave for short users, 256 threads up to 512 ratings, 512 threads up to 4096
// (all with the user's block in LDS), longer users through global scratch.  512 rather than 1024
// threads for the top classes: k_ustep needs more than the 128 VGPRs a 512-thread block may use.
static const int BIN_LIMIT[3] = {128, 512, 4096};
static const int BIN_BLOCK[4] = {64, 256, 512, 512};
static const int GRAM_DEFAULT_CAP = 0;       // default length bound of the dual-form U-step class (0: off; pcr_tune "ustep_gram")

// users by rating count, longest first, ties in user order (what a stable sort by descending length gives): a counting sort,
// once per CSR -- every class layout below is then one pass over this list
static void length_order(const std::vector<int64_t>& uptr, int64_t nu, std::vector<int32_t>& order) {
    order.resize((size_t)nu);
    int64_t maxlen = 0;
    for (int64_t u = 0; u < nu; ++u) maxlen = std::max(maxlen, uptr[u + 1] - uptr[u]);
    if (maxlen > ((int64_t)1 << 24)) {
        for (int64_t u = 0; u < nu; ++u) order[u] = (int32_t)u;
        std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return (uptr[a + 1] - uptr[a]) > (uptr[b + 1] - uptr[b]); });
        return;
    }
    std::vector<int64_t> start((size_t)maxlen + 2, 0);
    for (int64_t u = 0; u < nu; ++u) start[(size_t)(maxlen - (uptr[u + 1] - uptr[u])) + 1]++;
    for (int64_t l = 0; l <= maxlen; ++l) start[(size_t)l + 1] += start[(size_t)l];
    for (int64_t u = 0; u < nu; ++u) order[(size_t)start[(size_t)(maxlen - (uptr[u + 1] - uptr[u]))]++] = (int32_t)u;
}
static void make_bins(const std::vector<int64_t>& uptr, int64_t nu, const std::vector<int64_t>* runofs, std::vector<Bin>& out,
                      const std::vector<int32_t>& order,
                      const std::vector<int>& limits = {BIN_LIMIT[0], BIN_LIMIT[1], BIN_LIMIT[2]},
                      const std::vector<int>& blocks = {BIN_BLOCK[0], BIN_BLOCK[1], BIN_BLOCK[2], BIN_BLOCK[3]}) {
    const int nb = (int)limits.size() + 1;
    out.clear();
    out.resize(nb);
    for (int b = 0; b < nb; ++b) { out[b].block = blocks[b]; out[b].big = (b == nb - 1); out[b].limit = b < nb - 1 ? limits[b] : 0; }
    for (int64_t q = 0; q < nu; ++q) {       // longest first: the tail of a launch is made of short users
        const int32_t u = order[(size_t)q];
        int64_t len = uptr[u + 1] - uptr[u];
        int b = 0;
        while (b < nb - 1 && len > limits[b]) ++b;
        out[b].users.push_back(u);
        out[b].nnz += len;
        out[b].cap = std::max<int>(out[b].cap, (int)len);
        if (runofs) out[b].max_lev = std::max<int>(out[b].max_lev, (int)((*runofs)[u + 1] - (*runofs)[u]) - 1);
    }
}
// profile slot of one kernel launch: "<class>/<workgroup size>[g]" (g = global-scratch variant)
// ("ustep" has several classes per workgroup size: "<class>/<workgroup size>.<length bound>")
static std::string pname(const char* cls, const Bin& b) {
    if (b.gram) return std::string(cls) + "/gram" + std::to_string(b.block) + "." + std::to_string(b.limit);
    std::string s = std::string(cls) + "/" + std::to_string(b.block);
    if (!strcmp(cls, "ustep") && b.limit) s += "." + std::to_string(b.limit);
    // (k_ustep: l = the latency form, 8 rows in flight; r = one-wave class with its rows LDS-resident; #n = symbol id -- together
    // with the workgroup size they name ONE kernel symbol, so a profiler's per-symbol rows can be matched to a class)
    const bool us = !strcmp(cls, "ustep");
    return s + (b.big ? "g" : "") + (b.K > 1 ? "c" : "") + (us && b.K == 1 && b.unr == 8 ? "l" : "") + (us && b.block == 64 && b.rcap > 0 ? "r" : "") +
           (b.sym ? "#" + std::to_string(b.sym) : "");
}

// sweep / prepare classes: class 0 = one wave per user, class 1 = one 512-thread workgroup, class 2 = global scratch.
// The sweeps keep 12 B per rating in LDS.  Where to cut between "a wave per user, eight users per workgroup" and "a
// workgroup per user": a higher cut turns whole workgroups into waves (fewer workgroups to run through the CUs) but
// lengthens the one-wave chains and, past 384, the LDS of eight waves leaves 3 instead of 4 workgroups per CU.
// Cost model = rounds of workgroups through the chip x (1 + cut / 1024), over the candidate cuts (measured: ml1m 256:
// 20.4-22.7 us per sweep, 320: 19.4, 384: 20.1-21.0, 512: 25.9; 10 M-rating Netflix-shaped slice 256: 181, 512: 163).
template <typename T>
static int pick_sweep_wave_cap(const std::vector<int64_t>& uptr, int64_t nu, const std::vector<int32_t>& by_len, int ncu) {
    int sweep_wave_cap = 256;
    {
        std::vector<int64_t> lens(nu);               // ascending
        for (int64_t q = 0; q < nu; ++q) { const int32_t u = by_len[(size_t)(nu - 1 - q)]; lens[q] = uptr[u + 1] - uptr[u]; }
        const int64_t max_lds = std::upper_bound(lens.begin(), lens.end(), (int64_t)4096) - lens.begin();     // users that fit LDS
        const int64_t cap_b = max_lds > 0 ? lens[max_lds - 1] : 0;
        double best = 0.0;
        for (int c : {256, 320, 384, 448, 512}) {
            const int64_t n_wave = std::upper_bound(lens.begin(), lens.end(), (int64_t)c) - lens.begin();
            const int64_t n_blk = std::max<int64_t>(0, max_lds - n_wave);
            const size_t wave_lds = 8 * ((size_t)c * sizeof(T) + (size_t)(c + 1) * 8 + 64);
            const size_t blk_lds = n_blk > 0 ? (size_t)cap_b * sizeof(T) + (size_t)(cap_b + 1) * 8 + 1024 : 0;
            const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(4, ((size_t)160 << 10) / std::max<size_t>(1, std::max(wave_lds, blk_lds))));
            const double rounds = (double)(cdiv(n_wave, 8) + n_blk) / ((double)ncu * per_cu);
            const double cost = std::max(rounds, 1.0) * (1.0 + c / 1024.0);
            if (best == 0.0 || cost < best) { best = cost; sweep_wave_cap = c; }
        }
    }
    return sweep_wave_cap;
}

// what the U-step class layout reads: the shard's rows (CSR offsets, level-table offsets, the users longest first), the
// factor geometry, the CU count and the pcr_tune knobs
struct UstepLayoutIn {
    const std::vector<int64_t>& uptr;
    int64_t nu;
    const std::vector<int64_t>& run_ofs;
    const std::vector<int32_t>& by_len;
    int max_levels;
    int ld, nchunk, ncu;
    const std::string& ubins;
    int ustep_gram, ustep_mode, cluster_k, cluster_users, window_cache, ustep_win_lds;
};
struct UstepLayout {
    std::vector<Bin> ubins;      // the classes in launch-table order (user lists not uploaded); the cluster class, if any, is last
    size_t nsmall = 0;           // classes below 1024 ratings
    int ws = 0;                  // window-cache slots per rating (Shard::ws)
    int u_big_blocks = 0;        // scratch slices the concurrent big U-step bins need together
    int max_clusters = 1;
    size_t xch_stride = 0;       // bytes of one cluster's exchange area
    size_t bar_n = 0;            // cluster arrival counters
};
// ---- the steps of ustep_class_layout, in the order it runs them
// the classes below 1024 ratings: upper bounds, workgroup sizes, LDS residency; how many of the first are Gram classes
template <typename T>
static int ustep_short_classes(const UstepLayoutIn& in, std::vector<int>& ucap, std::vector<int>& ublk, std::vector<int>& ures, size_t& ngram, std::string& err) {
    // U step: users with more than 1024 ratings are bound by one CU's gather bandwidth -> clusters of 4 workgroups
    // The U step keeps each user's rows of V in LDS (k_ustep, stage_rows), so its occupancy is set by LDS bytes, not
    // registers: finer length classes than the V side, and a workgroup size that grows with the class.
    // pcr_tune("ubins", "cap:block:resident,...") overrides the classes below 1024.
    // Measured (ml1m shape, k = 100): residency pays for users of <= 32 ratings (13 KB of rows: 10 one-wave workgroups
    // per CU still fit); above that the LDS image costs more occupancy than the faster passes gain -- the 33..64 class
    // was resident until its non-resident form got leaner (108 VGPRs against 124): 1.622 -> 1.604 ms, 10 M-rating
    // Netflix-shaped slice 82.5 -> 80.9 ms over 4 iterations; 65..128 resident: 1.80 ms -- so those classes gather from
    // the L2s with 16 waves per CU.
    ucap = {32, 64, 128, 512}; ublk = {64, 64, 64, 256}; ures = {1, 0, 0, 0};
    if (const char* e = in.ubins.empty() ? nullptr : in.ubins.c_str()) {                 // "cap:block:resident,..."
        ucap.clear(); ublk.clear(); ures.clear();
        for (const char* q = e; *q;) {
            int c = 0, bl = 0, rs = 1, used = 0;
            if (sscanf(q, "%d:%d:%d%n", &c, &bl, &rs, &used) != 3 || (bl != 64 && bl != 256) || c < 1 || c >= 1024 || (rs && bl != 64) ||
                (!ucap.empty() && c <= ucap.back())) { err = "bad pcr_tune ubins"; return PCR_ERR_ARG; }
            ucap.push_back(c); ublk.push_back(bl); ures.push_back(rs);
            q += used; if (*q == ',') ++q;
        }
    }
    // Dual form (pcr_gram.h): users with at most gram_cap ratings run k_ustep_gram -- one class in place of the one-wave
    // classes.  gram_cap = pcr_tune("ustep_gram") or the largest count whose LDS (row image / Gram matrix + n-vectors)
    // still lets two workgroups share a CU, at most 128 (fp64: 64).
    int gram_cap = 0;
    if (in.ustep_gram != 0 && in.ubins.empty()) {
        const int hard = sizeof(T) == 4 ? 128 : 64;
        const int want = in.ustep_gram > 0 ? std::min(in.ustep_gram, hard) : GRAM_DEFAULT_CAP;
        const int nchp0 = in.nchunk | 1;
        for (int c = want; c >= 16; c -= 8)
            if (gram_bytes<T>(c, host_pow2(c), in.max_levels + 2, in.ld, nchp0, 256) <= (in.ustep_gram > 0 ? (size_t)160 : (size_t)80) * 1024) { gram_cap = c; break; }
        if (in.max_levels > 64) gram_cap = 0;              // (real-valued ratings under PrimalCR: a level per rating -- keep the general kernel)
    }
    ngram = 0;
    if (gram_cap > 64) { ucap = {64, gram_cap, 512}; ublk = {64, 256, 256}; ures = {0, 0, 0}; ngram = 2; }       // one wave up to 64 ratings
    else if (gram_cap > 0) { ucap = {gram_cap, 512}; ublk = {64, 256}; ures = {0, 0}; ngram = 1; }
    return PCR_OK;
}
static void ustep_cluster_head(const UstepLayoutIn& in, size_t nsmall, UstepLayout& out) {
    const std::vector<int64_t>& uptr = in.uptr;
    const int ncu = in.ncu;
    std::vector<Bin>& ubins = out.ubins;
    // Workgroup clusters trade throughput for latency: only the longest users of the shard (the critical path, more than
    // 1024 ratings) get them, ncu/(4K) users (all their workgroups fit the chip at once, see below) -- ONE extra class
    // whatever length class they came from (in global scratch if any of them needs it).  pcr_tune("cluster_k", "1") disables.
    int cluster_k = 4;
    if (in.cluster_k != 4) cluster_k = 1;
    out.max_clusters = std::max(1, ncu / 2);
    if (cluster_k > 1) {
        Bin head;
        head.block = 512; head.K = cluster_k;
        // ncu / (4K) users = a quarter of the CUs: every cluster workgroup keeps a CU to itself (its LDS image) for the
        // whole launch, CUs the many short users cannot use meanwhile -- ml1m: 8 users 1.610 ms, 12-20: 1.59-1.61, 24: 1.63,
        // 32: 1.645, 48: 1.79 per iteration; 10 M-rating Netflix-shaped slice: U step 7.24 (32) -> 6.98 ms (16)
        size_t budget = (size_t)std::max(1, ncu / (4 * cluster_k));
        if (in.cluster_users > 0) budget = (size_t)std::max(1, std::min(in.cluster_users, ncu / cluster_k));
        for (size_t q = ubins.size(); q-- > nsmall + 1 && budget > 0;) {       // longest class first; users are sorted longest first
            Bin& b = ubins[q];
            const size_t take = std::min(budget, b.users.size());
            if (take == 0) continue;
            budget -= take;
            head.big = head.big || b.big;
            head.max_lev = std::max(head.max_lev, b.max_lev);
            for (size_t i = 0; i < take; ++i) {
                const int32_t u = b.users[i];
                const int64_t len = uptr[u + 1] - uptr[u];
                head.users.push_back(u); head.nnz += len; head.cap = std::max<int>(head.cap, (int)len);
                b.nnz -= len;
            }
            b.users.erase(b.users.begin(), b.users.begin() + take);
            b.cap = b.users.empty() ? 0 : (int)(uptr[b.users[0] + 1] - uptr[b.users[0]]);
        }
        if (!head.users.empty()) ubins.push_back(std::move(head));
    }
}
template <typename T>
static void ustep_lds_images(const UstepLayoutIn& in, const std::vector<int>& ures, UstepLayout& out) {
    const size_t nsmall = out.nsmall;
    std::vector<Bin>& ubins = out.ubins;
    // window cache (pcr_kernels.h, Shard::win): one slot per other level, up to 9 levels
    out.ws = (in.window_cache && in.max_levels >= 2 && in.max_levels <= 9) ? in.max_levels - 1 : 0;
    {   // LDS residency: what is left of the 160 KB after the r-vectors and the per-rating arrays, in rows of V
        const int nchp = in.nchunk | 1;
        // (capping the image at 128 / 112 / 96 / 64 KB, so that workgroups of the short classes could share the CU, changes
        // nothing: ml1m 1.424-1.438 ms per step at every cap, Netflix-shaped U step 62.6-62.8 ms -- NOTES.md round 4)
        const size_t lim = 160 * 1024;
        for (size_t bi = 0; bi < ubins.size(); ++bi) {
            Bin& b = ubins[bi];
            if (b.users.empty() || b.gram) continue;
            // the LDS image pays where LDS is spare: the one-wave classes of <= 64 ratings, and the latency-bound
            // 512-thread classes (one workgroup per CU anyway), which keep as many rows as fit beside their arrays
            const int res_on = bi < nsmall ? (b.block == 64 ? ures[bi] : 0) : (b.unr == 8);
            // the window rows of the class's longest user in LDS (16 bit), where that still leaves the class its occupancy:
            // every class of at most 1024 ratings (8 KB), the one-workgroup-per-CU classes whatever their length
            b.wcap = 0;
            if (in.ustep_win_lds && !b.big && out.ws > 0 && (b.cap <= 1024 || b.unr == 8) &&
                ustep_small_bytes(in.ld, b.block, sizeof(T)) + ustep_big_bytes<T>(b.cap, host_pow2(b.cap), b.max_lev + 2, 4) +
                    carve_bytes((size_t)b.cap * out.ws, 2) <= lim - 8 * 1024)
                b.wcap = b.cap * out.ws;
            const size_t fixed = ustep_small_bytes(in.ld, b.block, sizeof(T)) + carve_bytes(b.wcap, 2) +
                                 (b.big ? 0 : ustep_big_bytes<T>(b.cap, host_pow2(b.cap), b.max_lev + 2, 4));
            const int64_t room = fixed < lim ? (int64_t)((lim - fixed) / ((size_t)nchp * 16)) : 0;
            const int64_t want = (b.cap + b.K - 1) / b.K;                  // longest slice a member gathers
            b.rcap = res_on ? (int)std::max<int64_t>(0, std::min(room, want)) : 0;
        }
    }
}
template <typename T>
static void ustep_symbols(const UstepLayoutIn& in, std::vector<Bin>& ubins) {
    {   // two length classes that run the same workgroup form get kernel symbols of their own (k_ustep's CLS), so that
        // rocprofv3's per-symbol durations and PMC bytes belong to one class each
        std::map<std::string, int> seen;
        for (auto& b : ubins) {
            if (b.users.empty() || b.gram) continue;
            const std::string key = std::to_string(b.block) + (b.big ? "g" : "") + "k" + std::to_string(b.K) + (b.rcap > 0 ? "r" : "") + "u" + std::to_string(b.unr);
            const bool two = !b.big && b.K == 1 && b.rcap == 0 && b.unr == 4;       // the forms instantiated twice (set_lds_limits)
            b.sym = two ? (seen[key]++ & 1) : 0;
            // the 512-thread throughput form: symbol 0 is the register-capped one (two workgroups per CU), compiled for at most
            // half a CU's LDS; a class that needs more LDS than that takes symbol 1 (pcr_kernels.h, k_ustep)
            if (two && b.block == 512 && sizeof(T) == 4)
                b.sym = ustep_small_bytes(in.ld, b.block, sizeof(T)) + carve_bytes(b.wcap, 2) + ustep_big_bytes<T>(b.cap, host_pow2(b.cap), b.max_lev + 2, 4) > (size_t)80 * 1024 ? 1 : 0;
        }
    }
}

template <typename T>
static int ustep_class_layout(const UstepLayoutIn& in, UstepLayout& out, std::string& err) {
    const std::vector<int64_t>& uptr = in.uptr;
    const int64_t nu = in.nu;
    const int ncu = in.ncu;
    std::vector<Bin>& ubins = out.ubins;
    std::vector<int> ucap, ublk, ures;
    size_t ngram = 0;
    RC(ustep_short_classes<T>(in, ucap, ublk, ures, ngram, err));
    const size_t nsmall = out.nsmall = ucap.size();
    // Latency or throughput?  A class with few users is one round of workgroups and is bound by the per-user dependency
    // chain: 512 threads, 8 rows in flight per lane group, 174-205 VGPRs = one workgroup per CU.  A class with many users
    // is bound by how busy each CU's memory pipe stays: smaller / leaner workgroups, so that two share a CU and one
    // gathers while the other scans or sorts (<= 1024 ratings: 256 threads; above: 512 threads at 4 rows in flight =
    // 124 VGPRs, and a class boundary at 2048 so that the per-rating arrays of two fit the LDS).  "Many" is more than
    // CUs/4 users: the greedy one-per-CU workgroups of all long classes together must leave CUs for the short classes
    // (ml1m: 88 + 221 users in throughput form 2.09 -> 2.03 ms per iteration; Netflix shape: U step 87 -> 69 ms).
    const int force_mode = in.ustep_mode;                                                  // 1 latency, 2 throughput
    const int64_t many_users = std::max<int64_t>(1, ncu / 4);
    auto many = [&](int64_t users) { return force_mode ? force_mode == 2 : users > many_users; };
    int64_t n_mid = 0;
    for (int64_t u = 0; u < nu; ++u) { const int64_t len = uptr[u + 1] - uptr[u]; n_mid += len > 1024 && len <= 4096; }
    ucap.push_back(1024); ublk.push_back(512);
    if (many(n_mid)) { ucap.push_back(2048); ublk.push_back(512); }
    ucap.push_back(4096); ublk.push_back(512); ublk.push_back(512);
    make_bins(uptr, nu, &in.run_ofs, ubins, in.by_len, ucap, ublk);
    for (size_t q = 0; q < ngram; ++q) ubins[q].gram = true;
    ustep_cluster_head(in, nsmall, out);
    for (size_t q = nsmall; q < ubins.size(); ++q) {
        Bin& b = ubins[q];
        // (a class whose per-rating arrays fill more than half the LDS runs one workgroup per CU whatever its register
        // count: it keeps the 8-rows-in-flight form)
        const bool lds_bound = !b.big && ustep_big_bytes<T>(b.cap, host_pow2(b.cap), b.max_lev + 2, 4) > 72 * 1024;
        if (b.K > 1 || lds_bound || !many((int64_t)b.users.size())) { b.unr = 8; continue; }
        b.unr = 4;
        // (re-checked in round 3 for a 513..1024 class of 200 users, one round of workgroups: 256 threads at 8 rows in flight
        // 1.49 -> 1.69 ms per ml1m step, 512 threads at 4 rows: no change)
        if (b.limit == 1024 && !b.big) b.block = 256;
    }
    // A class whose per-rating arrays + r-vectors do not fit the 160 KB of LDS (fp64 at wide ranks with users near 4096
    // ratings, or thousands of rating levels under PrimalCR) runs the global-scratch form of the kernel instead.
    for (auto& b : ubins) {
        if (b.big || b.users.empty() || b.gram) continue;
        const size_t fixed = ustep_small_bytes(in.ld, b.block, sizeof(T)) + ustep_big_bytes<T>(b.cap, host_pow2(b.cap), b.max_lev + 2, 4);
        if (fixed > (size_t)160 * 1024) { b.big = true; b.block = 512; }
    }
    // the one-wave and 256-thread classes keep 4 rows in flight per lane group (8 measured on ml1m: the one-wave classes alone
    // 1.58 -> 1.67 ms per step, the 256-thread classes too 1.89 ms; Netflix shape U step 52 -> 68 ms: the registers cost more
    // occupancy than the deeper gathers gain)
    for (size_t q = 0; q < nsmall && q < ubins.size(); ++q)
        if (!ubins[q].gram && !ubins[q].users.empty()) ubins[q].unr = 4;
    out.u_big_blocks = 0;
    for (auto& b : ubins) {
        const int nus = (int)b.users.size();
        b.ugrid = b.K > 1 ? std::min(nus, std::max(1, ncu / b.K)) * b.K : (b.big ? std::min(nus, 2 * ncu) : nus);
        if (b.big) { b.scratch_ofs = out.u_big_blocks; out.u_big_blocks += b.ugrid; }
    }
    ustep_lds_images<T>(in, ures, out);
    {
        size_t need_x = 0;
        for (auto& b : ubins)
            if (b.K > 1 && !b.users.empty()) need_x = std::max(need_x, ustep_xch_bytes<T>(host_pow2(b.cap), in.ld, b.K));
        out.xch_stride = (need_x + 255) & ~(size_t)255;
        out.bar_n = (size_t)out.max_clusters * ubins.size();               // the classes run concurrently: one set per class
    }
    ustep_symbols<T>(in, ubins);
    return PCR_OK;
}
