// classes_dump.hip -- prints the U step's length-class layout (pcr_classes.h) of one case, on the host: no device is opened.
// tests/test_classes.py compares its output with what solvers on the GPU reported (tests/golden/ustep_classes.json).
//
//   classes_dump CASE
//
// CASE is a text file: one line of key=value pairs -- precision (f32 | f64), ld, ncu, users, and any of the knobs ubins, ustep_gram,
// ustep_mode, cluster_k, cluster_users, window_cache, ustep_win_lds (pcr_tune's defaults otherwise) -- then one line
// "ratings levels" per user.  Output: one "class" line per class of the layout in table order (empty ones included), then the
// scalar outputs and the V side's sweep_wave_cap.  A layout the solver would refuse prints "error <code> <text>" and exits 2.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pcr_kernels.h"
#include "pcr_gram.h"
#include "pcr_classes.h"

struct Case {
    std::string precision = "f64", ubins;
    int ld = 0, ncu = 256, ustep_gram = -1, ustep_mode = 0, cluster_k = 4, cluster_users = 0, window_cache = 1, ustep_win_lds = 1;
    std::vector<int64_t> uptr{0}, run_ofs{0};
    int max_levels = 0;
};

template <typename T>
static int dump(const Case& c) {
    const int64_t nu = (int64_t)c.uptr.size() - 1;
    std::vector<int32_t> by_len;
    length_order(c.uptr, nu, by_len);
    UstepLayout L;
    std::string err;
    const int rc = ustep_class_layout<T>({c.uptr, nu, c.run_ofs, by_len, c.max_levels, c.ld, c.ld / VecOf<T>::N, c.ncu, c.ubins, c.ustep_gram, c.ustep_mode,
                                          c.cluster_k, c.cluster_users, c.window_cache, c.ustep_win_lds}, L, err);
    if (rc != PCR_OK) { printf("error %d %s\n", rc, err.c_str()); return 2; }
    for (const Bin& b : L.ubins)
        printf("class %s limit=%d block=%d big=%d K=%d ugrid=%d scratch_ofs=%d cap=%d rcap=%d unr=%d gram=%d wcap=%d sym=%d max_lev=%d nnz=%" PRId64
               " users=%zu first=%d last=%d\n", pname("ustep", b).c_str(), b.limit, b.block, (int)b.big, b.K, b.ugrid, b.scratch_ofs, b.cap, b.rcap, b.unr,
               (int)b.gram, b.wcap, b.sym, b.max_lev, b.nnz, b.users.size(), b.users.empty() ? -1 : (int)b.users.front(), b.users.empty() ? -1 : (int)b.users.back());
    printf("nsmall=%zu ws=%d u_big_blocks=%d max_clusters=%d xch_stride=%zu bar_n=%zu\n", L.nsmall, L.ws, L.u_big_blocks, L.max_clusters, L.xch_stride, L.bar_n);
    printf("sweep_wave_cap=%d\n", pick_sweep_wave_cap<T>(c.uptr, nu, by_len, c.ncu));
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: classes_dump CASE\n"); return 1; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 1; }
    Case c;
    long users = -1;
    char line[4096];
    if (!fgets(line, sizeof line, f)) { fprintf(stderr, "%s: empty\n", argv[1]); return 1; }
    for (char* tok = strtok(line, " \n"); tok; tok = strtok(nullptr, " \n")) {
        char* eq = strchr(tok, '=');
        if (!eq) { fprintf(stderr, "not key=value: %s\n", tok); return 1; }
        const std::string key(tok, eq), val(eq + 1);
        const std::pair<const char*, int*> ints[] = {{"ld", &c.ld}, {"ncu", &c.ncu}, {"ustep_gram", &c.ustep_gram}, {"ustep_mode", &c.ustep_mode},
                                                     {"cluster_k", &c.cluster_k}, {"cluster_users", &c.cluster_users}, {"window_cache", &c.window_cache},
                                                     {"ustep_win_lds", &c.ustep_win_lds}};
        bool known = true;
        if (key == "precision") c.precision = val;
        else if (key == "ubins") c.ubins = val;
        else if (key == "users") users = atol(val.c_str());
        else {
            known = false;
            for (auto& kv : ints) if (key == kv.first) { *kv.second = atoi(val.c_str()); known = true; }
        }
        if (!known) { fprintf(stderr, "unknown key: %s\n", key.c_str()); return 1; }
    }
    if ((c.precision != "f32" && c.precision != "f64") || c.ld < 4 || c.ld % 4 || c.ncu < 1 || users < 0) { fprintf(stderr, "bad case header\n"); return 1; }
    for (long u = 0; u < users; ++u) {
        long long len = 0, lev = 0;
        if (fscanf(f, "%lld %lld", &len, &lev) != 2 || len < 0 || lev < 0 || lev > len) { fprintf(stderr, "bad user line %ld\n", u); return 1; }
        c.uptr.push_back(c.uptr.back() + len);
        c.run_ofs.push_back(c.run_ofs.back() + lev + 1);        // (PcrLevels::run_ofs: T_u + 1 slots per user)
        c.max_levels = std::max(c.max_levels, (int)lev);
    }
    fclose(f);
    return c.precision == "f32" ? dump<float>(c) : dump<double>(c);
}
