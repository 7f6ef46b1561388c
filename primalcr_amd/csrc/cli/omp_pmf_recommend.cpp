// omp-pmf-recommend -- top-K unrated items per user from a model file (pcr_recommend_model, include/primalcr.h).  The reference
// has no counterpart: pmf-predict.cpp scores the pairs of a test file only.
//   omp-pmf-recommend [-K topk] [-x data_dir] [-u users_file] [--f32] [--scores] model_file output_file
//     -K topk       items per user (default 10, at most PCR_RECOMMEND_MAX_K)
//     -x data_dir   leave out the training ratings of a data directory (its meta file; d1 / d2 must match the model)
//     -u users_file one 1-based user id per line (default: every user of the model)
//     --f32         score with f32 factors (default: fp64, as the model file holds them)
//     --scores      write every item as item:score (score in "%lf", as omp-pmf-predict prints it)
// Output: one line per user, in input order: the 1-based user id, then the 1-based item ids (padding is left out).  Users go
// to the device in batches, so host memory for the lists stays bounded on any catalogue.
#include <algorithm>
#include <cerrno>
#include <charconv>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <unistd.h>

#include "primalcr.h"

static const char* USAGE =
    "Usage: omp-pmf-recommend [-K topk] [-x data_dir] [-u users_file] [--f32] [--scores] model_file output_file\n"
    "    -K topk       items per user (default 10, 1 .. 1024)\n"
    "    -x data_dir   leave out the training ratings of this data directory (meta file)\n"
    "    -u users_file one 1-based user id per line (default: every user)\n"
    "    --f32         score in f32 (default fp64)\n"
    "    --scores      write item:score instead of item\n";

static int usage() { printf("%s", USAGE); return 1; }

// one 1-based id per line (blank lines skipped); 0-based ids into `out`
static bool read_users(const char* path, int64_t d1, std::vector<int32_t>& out) {
    FILE* fp = fopen(path, "r");
    if (!fp) { fprintf(stderr, "can't open users file %s\n", path); return false; }
    char line[256];
    int64_t ln = 0;
    bool ok = true;
    while (fgets(line, sizeof line, fp)) {
        ++ln;
        char* p = line;
        while (*p == ' ' || *p == '\t') ++p;
        if (*p == '\n' || *p == '\r' || *p == 0) continue;
        errno = 0;
        char* end = nullptr;
        const long long v = strtoll(p, &end, 10);
        while (end && (*end == ' ' || *end == '\t' || *end == '\r' || *end == '\n')) ++end;
        if (end == p || errno || !end || *end != 0) { fprintf(stderr, "users file %s, line %lld: not a user id\n", path, (long long)ln); ok = false; break; }
        if (v < 1 || v > d1) { fprintf(stderr, "users file %s, line %lld: user %lld outside 1 .. %lld\n", path, (long long)ln, v, (long long)d1); ok = false; break; }
        out.push_back((int32_t)(v - 1));
    }
    fclose(fp);
    return ok;
}

int main(int argc, char** argv) {
    int K = 10;
    bool f32 = false, with_scores = false;
    const char *xdir = nullptr, *ufile = nullptr;
    std::vector<const char*> pos;
    for (int i = 1; i < argc; ++i) {
        const char* a = argv[i];
        if (!strcmp(a, "-K") || !strcmp(a, "-x") || !strcmp(a, "-u")) {
            if (i + 1 >= argc) return usage();
            const char* v = argv[++i];
            if (a[1] == 'K') {
                char* end = nullptr;
                const long x = strtol(v, &end, 10);
                if (!*v || *end || x < 1 || x > PCR_RECOMMEND_MAX_K) { fprintf(stderr, "-K %s: must be an integer in 1 .. %d\n", v, PCR_RECOMMEND_MAX_K); return 1; }
                K = (int)x;
            } else if (a[1] == 'x') xdir = v;
            else ufile = v;
        } else if (!strcmp(a, "--f32")) f32 = true;
        else if (!strcmp(a, "--scores")) with_scores = true;
        else if (a[0] == '-' && a[1]) { fprintf(stderr, "unknown option %s\n", a); return usage(); }
        else pos.push_back(a);
    }
    if (pos.size() != 2) return usage();
    int64_t d1, d2, k;
    if (pcr_model_load(pos[0], &d1, &d2, &k, nullptr, nullptr) != PCR_OK) { fprintf(stderr, "can't open model file %s\n", pos[0]); return 1; }
    std::vector<double> U((size_t)d1 * k), V((size_t)d2 * k);
    if (pcr_model_load(pos[0], &d1, &d2, &k, U.data(), V.data()) != PCR_OK) { fprintf(stderr, "%s\n", pcr_last_error()); return 1; }
    std::vector<int32_t> users;
    if (ufile) { if (!read_users(ufile, d1, users)) return 1; }
    else { users.resize((size_t)d1); for (int64_t u = 0; u < d1; ++u) users[(size_t)u] = (int32_t)u; }
    std::vector<int64_t> xindex;
    std::vector<int32_t> xitem;
    if (xdir) {
        pcr_dataset* ds = nullptr;
        if (pcr_dataset_load_mt(xdir, 0, &ds) != PCR_OK) { fprintf(stderr, "%s\n", pcr_last_error()); return 1; }
        int64_t xd1, xd2, nnz, tnnz;
        pcr_dataset_dims(ds, &xd1, &xd2, &nnz, &tnnz);
        if (xd1 != d1 || xd2 != d2) {
            fprintf(stderr, "data set %s is %lld x %lld, the model %lld x %lld\n", xdir, (long long)xd1, (long long)xd2, (long long)d1, (long long)d2);
            pcr_dataset_free(ds);
            return 1;
        }
        xindex.resize((size_t)d1 + 1);
        std::vector<int64_t> it64((size_t)nnz);
        pcr_dataset_csr(ds, 0, xindex.data(), it64.data(), nullptr);
        pcr_dataset_free(ds);
        xitem.assign(it64.begin(), it64.end());
    }
    FILE* out_fp = fopen(pos[1], "wb");
    if (!out_fp) { fprintf(stderr, "can't open output file %s\n", pos[1]); return 1; }
    const int64_t n = (int64_t)users.size();
    const int64_t batch = std::max<int64_t>(1, ((int64_t)1 << 22) / K);   // 4 M list entries per call
    std::vector<int32_t> items;
    std::vector<double> scores;
    std::string o;
    bool ok = true;
    for (int64_t b0 = 0; b0 < n && ok; b0 += batch) {
        const int64_t m = std::min(batch, n - b0);
        items.resize((size_t)(m * K)); scores.resize((size_t)(m * K));
        if (pcr_recommend_model(U.data(), d1, V.data(), d2, k, xdir ? xindex.data() : nullptr, xdir ? xitem.data() : nullptr, m, users.data() + b0, K,
                                f32 ? PCR_F32 : PCR_F64, items.data(), scores.data(), 0) != PCR_OK) {
            fprintf(stderr, "recommend: %s\n", pcr_last_error());
            fclose(out_fp);
            return 1;
        }
        o.resize((size_t)(m * (12 + (int64_t)K * (with_scores ? 348 : 12))));
        char* p = &o[0];
        for (int64_t i = 0; i < m; ++i) {
            p = std::to_chars(p, p + 12, (long long)users[(size_t)(b0 + i)] + 1).ptr;
            for (int e = 0; e < K; ++e) {
                const int32_t j = items[(size_t)(i * K + e)];
                if (j < 0) break;
                *p++ = ' ';
                p = std::to_chars(p, p + 12, (long long)j + 1).ptr;
                if (with_scores) { *p++ = ':'; p = std::to_chars(p, p + 334, scores[(size_t)(i * K + e)], std::chars_format::fixed, 6).ptr; }
            }
            *p++ = '\n';
        }
        ok = fwrite(o.data(), 1, (size_t)(p - o.data()), out_fp) == (size_t)(p - o.data());
    }
    ok = (fclose(out_fp) == 0) && ok;
    if (!ok) { fprintf(stderr, "short write to %s\n", pos[1]); return 1; }
    fflush(stdout); fflush(stderr);
    _exit(0);
}
