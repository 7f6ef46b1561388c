// sanitize/device_absent.cpp -- SANITIZER BUILDS ONLY (make -C primalcr_amd/csrc asan): never part of libprimalcr.so.
//
// AddressSanitizer / UBSan run on the CPU build only (GPU sanitizers are not available on this pool), so the sanitized
// library is pcr_host.cpp (loader, parser, cache, partitioner, model file, knob table) + the CLIs' host paths built with g++
// -fsanitize=address,undefined and NO HIP object.  The [device] entry points of include/primalcr.h must still resolve; here
// every one of them does what the real library does on a box without a GPU: set the error message and return
// PCR_ERR_DEVICE.  Nothing is computed -- this is not a CPU path.
#include <cstring>
#include <string>

#include "pcr_host.h"

struct pcr_solver { int unused; };

static int absent() {
    pcr_set_error("no HIP device available: libprimalcr has no CPU fallback for the training path (sanitizer build: host code only)");
    return PCR_ERR_DEVICE;
}

extern "C" {
int pcr_solver_create(const pcr_dataset* ds, const pcr_params* p, int rank, int nranks, pcr_solver** out) {
    if (!ds || !p || !out || nranks < 1 || rank < 0 || rank >= nranks) { pcr_set_error("pcr_solver_create: bad argument"); return PCR_ERR_ARG; }
    return absent();
}
int pcr_solver_create_shard(const pcr_dataset* ds, const pcr_params* p, int rank, int nranks, int64_t first_user, int64_t, pcr_solver** out) {
    if (!ds || !p || !out || nranks < 1 || rank < 0 || rank >= nranks || first_user < 0) { pcr_set_error("pcr_solver_create_shard: bad argument"); return PCR_ERR_ARG; }
    return absent();
}
void pcr_solver_destroy(pcr_solver*) {}
int pcr_device_warmup(int) { return absent(); }
int pcr_comm_unique_id(void* id128) { if (!id128) { pcr_set_error("null id"); return PCR_ERR_ARG; } return absent(); }
#define NO_SOLVER(name, ...) int name(__VA_ARGS__) { pcr_set_error("null solver"); return PCR_ERR_ARG; }
NO_SOLVER(pcr_solver_comm_init, pcr_solver*, const void*)
NO_SOLVER(pcr_solver_comm_init_p2p, pcr_solver*, const char*)
int pcr_solver_comm_nranks(pcr_solver*) { return -1; }
NO_SOLVER(pcr_solver_counter, pcr_solver*, const char*, double*)
NO_SOLVER(pcr_solver_set_ccd_params, pcr_solver*, const pcr_ccd_params*)
NO_SOLVER(pcr_solver_ustep_classes, pcr_solver*, char*, int64_t)
NO_SOLVER(pcr_solver_setup_phase, const pcr_solver*, int, const char**, double*)
NO_SOLVER(pcr_solver_set_local_only, pcr_solver*, int)
NO_SOLVER(pcr_solver_shard, const pcr_solver*, int64_t*, int64_t*, int64_t*)
NO_SOLVER(pcr_solver_set_factors, pcr_solver*, const double*, const double*)
NO_SOLVER(pcr_solver_get_factors, pcr_solver*, double*, double*)
NO_SOLVER(pcr_solver_set_factors_local, pcr_solver*, const double*, const double*)
NO_SOLVER(pcr_solver_set_user_weights, pcr_solver*, const double*)
NO_SOLVER(pcr_solver_set_user_weights_local, pcr_solver*, const double*)
NO_SOLVER(pcr_solver_set_rating_weights, pcr_solver*, const double*)
NO_SOLVER(pcr_solver_set_implicit, pcr_solver*, double)
NO_SOLVER(pcr_solver_get_factors_local, pcr_solver*, double*, double*)
NO_SOLVER(pcr_comp_m, pcr_solver*, double*)
NO_SOLVER(pcr_objective, pcr_solver*, double*)
NO_SOLVER(pcr_obtain_g, pcr_solver*, double*)
NO_SOLVER(pcr_compute_Ha, pcr_solver*, const double*, double*)
NO_SOLVER(pcr_solve_delta, pcr_solver*, const double*, double*, int*)
NO_SOLVER(pcr_update_V, pcr_solver*, double*, int*)
NO_SOLVER(pcr_update_U, pcr_solver*, double*, int64_t*)
NO_SOLVER(pcr_evaluate, pcr_solver*, int, int, double*, double*)
NO_SOLVER(pcr_train, pcr_solver*, pcr_log_fn, void*, pcr_iter_stats*)
NO_SOLVER(pcr_iterate, pcr_solver*, int, pcr_iter_stats*)
NO_SOLVER(pcr_solver_sync, pcr_solver*)
NO_SOLVER(pcr_profile_enable, pcr_solver*, int)
NO_SOLVER(pcr_profile_list, pcr_solver*, char*, int64_t)
NO_SOLVER(pcr_profile_get, pcr_solver*, const char*, double*, int64_t*)
NO_SOLVER(pcr_profile_launches, pcr_solver*, const char*, int64_t*)
NO_SOLVER(pcr_profile_scope, pcr_solver*, const char*, int64_t*, int64_t*)
NO_SOLVER(pcr_profile_reset, pcr_solver*)
int pcr_predict(const double* U, int64_t, const double* V, int64_t, int64_t k, int64_t n, const int32_t* user, const int32_t* item, double* pred, int) {
    if (!U || !V || k < 1 || n < 0 || (n > 0 && (!user || !item || !pred))) { pcr_set_error("pcr_predict: bad argument"); return PCR_ERR_ARG; }
    return absent();
}
int pcr_recommend_model(const double* U, int64_t d1, const double* V, int64_t d2, int64_t k, const int64_t* index, const int32_t* item,
                        int64_t n, const int32_t* users, int topk, int dtype, int32_t* items, double* scores, int) {
    const int rc = pcr_recommend_model_check(U, d1, V, d2, k, index, item, n, users, topk, dtype, items, scores, nullptr);
    return rc != PCR_OK ? rc : absent();
}
NO_SOLVER(pcr_recommend, pcr_solver*, int64_t, const int32_t*, int, int, int32_t*, double*)
int pcr_recommend_filtered_model(const double* U, int64_t d1, const double* V, int64_t d2, int64_t k, const int64_t* index, const int32_t* item,
                                 int64_t n, const int32_t* users, int topk, int dtype, const pcr_item_filter* f, int32_t* items, double* scores, int) {
    const int rc = pcr_recommend_filtered_model_check(U, d1, V, d2, k, index, item, n, users, topk, dtype, f, items, scores, nullptr);
    return rc != PCR_OK ? rc : absent();
}
NO_SOLVER(pcr_recommend_filtered, pcr_solver*, int64_t, const int32_t*, int, int, const pcr_item_filter*, int32_t*, double*)
int pcr_evaluate_topn_model(const double* U, int64_t d1, const double* V, int64_t d2, int64_t k, const int64_t* index, const int32_t* item,
                            const int64_t* tindex, const int32_t* titem, const double* tval, int ncut, const int* cutoffs, double threshold,
                            int dtype, pcr_topn_stats* stats, double*, int) {
    const int rc = pcr_evaluate_topn_model_check(U, d1, V, d2, k, index, item, tindex, titem, tval, ncut, cutoffs, threshold, dtype, stats, nullptr);
    return rc != PCR_OK ? rc : absent();
}
NO_SOLVER(pcr_evaluate_topn, pcr_solver*, int, const int*, double, int, pcr_topn_stats*, double*)
int pcr_evaluate_ranks_model(const double* U, int64_t d1, const double* V, int64_t d2, int64_t k, const int64_t* index, const int32_t* item,
                             const int64_t* tindex, const int32_t* titem, const double* tval, double threshold, int dtype,
                             pcr_rank_stats* stats, double*, int64_t*, int) {
    const int rc = pcr_evaluate_ranks_model_check(U, d1, V, d2, k, index, item, tindex, titem, tval, threshold, dtype, stats, nullptr);
    return rc != PCR_OK ? rc : absent();
}
NO_SOLVER(pcr_evaluate_ranks, pcr_solver*, double, int, pcr_rank_stats*, double*, int64_t*)
int pcr_evaluate_topn_filtered_model(const double* U, int64_t d1, const double* V, int64_t d2, int64_t k, const int64_t* index, const int32_t* item,
                                     const int64_t* tindex, const int32_t* titem, const double* tval, int ncut, const int* cutoffs, double threshold,
                                     int dtype, const pcr_item_filter* f, pcr_topn_stats* stats, double*, int) {
    int rc = pcr_evaluate_topn_model_check(U, d1, V, d2, k, index, item, tindex, titem, tval, ncut, cutoffs, threshold, dtype, stats, nullptr,
                                           "pcr_evaluate_topn_filtered_model");
    if (rc == PCR_OK) rc = pcr_eval_filter_check("pcr_evaluate_topn_filtered_model", "pcr_evaluate_topn_model", d2, d1, f);
    return rc != PCR_OK ? rc : absent();
}
NO_SOLVER(pcr_evaluate_topn_filtered, pcr_solver*, int, const int*, double, int, const pcr_item_filter*, pcr_topn_stats*, double*)
int pcr_evaluate_ranks_filtered_model(const double* U, int64_t d1, const double* V, int64_t d2, int64_t k, const int64_t* index, const int32_t* item,
                                      const int64_t* tindex, const int32_t* titem, const double* tval, double threshold, int dtype,
                                      const pcr_item_filter* f, pcr_rank_stats* stats, double*, int64_t*, int) {
    int rc = pcr_evaluate_ranks_model_check(U, d1, V, d2, k, index, item, tindex, titem, tval, threshold, dtype, stats, nullptr,
                                            "pcr_evaluate_ranks_filtered_model");
    if (rc == PCR_OK) rc = pcr_eval_filter_check("pcr_evaluate_ranks_filtered_model", "pcr_evaluate_ranks_model", d2, d1, f);
    return rc != PCR_OK ? rc : absent();
}
NO_SOLVER(pcr_evaluate_ranks_filtered, pcr_solver*, double, int, const pcr_item_filter*, pcr_rank_stats*, double*, int64_t*)
int pcr_evaluate_diversity_model(const double* U, int64_t d1, const double* V, int64_t d2, int64_t k, const int64_t* index, const int32_t* item,
                                 int64_t n, const int32_t* users, int ncut, const int* cutoffs, int dtype, pcr_diversity_stats* stats, double*,
                                 int64_t*, int) {
    const int rc = pcr_evaluate_diversity_model_check(U, d1, V, d2, k, index, item, n, users, ncut, cutoffs, dtype, stats, nullptr);
    return rc != PCR_OK ? rc : absent();
}
NO_SOLVER(pcr_evaluate_diversity, pcr_solver*, int64_t, const int32_t*, int, const int*, int, pcr_diversity_stats*, double*, int64_t*)
int pcr_recommend_diverse_model(const double* U, int64_t d1, const double* V, int64_t d2, int64_t k, const int64_t* index, const int32_t* item,
                                int64_t n, const int32_t* users, int topk, int pool, double theta, int dtype, int32_t* items, double* scores, int) {
    const int rc = pcr_recommend_diverse_model_check(U, d1, V, d2, k, index, item, n, users, topk, pool, theta, dtype, items, scores, nullptr);
    return rc != PCR_OK ? rc : absent();
}
NO_SOLVER(pcr_recommend_diverse, pcr_solver*, int64_t, const int32_t*, int, int, double, int, int32_t*, double*)
int pcr_recommend_capped_model(const double* U, int64_t d1, const double* V, int64_t d2, int64_t k, const int64_t* index, const int32_t* item,
                               int64_t n, const int32_t* users, int topk, int pool, const int32_t* group, int cap, int dtype,
                               const pcr_item_filter* f, int32_t* items, double* scores, uint8_t*, pcr_cap_stats*, int) {
    const int rc = pcr_recommend_capped_model_check(U, d1, V, d2, k, index, item, n, users, topk, pool, group, cap, dtype, f, items, scores, nullptr);
    return rc != PCR_OK ? rc : absent();
}
NO_SOLVER(pcr_recommend_capped, pcr_solver*, int64_t, const int32_t*, int, int, const int32_t*, int, int, const pcr_item_filter*, int32_t*, double*,
          uint8_t*, pcr_cap_stats*)
int pcr_evaluate_lists_model(const double* V, int64_t d2, int64_t k, int64_t d1, const int64_t* index, const int32_t* item, const int64_t* tindex,
                             const int32_t* titem, const double* tval, int64_t n, const int32_t* users, int L, const int32_t* lists, int ncut,
                             const int* cutoffs, double threshold, int dtype, pcr_topn_stats* topn, double* per_user_topn,
                             pcr_diversity_stats* div, double*, int64_t*, int) {
    const int rc = pcr_evaluate_lists_model_check(V, d2, k, d1, index, item, tindex, titem, tval, n, users, L, lists, ncut, cutoffs, threshold,
                                                  dtype, topn, per_user_topn, div);
    return rc != PCR_OK ? rc : absent();
}
int pcr_evaluate_rerank_model(const double* U, int64_t d1, const double* V, int64_t d2, int64_t k, const int64_t* index, const int32_t* item,
                              const int64_t* tindex, const int32_t* titem, const double* tval, int64_t n, const int32_t* users, int nth,
                              const double* thetas, int pool, int ncut, const int* cutoffs, double threshold, int dtype, pcr_topn_stats* topn,
                              pcr_diversity_stats* div, double* per_user_topn, double*, int64_t*, int) {
    const int rc = pcr_evaluate_rerank_model_check(U, d1, V, d2, k, index, item, tindex, titem, tval, n, users, nth, thetas, pool, ncut, cutoffs,
                                                   threshold, dtype, topn, per_user_topn, div, nullptr);
    return rc != PCR_OK ? rc : absent();
}
int pcr_fold_in_model(const pcr_params* p, const double* V, int64_t d2, int64_t n, const int64_t* index, const int32_t* item, const double* val,
                      const double*, int steps, double* U_out, pcr_foldin_stats*, double*) {
    const int rc = pcr_fold_in_model_check(p, V, d2, n, index, item, val, steps, U_out, nullptr);
    return rc != PCR_OK ? rc : absent();
}
NO_SOLVER(pcr_fold_in, pcr_solver*, int64_t, const int64_t*, const int32_t*, const double*, const double*, int, double*, pcr_foldin_stats*, double*)
int pcr_fold_in_ridge_model(const double* F, int64_t rows, int64_t k, double lambda, int, int precision, int, int64_t n, const int64_t* index,
                            const int32_t* item, const double* val, double* U_out, pcr_ridge_stats*, double*) {
    const int rc = pcr_fold_in_ridge_check("pcr_fold_in_ridge_model", true, F, rows, k, lambda, precision, n, index, item, val, U_out, nullptr);
    return rc != PCR_OK ? rc : absent();
}
NO_SOLVER(pcr_fold_in_ridge, pcr_solver*, int, int64_t, const int64_t*, const int32_t*, const double*, double*, pcr_ridge_stats*, double*)
int pcr_fold_in_conf_model(const double* F, int64_t rows, int64_t k, double lambda, int, double alpha, int precision, int, int64_t n, const int64_t* index,
                           const int32_t* item, const double* val, const double* weight, double* U_out, pcr_ridge_stats*, double*) {
    const int rc = pcr_fold_in_conf_check("pcr_fold_in_conf_model", true, F, rows, k, lambda, alpha, precision, n, index, item, val, weight, U_out, nullptr);
    return rc != PCR_OK ? rc : absent();
}
NO_SOLVER(pcr_fold_in_conf, pcr_solver*, int, double, int64_t, const int64_t*, const int32_t*, const double*, const double*, double*, pcr_ridge_stats*,
          double*)
int pcr_fold_in_nnls_model(const double* F, int64_t rows, int64_t k, double lambda, int, int precision, int, int64_t n, const int64_t* index,
                           const int32_t* item, const double* val, double* U_out, pcr_nnls_stats*, double*) {
    const int rc = pcr_fold_in_nnls_check("pcr_fold_in_nnls_model", true, F, rows, k, lambda, precision, n, index, item, val, U_out, nullptr);
    return rc != PCR_OK ? rc : absent();
}
NO_SOLVER(pcr_fold_in_nnls, pcr_solver*, int, int64_t, const int64_t*, const int32_t*, const double*, double*, pcr_nnls_stats*, double*)
int pcr_fold_in_items_model(const pcr_params* p, const double* U, int64_t d1, const double* V, int64_t d2, const int64_t* tr_index,
                            const int32_t* tr_item, const double* tr_val, int64_t n, const int64_t* index, const int32_t* user, const double* val,
                            const double*, int steps, double* V_out, pcr_itemfold_stats*, double*) {
    const int rc = pcr_fold_in_items_check("pcr_fold_in_items_model", true, p, U, d1, V, d2, tr_index, tr_item, tr_val, n, index, user, val, steps, V_out,
                                           nullptr);
    return rc != PCR_OK ? rc : absent();
}
NO_SOLVER(pcr_fold_in_items, pcr_solver*, const pcr_dataset*, int64_t, const int64_t*, const int32_t*, const double*, const double*, int, double*,
          pcr_itemfold_stats*, double*)
int pcr_explain_model(const pcr_params* p, const double* V, int64_t d2, int64_t n, const int64_t* index, const int32_t* item, const double* val,
                      const double* U, const double* weights, int L, const int32_t* lists, int E, int32_t* expl_item, double* expl_contrib, double*,
                      double*, pcr_explain_stats*) {
    const int rc = pcr_explain_check("pcr_explain_model", true, p, V, d2, n, index, item, val, U, weights, L, lists, E, expl_item, expl_contrib, nullptr);
    return rc != PCR_OK ? rc : absent();
}
NO_SOLVER(pcr_explain, pcr_solver*, const pcr_dataset*, int64_t, const int32_t*, const double*, int, const int32_t*, int, int32_t*, double*, double*,
          double*, pcr_explain_stats*)
int pcr_explain_ridge_model(const double* F, int64_t rows, int64_t k, double lambda, int, int nonneg, int precision, int, int64_t n, const int64_t* index,
                            const int32_t* item, const double* val, const double* U, int L, const int32_t* lists, int E, int32_t* expl_item,
                            double* expl_contrib, double*, double*, pcr_explain_ridge_stats*) {
    const int rc = pcr_explain_ridge_check("pcr_explain_ridge_model", true, F, rows, k, lambda, nonneg, precision, n, index, item, val, U != nullptr, L,
                                           lists, E, expl_item, expl_contrib, nullptr);
    return rc != PCR_OK ? rc : absent();
}
NO_SOLVER(pcr_explain_ridge, pcr_solver*, const pcr_dataset*, int64_t, const int32_t*, int, int, int, const int32_t*, int, int32_t*, double*, double*,
          double*, pcr_explain_ridge_stats*)
NO_SOLVER(pcr_evaluate_rerank, pcr_solver*, int64_t, const int32_t*, int, const double*, int, int, const int*, double, int, pcr_topn_stats*,
          pcr_diversity_stats*, double*, double*, int64_t*)
}
