// pcr_host.h -- host-side data structures shared by the loader, the solver and the CLIs.
#pragma once
#include <cstdint>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "primalcr.h"

// std::vector whose resize(n) leaves the new elements UNINITIALISED: the loader's nnz-sized arrays are written exactly once, by the
// threads that parse / scatter into them (a zero-fill of 8.4 GB on one thread is seconds at the Yahoo!Music shape, and it
// would first-touch every page on the calling thread's NUMA node).
template <class T>
struct PcrNoInit : std::allocator<T> {
    template <class U> struct rebind { using other = PcrNoInit<U>; };
    PcrNoInit() = default;
    template <class U> PcrNoInit(const PcrNoInit<U>&) {}
    template <class U, class... A> void construct(U* p, A&&... a) {
        if constexpr (sizeof...(A) == 0) ::new ((void*)p) U; else ::new ((void*)p) U(std::forward<A>(a)...);
    }
};
template <class T> using pcr_vec = std::vector<T, PcrNoInit<T>>;

// user-major CSR in the reference's SparseMat layout (util.h:390-413); `item` is
// SparseMat::rows, the user id per rating (SparseMat::cols) is implied by `index`.
struct PcrCsr {
    int64_t d1 = 0, d2 = 0;
    std::vector<int64_t> index;   // d1 + 1
    pcr_vec<int32_t> item;        // nnz
    pcr_vec<double> val;          // nnz
    int64_t nnz() const { return index.empty() ? 0 : index.back(); }
};

struct pcr_dataset {
    PcrCsr train, test;
    int64_t tnnz_file = 0;        // test entries read from the file (T.nnz, pcrpp.cpp:865)
    // The test file's triplets in file order (the reference's testset_t T, util.h:360-371) when the test CSR does not hold them
    // as they are -- a file that is not user-sorted or names a user id >= d1 (convert()'s scan moves or drops such entries);
    // empty otherwise (the CSR, row by row, IS the file).  CCDR1's printed rmse walks T (util.cpp:206-215).
    std::vector<int32_t> traw_user, traw_item;
    std::vector<double> traw_val;
};

// dense rank of the rating bucket inside each user: lround(val) for PrimalCR++
// (pcrpp.cpp:38-49,182-189), the raw double for PrimalCR (pcr.cpp:23 compares doubles).
// level[z] in [0, T_u); run_ofs[u]..run_ofs[u+1] indexes run_start, which holds T_u + 1
// cumulative per-level counts for user u (run_start[run_ofs[u] + T_u] == len_u).
struct PcrLevels {
    std::vector<uint16_t> level;      // nnz
    std::vector<int64_t> run_ofs;     // d1 + 1
    std::vector<int32_t> run_start;   // sum_u (T_u + 1)
    std::vector<double> lev_val;      // same slots as run_start: the key of level l of user u at run_ofs[u] + l (slot T_u unused)
    int max_levels = 0;
    bool integer_valued = true;       // every rating of the range equals its own lround(): raw levels = rounded levels
};
int pcr_build_levels(const PcrCsr& X, int64_t u0, int64_t u1, int solver_type, PcrLevels& out, std::string& err);

// host set-up helpers: fn(thread, lo, hi) over contiguous pieces of [0, n); the thread count set-up work uses
void pcr_parallel_ranges(int64_t n, int nthreads, const std::function<void(int, int64_t, int64_t)>& fn);
void pcr_parallel_tasks(int ntasks, int nthreads, const std::function<void(int)>& fn);
int pcr_host_threads();

void pcr_set_error(const std::string& msg);

// launch knobs set through pcr_tune() (include/primalcr.h): consulted by the solver when it is created
bool pcr_tune_get(const char* key, std::string* out);
int pcr_tune_int(const char* key, int dflt);

// pcr_recommend_model's argument checks (the library and the sanitizer build's "no device" stub run the same ones): sizes, K,
// user ids inside the model, the exclusion CSR's shape (index[0] = 0, monotone, items inside [0, d2)).  *sorted = every row of
// `item` is non-decreasing (the kernel's exclusion cursor needs that; the caller sorts a copy otherwise).
int pcr_recommend_model_check(const double* U, int64_t d1, const double* V, int64_t d2, int64_t k, const int64_t* index,
                              const int32_t* item, int64_t n, const int32_t* users, int topk, int dtype, const int32_t* items,
                              const double* scores, bool* sorted, const char* who = "pcr_recommend_model");

// The item filter of pcr_recommend_filtered / pcr_recommend_filtered_model for n requests over d2 items (both entries and the
// sanitizer build's stub run this one): f != NULL with an allow set or candidate lists (neither: the message points to
// pcr_recommend); cand_ptr[0] = 0 and monotone over n + 1 entries, cand_item given with it, every id inside [0, d2), no id twice
// in a row (checked on a sorted copy of the row, by the host threads).  A message names `who` and the row's user (users[i],
// NULL: i).
int pcr_item_filter_check(const char* who, int64_t d2, int64_t n, const int32_t* users, const pcr_item_filter* f);
// pcr_recommend_filtered_model's argument checks: those of pcr_recommend_model, then pcr_item_filter_check
int pcr_recommend_filtered_model_check(const double* U, int64_t d1, const double* V, int64_t d2, int64_t k, const int64_t* index,
                                       const int32_t* item, int64_t n, const int32_t* users, int topk, int dtype, const pcr_item_filter* f,
                                       const int32_t* items, const double* scores, bool* sorted);

// the top-N evaluation's own arguments (both entries): 1 .. PCR_TOPN_MAX_CUTOFFS cutoffs, strictly ascending, inside
// [1, PCR_RECOMMEND_MAX_K]; threshold not NaN; stats != NULL.  Errors are prefixed with `who`.
int pcr_topn_check(const char* who, int ncut, const int* cutoffs, double threshold, const pcr_topn_stats* stats);
// pcr_evaluate_topn_model's argument checks (shared with the sanitizer build's stub): the factor / exclusion checks of
// pcr_recommend_model, pcr_topn_check and the test CSR's shape.  *sorted as pcr_recommend_model_check.
int pcr_evaluate_topn_model_check(const double* U, int64_t d1, const double* V, int64_t d2, int64_t k, const int64_t* index,
                                  const int32_t* item, const int64_t* tindex, const int32_t* titem, const double* tval, int ncut,
                                  const int* cutoffs, double threshold, int dtype, const pcr_topn_stats* stats, bool* sorted,
                                  const char* who = "pcr_evaluate_topn_model");

// Top-N evaluation's relevance tables (include/primalcr.h, "full-catalogue top-N evaluation") of rows [0, rows) of a test CSR
// (tptr[rows + 1] relative, items in any order): the counted users (|R_u| >= 1, ascending), their relevant rows (distinct items
// ascending, each with its graded gain pow(2, v_max) - 1), the discounts d(i) for i < the largest cutoff and per counted user
// and cutoff the ideal DCGs, binary then graded, each summed in position order.
struct PcrTopnRel {
    std::vector<int32_t> users;
    std::vector<int64_t> rptr;       // users.size() + 1
    std::vector<int32_t> ritem;
    std::vector<double> rgain;
    std::vector<double> disc;
    std::vector<double> idcg;        // [users][ncut][2]
};
void pcr_topn_relevance(int64_t rows, const int64_t* tptr, const int32_t* titem, const double* tval, double threshold, int ncut,
                        const int* cutoffs, PcrTopnRel& out);
// stats[c] from the reduced sums (k_topn_fin's layout: [ncut][8], then the counted users)
void pcr_topn_stats_from(const double* sums, int ncut, const int* cutoffs, pcr_topn_stats* stats);

// Beyond-accuracy metrics (include/primalcr.h, "beyond-accuracy top-N metrics").
// the cutoff list of an evaluation entry: 1 .. PCR_TOPN_MAX_CUTOFFS values, strictly ascending, inside [1, PCR_RECOMMEND_MAX_K]
int pcr_cutoffs_check(const char* who, int ncut, const int* cutoffs);
// pcr_evaluate_diversity_model's argument checks (shared with the sanitizer build's stub): the cutoffs, stats != NULL, then the
// factor / user / exclusion checks of pcr_recommend_model.  *sorted as pcr_recommend_model_check.
int pcr_evaluate_diversity_model_check(const double* U, int64_t d1, const double* V, int64_t d2, int64_t k, const int64_t* index,
                                       const int32_t* item, int64_t n, const int32_t* users, int ncut, const int* cutoffs, int dtype,
                                       const pcr_diversity_stats* stats, bool* sorted);
// info[j] = log2((d1 + 1) / (pop[j] + 1)) for the d2 popularity counts pop (exact integers in fp64)
void pcr_diversity_info(int64_t d1, const double* pop, int64_t d2, double* info);
// pcr_recommend_diverse's own arguments: 1 <= topk <= pool <= PCR_RECOMMEND_MAX_K, theta in [0, 1] (a NaN is refused)
int pcr_rerank_check(const char* who, int topk, int pool, double theta);
// pcr_recommend_diverse_model's argument checks (shared with the sanitizer build's stub): pcr_rerank_check, then the factor /
// user / exclusion / output checks of pcr_recommend_model.  *sorted as pcr_recommend_model_check.
int pcr_recommend_diverse_model_check(const double* U, int64_t d1, const double* V, int64_t d2, int64_t k, const int64_t* index,
                                      const int32_t* item, int64_t n, const int32_t* users, int topk, int pool, double theta, int dtype,
                                      const int32_t* items, const double* scores, bool* sorted);
// Group-capped lists (include/primalcr.h, "group-capped top-K lists").
// pcr_recommend_capped's own arguments (both entries): group != NULL, cap >= 1, 1 <= topk <= pool <= PCR_RECOMMEND_MAX_K
int pcr_cap_check(const char* who, int topk, int pool, const int32_t* group, int cap);
// its filter (NULL: none): candidate rows are PCR_ERR_UNSUPPORTED, a filter with nothing in it is PCR_ERR_ARG
int pcr_cap_filter_check(const char* who, const pcr_item_filter* f);
// pcr_recommend_capped_model's argument checks (shared with the sanitizer build's stub): pcr_cap_check, the factor / user /
// exclusion / output checks of pcr_recommend_model with K = pool, then pcr_cap_filter_check.  *sorted as pcr_recommend_model_check.
int pcr_recommend_capped_model_check(const double* U, int64_t d1, const double* V, int64_t d2, int64_t k, const int64_t* index,
                                     const int32_t* item, int64_t n, const int32_t* users, int topk, int pool, const int32_t* group, int cap,
                                     int dtype, const pcr_item_filter* f, const int32_t* items, const double* scores, bool* sorted);
// stats from the finished rows: status[n] and items[n][topk] (padding -1 only at a row's end)
void pcr_cap_stats_from(int64_t n, int topk, const uint8_t* status, const int32_t* items, pcr_cap_stats* stats);
// stats[c] from the reduced sums (k_topn_fin's layout: [ncut][8] = sum len, sum novelty, -, users with len >= 1, -, -, sum ild,
// users_ild; then the requested users) and the cumulative exposure rows expo[ncut][d2] (exact integers in fp64); exposure
// (may be NULL) receives them as int64.  pcr_exposure_stats' return code.
int pcr_diversity_stats_from(const double* sums, int ncut, const int* cutoffs, const double* expo, int64_t d2,
                             pcr_diversity_stats* stats, int64_t* exposure);

// Exact rank metrics (include/primalcr.h, "exact full-catalogue rank metrics").
// pcr_evaluate_ranks_model's argument checks (shared with the sanitizer build's stub): threshold not NaN, stats != NULL, the
// factor / exclusion checks of pcr_recommend_model and the test CSR's shape.  *sorted as pcr_recommend_model_check.
int pcr_evaluate_ranks_model_check(const double* U, int64_t d1, const double* V, int64_t d2, int64_t k, const int64_t* index,
                                   const int32_t* item, const int64_t* tindex, const int32_t* titem, const double* tval,
                                   double threshold, int dtype, const pcr_rank_stats* stats, bool* sorted,
                                   const char* who = "pcr_evaluate_ranks_model");
// stats from the reduced sums of k_rank_finish's rows (k_topn_fin's layout with one cutoff: |R_u|, rr, mean_rank, users, mpr,
// first_rank, auc, users_auc summed, then the counted users)
void pcr_rank_stats_from(const double* sums, pcr_rank_stats* stats);
// ranks[z] of rows [0, rows) of the test CSR from rrank (the ranks of rel.ritem, entry for entry): the rank of titem[z] where
// tval[z] >= threshold, 0 elsewhere
void pcr_rank_scatter(int64_t rows, const int64_t* tptr, const int32_t* titem, const double* tval, double threshold,
                      const PcrTopnRel& rel, const int64_t* rrank, int64_t* ranks);

// Filtered evaluation (include/primalcr.h, "filtered evaluation").
// The filter of a filtered evaluation entry over `rows` users: f != NULL with an allow set or candidate rows (neither: the
// message points to `unfiltered`), then pcr_item_filter_check as it is, with rows 0 .. rows - 1.
int pcr_eval_filter_check(const char* who, const char* unfiltered, int64_t d2, int64_t rows, const pcr_item_filter* f);
// Rows [0, rows) of a test CSR restricted to F_u: the ratings whose item passes f's allow set and sits in the user's candidate
// row (a sorted copy of the row makes the membership test), in their order; pos[z'] is where rating z' stood in the test CSR.
// pcr_topn_relevance over this CSR gives R_u^f.
struct PcrFilteredTest {
    std::vector<int64_t> ptr;        // rows + 1
    std::vector<int32_t> item;
    std::vector<double> val;
    std::vector<int64_t> pos;
};
void pcr_filter_test_rows(int64_t rows, const int64_t* tptr, const int32_t* titem, const double* tval, const pcr_item_filter& f,
                          PcrFilteredTest& out);

// Metrics of device-resident lists (include/primalcr.h, "evaluating given and re-ranked lists").
// lists[n][L] as pcr_evaluate_lists_model takes them: every entry -1 or inside [0, d2), no entry after a -1, no id twice in a
// list; by the host threads.  Errors are prefixed with `who`.
int pcr_lists_check(const char* who, int64_t d2, int64_t n, int L, const int32_t* lists);
// pcr_evaluate_lists_model's argument checks (shared with the sanitizer build's stub): L, the cutoffs (the last one <= L), the
// threshold, the outputs (without a test CSR topn and per_user_topn must be NULL; with one topn is required), the factor / user
// / popularity-CSR checks of pcr_recommend_model, the test CSR's shape and pcr_lists_check.
int pcr_evaluate_lists_model_check(const double* V, int64_t d2, int64_t k, int64_t d1, const int64_t* index, const int32_t* item,
                                   const int64_t* tindex, const int32_t* titem, const double* tval, int64_t n, const int32_t* users, int L,
                                   const int32_t* lists, int ncut, const int* cutoffs, double threshold, int dtype,
                                   const pcr_topn_stats* topn, const double* per_user_topn, const pcr_diversity_stats* div);
// the theta sweep's own arguments: the cutoffs, topk = cutoffs[ncut - 1] <= pool <= PCR_RECOMMEND_MAX_K, 1 <= nth <=
// PCR_RERANK_MAX_THETAS, every theta in [0, 1] (a NaN is refused), threshold not NaN, div != NULL
int pcr_tradeoff_check(const char* who, int nth, const double* thetas, int pool, int ncut, const int* cutoffs, double threshold,
                       const pcr_diversity_stats* div);
// pcr_evaluate_rerank_model's argument checks (shared with the sanitizer build's stub): pcr_tradeoff_check, the outputs as
// pcr_evaluate_lists_model_check, the factor / user / exclusion checks of pcr_recommend_model and the test CSR's shape.
// *sorted as pcr_recommend_model_check.
int pcr_evaluate_rerank_model_check(const double* U, int64_t d1, const double* V, int64_t d2, int64_t k, const int64_t* index,
                                    const int32_t* item, const int64_t* tindex, const int32_t* titem, const double* tval, int64_t n,
                                    const int32_t* users, int nth, const double* thetas, int pool, int ncut, const int* cutoffs,
                                    double threshold, int dtype, const pcr_topn_stats* topn, const double* per_user_topn,
                                    const pcr_diversity_stats* div, bool* sorted);
// The relevance tables of n requested lists: row i is that of user users[i] (NULL: user i) among rows [0, rows) of the test CSR,
// possibly empty -- pcr_topn_relevance's tables are compact over the counted users, these have a row for every request (a user
// given twice has its row twice).  disc has L entries (the list length, which may exceed the last cutoff); idcg is
// [n][ncut][2], zeros for an empty row.  users, the compact ids of pcr_topn_relevance, is left empty.  Returns the number of
// requests with a non-empty row (the counted ones).
int64_t pcr_list_relevance(int64_t rows, const int64_t* tptr, const int32_t* titem, const double* tval, double threshold, int ncut,
                           const int* cutoffs, int64_t n, const int32_t* users, int L, PcrTopnRel& out);

// Fold-in (include/primalcr.h, "fold-in").  What the host prepares for k_foldin: the new users' ratings with item-ascending rows
// (a sorted copy when the caller's are not), their levels (pcr_build_levels) and the users by descending length -- order[0, n_big)
// take the global-scratch form, the next n_lds the LDS form, the rest one wave each.
struct PcrFoldinPlan {
    PcrCsr X;
    PcrLevels lv;
    std::vector<int32_t> order;
    int64_t n_big = 0, n_lds = 0;
};
// The argument checks of both entries (the library and the sanitizer build's "no device" stubs run the same ones): solver type
// 1 or 2 (0: PCR_ERR_UNSUPPORTED), the CSR's shape, item ids inside [0, d2), finite ratings, steps >= 1, the output, whatever
// pcr_build_levels refuses; errors are prefixed with `who`.  plan (may be NULL) receives the plan.
int pcr_fold_in_check(const char* who, int solver_type, int64_t d2, int64_t n, const int64_t* index, const int32_t* item, const double* val,
                      int steps, const double* U_out, PcrFoldinPlan* plan);
// ... without the fold-in entries' own arguments (steps, the output): the rows, their levels and the plan alone (pcr_explain_check)
int pcr_fold_in_rows_check(const char* who, int solver_type, int64_t d2, int64_t n, const int64_t* index, const int32_t* item, const double* val,
                           PcrFoldinPlan* plan);
// pcr_fold_in_model's: the parameters it reads of p (k, precision, lambda, stepsize, cg_max_iter, cg_tol), V, then pcr_fold_in_check
int pcr_fold_in_model_check(const pcr_params* p, const double* V, int64_t d2, int64_t n, const int64_t* index, const int32_t* item,
                            const double* val, int steps, const double* U_out, PcrFoldinPlan* plan);
// stats from the per-user table [n][PCR_FOLDIN_FIELDS]: the counts, and obj added in user order
void pcr_foldin_stats_from(const double* per_user, int64_t n, pcr_foldin_stats* stats);

// Explanations (include/primalcr.h, "explaining recommendations").  The argument checks of pcr_explain_model / pcr_explain in the
// order the header lists them (the library and the sanitizer build's "no device" stub run the same ones) and the plan, which is
// fold-in's: the rows item-ascending, their levels, the users by descending length in the three workgroup forms.  need_factors:
// V and U are the caller's (the standalone entry; k and precision of p are checked with them); p's lambda and solver type are
// read by both.  Errors are prefixed with `who`.  plan may be NULL.
int pcr_explain_check(const char* who, bool need_factors, const pcr_params* p, const double* V, int64_t d2, int64_t n, const int64_t* index,
                      const int32_t* item, const double* val, const double* U, const double* weights, int L, const int32_t* lists, int E,
                      const int32_t* expl_item, const double* expl_contrib, PcrFoldinPlan* plan);
// stats from the finished tables per_pair [n][L][PCR_EXPLAIN_PAIR_FIELDS] and expl_item [n][L][E]; lists [n][L] tells the padding
void pcr_explain_stats_from(const double* per_pair, const int32_t* expl_item, const int32_t* lists, int64_t n, int L, int E, pcr_explain_stats* stats);

// Item fold-in (include/primalcr.h, "item fold-in").  What the host prepares for k_rater_scores / k_itemfold: the new items as
// SLOTS by descending rater count (equal counts by ascending id) -- slots [0, n_big) take the global-scratch form, the next n_lds
// the LDS form, the rest one wave each -- with their (item, rater) pairs in ascending user order; the call's unique raters
// (ascending user id), a copy R of their training rows with its levels, and per pair the doubled rank of the new rating among
// the rater's levels: 2 * rank when the row holds the level, the odd value between its neighbours when it does not.
struct PcrItemfoldPlan {
    int64_t n = 0, n_big = 0, n_lds = 0;
    std::vector<int32_t> order;       // [n] slot -> item
    std::vector<int64_t> sptr;        // [n + 1] the slots' pairs
    std::vector<int32_t> puser, prater, pq;   // per pair: the user id, its position in `raters`, the doubled rank
    std::vector<int32_t> anypair;     // [n] per slot: some rater's row holds a level different from the new rating's
    std::vector<int32_t> raters;      // unique rater ids, ascending
    PcrCsr R;                         // their training rows: row i is user raters[i]
    PcrLevels lv;
};
// pcr_fold_in_items_model's / pcr_fold_in_items' argument checks, in the order include/primalcr.h lists the errors, and the plan.
// need_factors: U and V are the caller's (the standalone entry).  Errors are prefixed with `who`.  plan may be NULL.
int pcr_fold_in_items_check(const char* who, bool need_factors, const pcr_params* p, const double* U, int64_t d1, const double* V, int64_t d2,
                            const int64_t* tr_index, const int32_t* tr_item, const double* tr_val, int64_t n, const int64_t* index,
                            const int32_t* user, const double* val, int steps, const double* V_out, PcrItemfoldPlan* plan);
// stats from the per-item table [n][PCR_ITEMFOLD_FIELDS]: the counts, and obj added in item order (unique_raters is the caller's)
void pcr_itemfold_stats_from(const double* per_item, int64_t n, pcr_itemfold_stats* stats);

// What both fold-in plans share, factored out of pcr_fold_in_check.  pcr_csr_rows_scan: n CSR rows over d2 columns, by the host
// threads -- bit 0 = an id outside [0, d2), bit 1 = a rating that is not finite, bit 2 = a row that is not item-ascending.
// pcr_csr_sorted_copy: the copy X of the rows; sort = rows in ascending item order (equal items keep their order).
int pcr_csr_rows_scan(int64_t d2, int64_t n, const int64_t* index, const int32_t* item, const double* val);
void pcr_csr_sorted_copy(int64_t d2, int64_t n, const int64_t* index, const int32_t* item, const double* val, bool sort, PcrCsr& X);

// Ridge fold-in (include/primalcr.h, "ridge fold-in").  The form of a user of len ratings at rank k (PCR_RIDGE_DUAL / PRIMAL / CG).
int pcr_ridge_form(int64_t len, int64_t k);
// What the host prepares for k_ridge_direct / k_ridge_cg: the ratings with item-ascending rows (a sorted copy when the caller's are
// not) and the users grouped into launch ranges of `order` -- one per (form, workgroup size, 16 x 16 tiles per side of the Gram
// matrix), users in descending length inside a range.  force_cg: pcr_tune("ridge_form", "cg") when the plan was made.
struct PcrRidgePlan {
    struct Range { int form = 0, block = 0, tiles = 0; int64_t first = 0, count = 0; };
    PcrCsr X;
    std::vector<int32_t> order;
    std::vector<Range> ranges;
    bool force_cg = false;
};
// The argument checks of both entries and the plan (the library and the sanitizer build's "no device" stub run the same ones):
// F (need_F: the model entry; the solver entry reads its device V), k, rows, lambda, precision, the CSR's shape, ids inside
// [0, rows), finite ratings, the output; errors are PCR_ERR_ARG prefixed with `who`.  plan (may be NULL) receives the plan.
int pcr_fold_in_ridge_check(const char* who, bool need_F, const double* F, int64_t rows, int64_t k, double lambda, int precision, int64_t n,
                            const int64_t* index, const int32_t* item, const double* val, const double* U_out, PcrRidgePlan* plan);
// stats from the per-user table [n][PCR_RIDGE_FIELDS]: the counts, and loss / obj added in user order
void pcr_ridge_stats_from(const double* per_user, int64_t n, pcr_ridge_stats* stats);

// Confidence-weighted / implicit fold-in (include/primalcr.h, "confidence-weighted and implicit fold-in").  The form of a user of
// len ratings at rank k, a function of (len, k, alpha > 0) alone: the ridge rule for implicit == 0; else PRIMAL at every len while
// roundup(k, 16) <= PCR_RIDGE_DIRECT_MAX (the alpha G term makes the system k x k whatever the length), CG beyond.
// pcr_conf_block: the workgroup width of that user -- 256 threads for the CG form, for more than PCR_RIDGE_WAVE_MAX ratings and
// for an implicit primal system of more than 4 x 4 tiles (one wave carries at most 4 x 4), else 64.
int pcr_conf_form(int64_t len, int64_t k, int implicit);
int pcr_conf_block(int64_t len, int64_t k, int implicit);
// The ridge plan (ranges by pcr_conf_form / pcr_conf_block) and what the conf kernels read besides: wt = the weights in X's order
// (carried through the sorted copy's permutation; ones when the caller gave none), W[u] = sum of the user's weights in that order
// + alpha (rows - len).  plain: no weights and alpha == 0 -- the plan is pcr_fold_in_ridge_check's and the ridge kernels run it.
struct PcrConfPlan : PcrRidgePlan {
    std::vector<double> wt, W;
    double alpha = 0.0;
    bool plain = false;
};
// pcr_fold_in_ridge_check's checks, then: every weight finite and > 0 (weight may be NULL), alpha finite and >= 0; errors are
// PCR_ERR_ARG prefixed with `who`.  plan (may be NULL) receives the plan.
int pcr_fold_in_conf_check(const char* who, bool need_F, const double* F, int64_t rows, int64_t k, double lambda, double alpha, int precision, int64_t n,
                           const int64_t* index, const int32_t* item, const double* val, const double* weight, const double* U_out, PcrConfPlan* plan);

// Non-negative fold-in (include/primalcr.h, "non-negative fold-in").  The form at rank k (PCR_NNLS_DIRECT / CG), a function of k alone.
int pcr_nnls_form(int64_t k);
// The ridge entries' argument checks under the nnls entry's name (one shared routine), and the plan for k_nnls_direct / k_nnls_cg
// in a PcrRidgePlan: form and workgroup size follow from the rank, so there is one range, its users in descending length.
// force_cg: pcr_tune("nnls_form", "cg") when the plan was made.
int pcr_fold_in_nnls_check(const char* who, bool need_F, const double* F, int64_t rows, int64_t k, double lambda, int precision, int64_t n,
                           const int64_t* index, const int32_t* item, const double* val, const double* U_out, PcrRidgePlan* plan);
// stats from the per-user table [n][PCR_NNLS_FIELDS]: the counts, and loss / obj added in user order
void pcr_nnls_stats_from(const double* per_user, int64_t n, pcr_nnls_stats* stats);

// Explanations of squared-loss rows (include/primalcr.h, "explaining squared-loss recommendations").  The argument checks of
// pcr_explain_ridge_model / pcr_explain_ridge in the order the header lists them (the library and the sanitizer build's "no
// device" stub run the same ones): the ridge entries' checks of F (need_F: the model entry), k, rows, lambda, precision and the
// rows; lambda > 0; has_U: the entry has rows of U to explain (the solver entry always; false with nonneg is refused); the lists
// and outputs as pcr_explain_check; last the rank against PCR_RIDGE_DIRECT_MAX (PCR_ERR_UNSUPPORTED).  Errors are prefixed with
// `who`.  The plan (may be NULL) is a PcrRidgePlan with the item-ascending rows and ONE range: the users by descending length.
int pcr_explain_ridge_check(const char* who, bool need_F, const double* F, int64_t rows, int64_t k, double lambda, int nonneg, int precision,
                            int64_t n, const int64_t* index, const int32_t* item, const double* val, bool has_U, int L, const int32_t* lists, int E,
                            const int32_t* expl_item, const double* expl_contrib, PcrRidgePlan* plan);
// stats from the finished tables per_pair [n][L][PCR_EXPLAIN_PAIR_FIELDS], per_user [n][PCR_EXPLAIN_RIDGE_USER_FIELDS] and
// expl_item [n][L][E]; lists [n][L] tells the padding
void pcr_explain_ridge_stats_from(const double* per_pair, const double* per_user, const int32_t* expl_item, const int32_t* lists, int64_t n, int L,
                                  int E, pcr_explain_ridge_stats* stats);
