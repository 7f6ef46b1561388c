"""ctypes mirror of include/primalcr.h (the reference's solver interface, pmf.h:9-56)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

PCR_SOLVER_CCDR1, PCR_SOLVER_PCR, PCR_SOLVER_PCRPP = 0, 1, 2
PCR_F32, PCR_F64 = 0, 1
PCR_WEIGHT_UNIFORM, PCR_WEIGHT_PAIRS, PCR_WEIGHT_RATINGS = 0, 1, 2               # user_weights' schemes
PCR_RECOMMEND_MAX_K = 1024
PCR_REC_EXCLUDE_TRAIN = 1
PCR_TOPN_MAX_CUTOFFS = 8
PCR_RERANK_MAX_THETAS = 8
PCR_CAP_EXACT, PCR_CAP_POOL_EXHAUSTED = 0, 1
# evaluate_ranks' stage lengths (include/primalcr.h, pcr_topk.h): relevant rows up to these lengths are counted in LDS by the
# full sweep / by the candidate-row kernel, longer ones in global memory; results do not depend on them (tests straddle them)
PCR_RANK_STAGE, PCR_CAND_RANK_STAGE = 32, 64
TOPN_FIELDS = ("hits", "precision", "recall", "ap", "ndcg", "ndcg_graded")   # per_user columns
RANK_FIELDS = ("first_rank", "rr", "mean_rank", "auc", "mpr")                   # evaluate_ranks' per_user columns (PCR_RANK_FIELDS)
DIVERSITY_FIELDS = ("len", "novelty", "ild")                                     # evaluate_diversity's per_user columns (PCR_DIVERSITY_FIELDS)
PCR_FOLDIN_FIELDS = ("steps", "cg", "ls", "obj", "gnorm2", "status")             # fold_in's per_user columns
PCR_FOLDIN_CONVERGED, PCR_FOLDIN_STEP_CAP, PCR_FOLDIN_STALLED = 0, 1, 2          # ... and its status values
# fold_in's workgroup forms by user length (include/primalcr.h): one wave up to WAVE_MAX ratings, per-rating arrays in LDS up to
# LDS_MAX, global scratch beyond
PCR_FOLDIN_WAVE_MAX, PCR_FOLDIN_LDS_MAX = 64, 2048
PCR_ITEMFOLD_FIELDS = ("raters", "steps", "cg", "ls", "obj0", "obj", "gnorm2", "status")   # fold_in_items' per_item columns (status: PCR_FOLDIN_*)
# fold_in_items' workgroup forms by rater count (include/primalcr.h): one wave up to WAVE_MAX raters, per-rater arrays in LDS up to
# LDS_MAX, global scratch beyond; its rater table takes a rater on one wave up to SCORES_WAVE_MAX training ratings
PCR_ITEMFOLD_WAVE_MAX, PCR_ITEMFOLD_LDS_MAX, PCR_ITEMFOLD_SCORES_WAVE_MAX = 64, 2048, 64
PCR_RIDGE_FIELDS = ("n", "form", "iters", "loss", "obj", "status")               # fold_in_ridge's per_user columns
PCR_RIDGE_DUAL, PCR_RIDGE_PRIMAL, PCR_RIDGE_CG = 0, 1, 2                         # ... its forms
PCR_RIDGE_OK, PCR_RIDGE_SINGULAR, PCR_RIDGE_CG_CAP = 0, 1, 2                     # ... and its status values
# fold_in_ridge's rule (include/primalcr.h): one wave up to WAVE_MAX ratings; the direct (Cholesky) forms up to a system of side DIRECT_MAX
PCR_RIDGE_WAVE_MAX, PCR_RIDGE_DIRECT_MAX = 64, 112
PCR_NNLS_FIELDS = ("n", "form", "pivots", "zeros", "loss", "obj", "status")       # fold_in_nnls's per_user columns
PCR_NNLS_DIRECT, PCR_NNLS_CG = 0, 1                                               # ... its forms
PCR_NNLS_OK, PCR_NNLS_SINGULAR, PCR_NNLS_CAP = 0, 1, 2                            # ... its status values
PCR_NNLS_PIVOT_CAP = 64                                                           # ... and the pivots a user may take
# explain(): the list length and the contributors per listed item it takes at most, its per_pair / per_user columns, and the
# listed items per tile / ratings per chunk of its kernel (include/primalcr.h, pcr_explain.h)
PCR_EXPLAIN_MAX_L, PCR_EXPLAIN_MAX_E = 128, 16
PCR_EXPLAIN_PAIR_FIELDS = ("score", "support", "opposition", "residual")
PCR_EXPLAIN_USER_FIELDS = ("ratings", "loss", "gnorm2")
EXPLAIN_TILE, EXPLAIN_CHUNK = 16, 256
# explain_ridge(): its per_user columns (status: PCR_RIDGE_OK / PCR_RIDGE_SINGULAR) and the ratings its Gram build stages at a time
PCR_EXPLAIN_RIDGE_USER_FIELDS = ("ratings", "free", "loss", "dist2", "status")
EXPLAIN_RIDGE_STAGE = 16

_HERE = os.path.dirname(os.path.abspath(__file__))


_LIB_OVERRIDE = None


def use_library(path):
    """Developer hook for A/B runs of two builds (tools/): load `path` instead of lib/libprimalcr.so.  Call before anything
    else of the package; the product path reads no environment variable (include/primalcr.h)."""
    global _LIB_OVERRIDE, _lib
    _LIB_OVERRIDE, _lib = path, None


def lib_path() -> str:
    return _LIB_OVERRIDE or os.path.join(_HERE, "lib", "libprimalcr.so")


class PcrError(RuntimeError):
    pass


class Parameter(C.Structure):
    """class parameter, pmf.h:9-49 (fields the PrimalCR/PrimalCR++ path reads) + device extensions."""
    _fields_ = [("solver_type", C.c_int), ("k", C.c_int), ("threads", C.c_int), ("maxiter", C.c_int),
                ("lambda_", C.c_double), ("do_predict", C.c_int), ("verbose", C.c_int), ("stepsize", C.c_double),
                ("ndcg_k", C.c_int), ("precision", C.c_int), ("device", C.c_int), ("cg_max_iter", C.c_int),
                ("cg_tol", C.c_double)]

    def __init__(self, **kw):
        super().__init__()
        lib().pcr_params_default(C.byref(self))
        for k, v in kw.items():
            if k == "lambda":
                k = "lambda_"
            if not hasattr(self, k):
                raise AttributeError(k)
            setattr(self, k, v)


class CcdParameter(C.Structure):
    """pcr_ccd_params: CCDR1's own settings (pmf.h:36,39,47: maxinneriter -T, eps -e, do_nmf -N)."""
    _fields_ = [("maxinneriter", C.c_int), ("eps", C.c_double), ("do_nmf", C.c_int)]

    def __init__(self, **kw):
        super().__init__()
        lib().pcr_ccd_params_default(C.byref(self))
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError(k)
            setattr(self, k, v)


class IterStats(C.Structure):
    _fields_ = [("obj", C.c_double), ("train_err", C.c_double), ("train_ndcg", C.c_double), ("test_err", C.c_double),
                ("test_ndcg", C.c_double), ("seconds", C.c_double), ("cg_v", C.c_int64), ("ls_v", C.c_int64),
                ("cg_u", C.c_int64), ("ls_u", C.c_int64)]


class TopnStats(C.Structure):
    _fields_ = [("cutoff", C.c_int), ("users", C.c_int64), ("users_graded", C.c_int64), ("hits", C.c_int64), ("precision", C.c_double),
                ("recall", C.c_double), ("hit_rate", C.c_double), ("map", C.c_double), ("ndcg", C.c_double), ("ndcg_graded", C.c_double)]


class DiversityStats(C.Structure):
    """pcr_diversity_stats."""
    _fields_ = [("cutoff", C.c_int), ("users", C.c_int64), ("users_ild", C.c_int64), ("recs", C.c_int64), ("items_covered", C.c_int64),
                ("coverage", C.c_double), ("gini", C.c_double), ("novelty", C.c_double), ("ild", C.c_double)]


class RankStats(C.Structure):
    """pcr_rank_stats."""
    _fields_ = [("users", C.c_int64), ("users_auc", C.c_int64), ("relevant", C.c_int64), ("mrr", C.c_double), ("mean_rank", C.c_double),
                ("auc", C.c_double), ("mpr", C.c_double)]


class ItemFilter(C.Structure):
    """pcr_item_filter."""
    _fields_ = [("allow", C.c_void_p), ("cand_ptr", C.c_void_p), ("cand_item", C.c_void_p)]


class CapStats(C.Structure):
    """pcr_cap_stats."""
    _fields_ = [("users", C.c_int64), ("exact", C.c_int64), ("exhausted", C.c_int64), ("short_rows", C.c_int64), ("kept", C.c_int64)]


class FoldinStats(C.Structure):
    """pcr_foldin_stats."""
    _fields_ = [("users", C.c_int64), ("converged", C.c_int64), ("step_cap", C.c_int64), ("stalled", C.c_int64), ("steps", C.c_int64),
                ("cg", C.c_int64), ("ls", C.c_int64), ("obj", C.c_double)]


class ItemfoldStats(C.Structure):
    """pcr_itemfold_stats."""
    _fields_ = [("items", C.c_int64), ("converged", C.c_int64), ("step_cap", C.c_int64), ("stalled", C.c_int64), ("steps", C.c_int64),
                ("cg", C.c_int64), ("ls", C.c_int64), ("raters", C.c_int64), ("unique_raters", C.c_int64), ("obj", C.c_double)]


class RidgeStats(C.Structure):
    """pcr_ridge_stats."""
    _fields_ = [("users", C.c_int64), ("dual", C.c_int64), ("primal", C.c_int64), ("cg", C.c_int64), ("singular", C.c_int64),
                ("cg_cap", C.c_int64), ("iters", C.c_int64), ("loss", C.c_double), ("obj", C.c_double)]


class NnlsStats(C.Structure):
    """pcr_nnls_stats."""
    _fields_ = [("users", C.c_int64), ("direct", C.c_int64), ("cg", C.c_int64), ("singular", C.c_int64), ("cap", C.c_int64),
                ("pivots", C.c_int64), ("zeros", C.c_int64), ("loss", C.c_double), ("obj", C.c_double)]


class ExplainStats(C.Structure):
    """pcr_explain_stats."""
    _fields_ = [("users", C.c_int64), ("pairs", C.c_int64), ("contributors", C.c_int64), ("residual_abs_max", C.c_double)]


class ExplainRidgeStats(C.Structure):
    """pcr_explain_ridge_stats."""
    _fields_ = [("users", C.c_int64), ("pairs", C.c_int64), ("contributors", C.c_int64), ("singular", C.c_int64),
                ("residual_abs_max", C.c_double)]


_LOG_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p)
_lib = None
_dp = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
_ip = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
_lp = np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")


def lib():
    """Load libprimalcr.so; fail loudly when it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise PcrError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(make -C primalcr_amd/csrc). There is no CPU fallback.")
    L = C.CDLL(path)
    vp, ci, cd, i64 = C.c_void_p, C.c_int, C.c_double, C.c_int64
    L.pcr_last_error.restype = C.c_char_p
    L.pcr_version.restype = C.c_char_p
    L.pcr_params_default.argtypes = [C.POINTER(Parameter)]
    L.pcr_initial.argtypes = [_dp, i64, i64]
    L.pcr_initial_rows.argtypes = [_dp, i64, i64, i64, i64]
    L.pcr_initial_col.argtypes = [_dp, i64, i64]
    L.pcr_ccd_params_default.argtypes = [C.POINTER(CcdParameter)]
    L.pcr_ccd_params_default.restype = None
    L.pcr_solver_set_ccd_params.argtypes = [vp, C.POINTER(CcdParameter)]
    L.pcr_dataset_load.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.pcr_dataset_load_mt.argtypes = [C.c_char_p, ci, C.POINTER(vp)]
    L.pcr_dataset_load_cached.argtypes = [C.c_char_p, ci, C.c_char_p, C.POINTER(vp)]
    L.pcr_dataset_load_cache.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.pcr_dataset_save_cache.argtypes = [vp, C.c_char_p]
    L.pcr_dataset_from_triplets.argtypes = [i64, i64, i64, vp, vp, vp, i64, vp, vp, vp, C.POINTER(vp)]
    L.pcr_dataset_from_csr.argtypes = [i64, i64, vp, vp, vp, vp, vp, vp, C.POINTER(vp)]
    L.pcr_dataset_free.argtypes = [vp]
    L.pcr_tune.argtypes = [C.c_char_p, C.c_char_p]
    L.pcr_dataset_dims.argtypes = [vp] + [C.POINTER(i64)] * 4
    L.pcr_dataset_csr.argtypes = [vp, ci, vp, vp, vp]
    L.pcr_dataset_count_pairs.argtypes = [vp, ci]
    L.pcr_dataset_count_pairs.restype = i64
    if _LIB_OVERRIDE is None or hasattr(L, "pcr_solver_set_user_weights"):
        L.pcr_dataset_user_pairs.argtypes = [vp, ci, vp]
        L.pcr_user_weights.argtypes = [vp, ci, ci, vp]
        L.pcr_solver_set_user_weights.argtypes = [vp, vp]
        L.pcr_solver_set_user_weights_local.argtypes = [vp, vp]
    if _LIB_OVERRIDE is None or hasattr(L, "pcr_solver_set_rating_weights"):
        L.pcr_dataset_match_weights.argtypes = [vp, i64, vp, vp, vp, vp]
        L.pcr_rating_weights_popularity.argtypes = [vp, cd, vp]
        L.pcr_solver_set_rating_weights.argtypes = [vp, vp]
    if _LIB_OVERRIDE is None or hasattr(L, "pcr_solver_set_implicit"):
        L.pcr_solver_set_implicit.argtypes = [vp, cd]
    L.pcr_model_save.argtypes = [C.c_char_p, _dp, i64, _dp, i64, i64]
    L.pcr_model_load.argtypes = [C.c_char_p, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), vp, vp]
    L.pcr_partition_users.argtypes = [_lp, i64, ci, _lp]
    L.pcr_solver_create.argtypes = [vp, C.POINTER(Parameter), ci, ci, C.POINTER(vp)]
    L.pcr_solver_create_shard.argtypes = [vp, C.POINTER(Parameter), ci, ci, i64, i64, C.POINTER(vp)]
    L.pcr_solver_destroy.argtypes = [vp]
    L.pcr_comm_unique_id.argtypes = [vp]
    L.pcr_solver_comm_init.argtypes = [vp, vp]
    L.pcr_solver_comm_init_p2p.argtypes = [vp, C.c_char_p]
    L.pcr_solver_comm_nranks.argtypes = [vp]
    L.pcr_solver_counter.argtypes = [vp, C.c_char_p, C.POINTER(cd)]
    L.pcr_solver_setup_phase.argtypes = [vp, ci, C.POINTER(C.c_char_p), C.POINTER(cd)]
    L.pcr_solver_ustep_classes.argtypes = [vp, C.c_char_p, i64]
    L.pcr_solver_set_local_only.argtypes = [vp, ci]
    L.pcr_solver_shard.argtypes = [vp] + [C.POINTER(i64)] * 3
    L.pcr_solver_set_factors.argtypes = [vp, vp, vp]
    L.pcr_solver_get_factors.argtypes = [vp, vp, vp]
    L.pcr_solver_set_factors_local.argtypes = [vp, vp, vp]
    L.pcr_solver_get_factors_local.argtypes = [vp, vp, vp]
    L.pcr_comp_m.argtypes = [vp, vp]
    L.pcr_objective.argtypes = [vp, C.POINTER(cd)]
    L.pcr_obtain_g.argtypes = [vp, _dp]
    L.pcr_compute_Ha.argtypes = [vp, _dp, _dp]
    L.pcr_solve_delta.argtypes = [vp, _dp, _dp, C.POINTER(ci)]
    L.pcr_update_V.argtypes = [vp, C.POINTER(cd), C.POINTER(ci)]
    L.pcr_update_U.argtypes = [vp, C.POINTER(cd), C.POINTER(i64)]
    L.pcr_evaluate.argtypes = [vp, ci, ci, C.POINTER(cd), C.POINTER(cd)]
    L.pcr_train.argtypes = [vp, vp, vp, C.POINTER(IterStats)]
    L.pcr_iterate.argtypes = [vp, ci, C.POINTER(IterStats)]
    L.pcr_predict.argtypes = [_dp, i64, _dp, i64, i64, i64, _ip, _ip, _dp, ci]
    L.pcr_recommend_model.argtypes = [vp, i64, vp, i64, i64, vp, vp, i64, vp, ci, ci, vp, vp, ci]
    L.pcr_recommend.argtypes = [vp, i64, vp, ci, ci, vp, vp]
    if _LIB_OVERRIDE is None or hasattr(L, "pcr_recommend_filtered"):   # (use_library may load an older build for an A/B run: tools/exp_filter.py)
        L.pcr_recommend_filtered_model.argtypes = [vp, i64, vp, i64, i64, vp, vp, i64, vp, ci, ci, C.POINTER(ItemFilter), vp, vp, ci]
        L.pcr_recommend_filtered.argtypes = [vp, i64, vp, ci, ci, C.POINTER(ItemFilter), vp, vp]
    L.pcr_recommend_diverse_model.argtypes = [vp, i64, vp, i64, i64, vp, vp, i64, vp, ci, ci, cd, ci, vp, vp, ci]
    L.pcr_recommend_diverse.argtypes = [vp, i64, vp, ci, ci, cd, ci, vp, vp]
    if hasattr(L, "pcr_recommend_capped"):                      # (absent from an older build loaded through use_library)
        L.pcr_recommend_capped_model.argtypes = [vp, i64, vp, i64, i64, vp, vp, i64, vp, ci, ci, vp, ci, ci, C.POINTER(ItemFilter), vp, vp, vp,
                                                 C.POINTER(CapStats), ci]
        L.pcr_recommend_capped.argtypes = [vp, i64, vp, ci, ci, vp, ci, ci, C.POINTER(ItemFilter), vp, vp, vp, C.POINTER(CapStats)]
    L.pcr_evaluate_topn_model.argtypes = [vp, i64, vp, i64, i64, vp, vp, vp, vp, vp, ci, vp, cd, ci, vp, vp, ci]
    L.pcr_evaluate_topn.argtypes = [vp, ci, vp, cd, ci, vp, vp]
    L.pcr_evaluate_ranks_model.argtypes = [vp, i64, vp, i64, i64, vp, vp, vp, vp, vp, cd, ci, vp, vp, vp, ci]
    L.pcr_evaluate_ranks.argtypes = [vp, cd, ci, vp, vp, vp]
    if hasattr(L, "pcr_evaluate_topn_filtered_model"):           # (absent from an older build loaded through use_library)
        L.pcr_evaluate_topn_filtered_model.argtypes = [vp, i64, vp, i64, i64, vp, vp, vp, vp, vp, ci, vp, cd, ci, C.POINTER(ItemFilter), vp, vp, ci]
        L.pcr_evaluate_topn_filtered.argtypes = [vp, ci, vp, cd, ci, C.POINTER(ItemFilter), vp, vp]
        L.pcr_evaluate_ranks_filtered_model.argtypes = [vp, i64, vp, i64, i64, vp, vp, vp, vp, vp, cd, ci, C.POINTER(ItemFilter), vp, vp, vp, ci]
        L.pcr_evaluate_ranks_filtered.argtypes = [vp, cd, ci, C.POINTER(ItemFilter), vp, vp, vp]
        L.pcr_sample_negatives.argtypes = [i64, i64, vp, vp, vp, vp, i64, i64, C.c_uint64, ci, vp, vp]
    L.pcr_evaluate_diversity_model.argtypes = [vp, i64, vp, i64, i64, vp, vp, i64, vp, ci, vp, ci, vp, vp, vp, ci]
    L.pcr_evaluate_diversity.argtypes = [vp, i64, vp, ci, vp, ci, vp, vp, vp]
    L.pcr_evaluate_lists_model.argtypes = [vp, i64, i64, i64, vp, vp, vp, vp, vp, i64, vp, ci, vp, ci, vp, cd, ci, vp, vp, vp, vp, vp, ci]
    L.pcr_evaluate_rerank_model.argtypes = [vp, i64, vp, i64, i64, vp, vp, vp, vp, vp, i64, vp, ci, vp, ci, ci, vp, cd, ci, vp, vp, vp, vp, vp, ci]
    L.pcr_evaluate_rerank.argtypes = [vp, i64, vp, ci, vp, ci, ci, vp, cd, ci, vp, vp, vp, vp, vp]
    L.pcr_fold_in_model.argtypes = [C.POINTER(Parameter), vp, i64, i64, vp, vp, vp, vp, ci, vp, vp, vp]
    L.pcr_fold_in.argtypes = [vp, i64, vp, vp, vp, vp, ci, vp, vp, vp]
    if _LIB_OVERRIDE is None or hasattr(L, "pcr_fold_in_ridge"):
        L.pcr_fold_in_ridge_model.argtypes = [vp, i64, i64, cd, ci, ci, ci, i64, vp, vp, vp, vp, vp, vp]
        L.pcr_fold_in_ridge.argtypes = [vp, ci, i64, vp, vp, vp, vp, vp, vp]
    if _LIB_OVERRIDE is None or hasattr(L, "pcr_fold_in_conf"):
        L.pcr_fold_in_conf_model.argtypes = [vp, i64, i64, cd, ci, cd, ci, ci, i64, vp, vp, vp, vp, vp, vp, vp]
        L.pcr_fold_in_conf.argtypes = [vp, ci, cd, i64, vp, vp, vp, vp, vp, vp, vp]
    if _LIB_OVERRIDE is None or hasattr(L, "pcr_fold_in_nnls"):
        L.pcr_fold_in_nnls_model.argtypes = [vp, i64, i64, cd, ci, ci, ci, i64, vp, vp, vp, vp, vp, vp]
        L.pcr_fold_in_nnls.argtypes = [vp, ci, i64, vp, vp, vp, vp, vp, vp]
    if _LIB_OVERRIDE is None or hasattr(L, "pcr_fold_in_items"):
        L.pcr_fold_in_items_model.argtypes = [C.POINTER(Parameter), vp, i64, vp, i64, vp, vp, vp, i64, vp, vp, vp, vp, ci, vp, vp, vp]
        L.pcr_fold_in_items.argtypes = [vp, vp, i64, vp, vp, vp, vp, ci, vp, vp, vp]
    if _LIB_OVERRIDE is None or hasattr(L, "pcr_explain"):
        L.pcr_explain_model.argtypes = [C.POINTER(Parameter), vp, i64, i64, vp, vp, vp, vp, vp, ci, vp, ci, vp, vp, vp, vp, vp]
        L.pcr_explain.argtypes = [vp, vp, i64, vp, vp, ci, vp, ci, vp, vp, vp, vp, vp]
    if _LIB_OVERRIDE is None or hasattr(L, "pcr_explain_ridge"):
        L.pcr_explain_ridge_model.argtypes = [vp, i64, i64, cd, ci, ci, ci, ci, i64, vp, vp, vp, vp, ci, vp, ci, vp, vp, vp, vp, vp]
        L.pcr_explain_ridge.argtypes = [vp, vp, i64, vp, ci, ci, ci, vp, ci, vp, vp, vp, vp, vp]
    L.pcr_exposure_stats.argtypes = [vp, i64, C.POINTER(i64), C.POINTER(i64), C.POINTER(cd), C.POINTER(cd)]
    L.pcr_profile_enable.argtypes = [vp, ci]
    L.pcr_profile_get.argtypes = [vp, C.c_char_p, C.POINTER(cd), C.POINTER(i64)]
    L.pcr_profile_scope.argtypes = [vp, C.c_char_p, C.POINTER(i64), C.POINTER(i64)]
    L.pcr_profile_launches.argtypes = [vp, C.c_char_p, C.POINTER(i64)]
    L.pcr_profile_reset.argtypes = [vp]
    L.pcr_profile_list.argtypes = [vp, C.c_char_p, i64]
    L.pcr_solver_sync.argtypes = [vp]
    _lib = L
    return L


def _chk(rc):
    if rc != 0:
        raise PcrError(f"libprimalcr error {rc}: {lib().pcr_last_error().decode()}")


def tune(key, value=None):
    """pcr_tune(): a process-wide launch knob read by the next Solver (value None removes it)."""
    _chk(lib().pcr_tune(key.encode(), None if value is None else str(value).encode()))


class tuned:
    """with tuned(spmm_tiles=16, lanes=1): ... -- knobs set for the block, removed afterwards."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        for k, v in self.kw.items():
            tune(k, v)
        return self

    def __exit__(self, *exc):
        for k in self.kw:
            tune(k, None)
        return False


def initial(n, k):
    """util.cpp:80-93 initial()."""
    X = np.empty((n, k), np.float64)
    _chk(lib().pcr_initial(X, n, k))
    return X


def initial_col(n, k):
    """util.cpp:95-101 initial_col(): n x k values 0.1 * drand48() of glibc's unseeded stream, drawn row by row."""
    X = np.empty((n, k), np.float64)
    _chk(lib().pcr_initial_col(X, n, k))
    return X


def initial_rows(n, k, row0, nrows):
    """Rows [row0, row0 + nrows) of initial(n, k) (the stream is sequential: the rows before are generated and dropped)."""
    X = np.empty((nrows, k), np.float64)
    _chk(lib().pcr_initial_rows(X, n, k, row0, nrows))
    return X


def model_save(path, U, V):
    U = np.ascontiguousarray(U, np.float64); V = np.ascontiguousarray(V, np.float64)
    _chk(lib().pcr_model_save(os.fsencode(path), U, U.shape[0], V, V.shape[0], U.shape[1]))


def model_load(path):
    d1, d2, k = C.c_int64(), C.c_int64(), C.c_int64()
    _chk(lib().pcr_model_load(os.fsencode(path), d1, d2, k, None, None))
    U = np.empty((d1.value, k.value)); V = np.empty((d2.value, k.value))
    _chk(lib().pcr_model_load(os.fsencode(path), d1, d2, k, U.ctypes.data, V.ctypes.data))
    return U, V


def partition_users(index, nparts):
    index = np.ascontiguousarray(index, np.int64)
    b = np.empty(nparts + 1, np.int64)
    _chk(lib().pcr_partition_users(index, index.shape[0] - 1, nparts, b))
    return b


def predict(U, V, user, item, device=0):
    """pmf-predict.cpp:56-64 on the GPU (0-based pairs)."""
    U = np.ascontiguousarray(U, np.float64); V = np.ascontiguousarray(V, np.float64)
    user = np.ascontiguousarray(user, np.int32); item = np.ascontiguousarray(item, np.int32)
    out = np.empty(user.shape[0], np.float64)
    _chk(lib().pcr_predict(U, U.shape[0], V, V.shape[0], U.shape[1], user.shape[0], user, item, out, device))
    return out


def _item_filter(allow, candidates, d2, n):
    """Shared by recommend() and Solver.recommend(): the pcr_item_filter of an allow mask (bool / uint8, length d2) and an
    (index, item) pair of candidate rows, one per requested user; returns (filter, the arrays it points into)."""
    f = ItemFilter()
    keep = []
    if allow is not None:
        allow = np.asarray(allow)
        if allow.ndim != 1 or allow.shape[0] != d2:
            raise ValueError(f"allow: a mask of d2 = {d2} entries is expected, got shape {allow.shape}")
        allow = np.ascontiguousarray(allow != 0, np.uint8)
        f.allow = allow.ctypes.data
        keep.append(allow)
    if candidates is not None:
        idx, it = candidates
        idx = np.ascontiguousarray(idx, np.int64); it = np.ascontiguousarray(it, np.int32)
        if idx.ndim != 1 or it.ndim != 1 or idx.shape[0] != n + 1 or idx[-1] != it.shape[0]:
            raise ValueError(f"candidates: index must have one row per requested user (n + 1 = {n + 1} entries), the last equal to "
                             f"len(item) = {it.shape[0]}")
        f.cand_ptr = idx.ctypes.data; f.cand_item = it.ctypes.data
        keep += [idx, it]
    return f, keep


def recommend(U, V, topk, exclude=None, users=None, dtype=PCR_F64, device=0, allow=None, candidates=None):
    """Top-K items per user on the GPU (pcr_recommend_model): descending score, equal scores by ascending item id, rows padded
    with (-1, -inf).  exclude: a Dataset (its training CSR) or an (index, item) pair, or None; users: 0-based ids (None: all).
    allow: a boolean / uint8 mask over the d2 items, eligible where nonzero; candidates: an (index, item) CSR pair with one row
    of 0-based item ids per requested user (any order, no id twice in a row) -- with either, the list is the K best of the items
    that pass every filter (pcr_recommend_filtered_model), with the scores of the unfiltered call bit for bit.
    Returns (items int32 [n, topk], scores float64 [n, topk])."""
    U = np.ascontiguousarray(U, np.float64); V = np.ascontiguousarray(V, np.float64)
    d1, k = U.shape
    idx = it = None
    if exclude is not None:
        if isinstance(exclude, Dataset):
            idx, it, _ = exclude.csr(0)
        else:
            idx, it = exclude
        idx = np.ascontiguousarray(idx, np.int64); it = np.ascontiguousarray(it, np.int32)
        if idx.shape[0] != d1 + 1 or idx[-1] != it.shape[0]:
            raise ValueError(f"exclude: index must have d1 + 1 = {d1 + 1} entries, the last equal to len(item) = {it.shape[0]}")
    if users is not None:
        users = np.ascontiguousarray(users, np.int32)
    n = d1 if users is None else users.shape[0]
    items = np.empty((n, max(int(topk), 1)), np.int32); scores = np.empty((n, max(int(topk), 1)), np.float64)
    if allow is not None or candidates is not None:
        f, _keep = _item_filter(allow, candidates, V.shape[0], n)
        _chk(lib().pcr_recommend_filtered_model(U.ctypes.data, d1, V.ctypes.data, V.shape[0], k, None if idx is None else idx.ctypes.data,
                                                None if it is None else it.ctypes.data, n, None if users is None else users.ctypes.data,
                                                int(topk), int(dtype), C.byref(f), items.ctypes.data, scores.ctypes.data, device))
        return items, scores
    _chk(lib().pcr_recommend_model(U.ctypes.data, d1, V.ctypes.data, V.shape[0], k, None if idx is None else idx.ctypes.data,
                                   None if it is None else it.ctypes.data, n, None if users is None else users.ctypes.data, int(topk),
                                   int(dtype), items.ctypes.data, scores.ctypes.data, device))
    return items, scores


def _rerank_args(topk, pool, theta):
    """Shared by recommend_diverse() and Solver.recommend_diverse(): (topk, pool, theta) checked as the library checks them;
    pool None = min(PCR_RECOMMEND_MAX_K, max(topk, 10 * topk))."""
    topk = int(topk)
    if topk < 1:
        raise ValueError(f"topk = {topk} must be at least 1")
    pool = min(PCR_RECOMMEND_MAX_K, max(topk, 10 * topk)) if pool is None else int(pool)
    if pool < topk or pool > PCR_RECOMMEND_MAX_K:
        raise ValueError(f"pool = {pool} must be in [topk = {topk}, {PCR_RECOMMEND_MAX_K}]")
    theta = float(theta)
    if not 0.0 <= theta <= 1.0:
        raise ValueError(f"theta = {theta} must be in [0, 1]")
    return topk, pool, theta


def recommend_diverse(U, V, topk, pool=None, theta=0.5, exclude=None, users=None, dtype=PCR_F64, device=0):
    """Top-K lists re-ranked by Maximal Marginal Relevance on the GPU (pcr_recommend_diverse_model): topk items taken greedily
    from the `pool` best of recommend(), each time the largest (1 - theta) (s - smin) - theta R max cos to the items already
    taken (cosine of rows of V; theta = 0 is recommend()'s list).  pool None: min(1024, 10 topk).  exclude / users / dtype as
    recommend().  Returns (items int32 [n, topk], scores float64 [n, topk]) in the order taken, rows padded with (-1, -inf)."""
    topk, pool, theta = _rerank_args(topk, pool, theta)
    U = np.ascontiguousarray(U, np.float64); V = np.ascontiguousarray(V, np.float64)
    d1, k = U.shape
    idx = it = None
    if exclude is not None:
        if isinstance(exclude, Dataset):
            idx, it, _ = exclude.csr(0)
        else:
            idx, it = exclude[:2]
        idx = np.ascontiguousarray(idx, np.int64); it = np.ascontiguousarray(it, np.int32)
        if idx.shape[0] != d1 + 1 or idx[-1] != it.shape[0]:
            raise ValueError(f"exclude: index must have d1 + 1 = {d1 + 1} entries, the last equal to len(item) = {it.shape[0]}")
    if users is not None:
        users = np.ascontiguousarray(users, np.int32)
    n = d1 if users is None else users.shape[0]
    items = np.empty((n, topk), np.int32); scores = np.empty((n, topk), np.float64)
    _chk(lib().pcr_recommend_diverse_model(U.ctypes.data, d1, V.ctypes.data, V.shape[0], k, None if idx is None else idx.ctypes.data,
                                           None if it is None else it.ctypes.data, n, None if users is None else users.ctypes.data,
                                           topk, pool, theta, int(dtype), items.ctypes.data, scores.ctypes.data, device))
    return items, scores


def _cap_args(topk, pool, groups, cap, d2):
    """Shared by recommend_capped() and Solver.recommend_capped(): (topk, pool, groups int32 [d2], cap) checked as the library
    checks them; pool None = _rerank_args' default.  d2 None: the length of groups is left to the caller."""
    topk, pool, _ = _rerank_args(topk, pool, 0.0)
    cap = int(cap)
    if cap < 1:
        raise ValueError(f"cap = {cap} must be at least 1")
    if groups is None:
        raise ValueError("groups: one group id per item is expected")
    g = np.asarray(groups)
    if g.ndim != 1 or (d2 is not None and g.shape[0] != d2) or not np.issubdtype(g.dtype, np.integer):
        raise ValueError(f"groups: d2 = {d2} integer group ids are expected, got shape {g.shape} of {g.dtype}")
    if g.size and (g.max() > np.iinfo(np.int32).max or g.min() < np.iinfo(np.int32).min):
        raise ValueError("groups: a group id outside int32")
    return topk, pool, np.ascontiguousarray(g, np.int32), cap


def _cap_result(items, scores, status, st):
    return items, scores, status, dict(users=st.users, exact=st.exact, exhausted=st.exhausted, short_rows=st.short_rows, kept=st.kept)


def recommend_capped(U, V, topk, groups, cap, pool=None, exclude=None, users=None, dtype=PCR_F64, device=0, allow=None):
    """Group-capped top-K lists on the GPU (pcr_recommend_capped_model): the first topk of the `pool` best items of recommend()
    that the rule "at most cap items of one group" keeps.  groups: one integer per item, a negative id = in no group, never
    capped.  pool None: min(1024, 10 topk).  exclude / users / dtype / allow as recommend().  Returns (items int32 [n, topk],
    scores float64 [n, topk], status uint8 [n], stats dict): status PCR_CAP_EXACT = the row is the capped top-K of the whole
    eligible catalogue, PCR_CAP_POOL_EXHAUSTED = a full pool ran out first (the row is a prefix; a larger pool may continue it)."""
    U = np.ascontiguousarray(U, np.float64); V = np.ascontiguousarray(V, np.float64)
    d1, k = U.shape
    topk, pool, groups, cap = _cap_args(topk, pool, groups, cap, V.shape[0])
    idx = it = None
    if exclude is not None:
        if isinstance(exclude, Dataset):
            idx, it, _ = exclude.csr(0)
        else:
            idx, it = exclude[:2]
        idx = np.ascontiguousarray(idx, np.int64); it = np.ascontiguousarray(it, np.int32)
        if idx.shape[0] != d1 + 1 or idx[-1] != it.shape[0]:
            raise ValueError(f"exclude: index must have d1 + 1 = {d1 + 1} entries, the last equal to len(item) = {it.shape[0]}")
    if users is not None:
        users = np.ascontiguousarray(users, np.int32)
    n = d1 if users is None else users.shape[0]
    f, _keep = _item_filter(allow, None, V.shape[0], n)
    items = np.empty((n, topk), np.int32); scores = np.empty((n, topk), np.float64); status = np.empty(n, np.uint8)
    st = CapStats()
    _chk(lib().pcr_recommend_capped_model(U.ctypes.data, d1, V.ctypes.data, V.shape[0], k, None if idx is None else idx.ctypes.data,
                                          None if it is None else it.ctypes.data, n, None if users is None else users.ctypes.data,
                                          topk, pool, groups.ctypes.data, cap, int(dtype), None if allow is None else C.byref(f),
                                          items.ctypes.data, scores.ctypes.data, status.ctypes.data, C.byref(st), device))
    return _cap_result(items, scores, status, st)


def _topn_call(cutoffs, per_user, rows, fn):
    """Shared by evaluate_topn() and Solver.evaluate_topn(): fn(ncut, cutoffs_ptr, stats_ptr, per_user_ptr) -> status."""
    cuts = np.ascontiguousarray(np.atleast_1d(np.asarray(cutoffs)), np.int32)
    ncut = int(cuts.shape[0])
    stats = (TopnStats * max(ncut, 1))()
    pu = np.empty((rows, max(ncut, 1), len(TOPN_FIELDS)), np.float64) if per_user else None
    _chk(fn(ncut, cuts.ctypes.data, C.cast(stats, C.c_void_p), None if pu is None else pu.ctypes.data))
    out = [{f: getattr(stats[c], f) for f, _ in TopnStats._fields_} for c in range(ncut)]
    return (out, pu) if per_user else out


def evaluate_topn(U, V, test, cutoffs=(10,), exclude=None, threshold=-np.inf, dtype=PCR_F64, device=0, per_user=False, allow=None,
                  candidates=None):
    """Full-catalogue top-N evaluation on the GPU (pcr_evaluate_topn_model): every user with a relevant test rating (value >=
    threshold) gets its top max(cutoffs) list, as recommend() returns it, scored against its test items.  test / exclude: a
    Dataset (its test / training CSR) or an (index, item, val) / (index, item) tuple; exclude None: no exclusion.  Returns one
    dict per cutoff (cutoff, users, users_graded, hits, precision, recall, hit_rate, map, ndcg, ndcg_graded) and, with
    per_user, also the array [d1, ncut, 6] of TOPN_FIELDS (NaN for users not counted and for an undefined ndcg_graded).
    allow / candidates as recommend(), with one candidate row per user of the model: the evaluation within the items that pass
    every filter (pcr_evaluate_topn_filtered_model) -- the list is recommend()'s with the same filter, and a test item outside
    the filter is not relevant.  sample_negatives() makes the rows of the sampled-candidate protocol."""
    U = np.ascontiguousarray(U, np.float64); V = np.ascontiguousarray(V, np.float64)
    d1, k = U.shape
    if isinstance(test, Dataset):
        tidx, tit, tval = test.csr(1)
    else:
        tidx, tit, tval = test
    tidx = np.ascontiguousarray(tidx, np.int64); tit = np.ascontiguousarray(tit, np.int32); tval = np.ascontiguousarray(tval, np.float64)
    if tidx.shape[0] != d1 + 1 or tidx[-1] != tit.shape[0] or tit.shape[0] != tval.shape[0]:
        raise ValueError(f"test: index must have d1 + 1 = {d1 + 1} entries, the last equal to len(item) = len(val)")
    idx = it = None
    if exclude is not None:
        if isinstance(exclude, Dataset):
            idx, it, _ = exclude.csr(0)
        else:
            idx, it = exclude[:2]
        idx = np.ascontiguousarray(idx, np.int64); it = np.ascontiguousarray(it, np.int32)
        if idx.shape[0] != d1 + 1 or idx[-1] != it.shape[0]:
            raise ValueError(f"exclude: index must have d1 + 1 = {d1 + 1} entries, the last equal to len(item) = {it.shape[0]}")
    if allow is not None or candidates is not None:
        f, _keep = _item_filter(allow, candidates, V.shape[0], d1)
        return _topn_call(cutoffs, per_user, d1, lambda nc, cp, sp, pp: lib().pcr_evaluate_topn_filtered_model(
            U.ctypes.data, d1, V.ctypes.data, V.shape[0], k, None if idx is None else idx.ctypes.data, None if it is None else it.ctypes.data,
            tidx.ctypes.data, tit.ctypes.data, tval.ctypes.data, nc, cp, float(threshold), int(dtype), C.byref(f), sp, pp, device))
    return _topn_call(cutoffs, per_user, d1, lambda nc, cp, sp, pp: lib().pcr_evaluate_topn_model(
        U.ctypes.data, d1, V.ctypes.data, V.shape[0], k, None if idx is None else idx.ctypes.data, None if it is None else it.ctypes.data,
        tidx.ctypes.data, tit.ctypes.data, tval.ctypes.data, nc, cp, float(threshold), int(dtype), sp, pp, device))


def _ranks_call(per_user, ranks, rows, tnnz, fn):
    """Shared by evaluate_ranks() and Solver.evaluate_ranks(): fn(stats_ptr, per_user_ptr, ranks_ptr) -> status.  Returns the
    summary dict, then the per-user table and / or the ranks array when asked for."""
    stats = RankStats()
    pu = np.empty((rows, len(RANK_FIELDS)), np.float64) if per_user else None
    rk = np.empty(max(int(tnnz), 1), np.int64) if ranks else None
    _chk(fn(C.addressof(stats), None if pu is None else pu.ctypes.data, None if rk is None else rk.ctypes.data))
    out = ({f: getattr(stats, f) for f, _ in RankStats._fields_},)
    if per_user:
        out += (pu,)
    if ranks:
        out += (rk[:int(tnnz)],)
    return out[0] if len(out) == 1 else out


def evaluate_ranks(U, V, test, exclude=None, threshold=-np.inf, dtype=PCR_F64, device=0, per_user=False, ranks=False, allow=None,
                   candidates=None):
    """Exact full-catalogue rank metrics on the GPU (pcr_evaluate_ranks_model): the position of every relevant test item (value >=
    threshold) among all items the user has not rated (exclude given) in the order of recommend().  test / exclude as
    evaluate_topn().  Returns the summary dict (users, users_auc, relevant, mrr, mean_rank, auc, mpr); with per_user also the
    array [d1, 5] of RANK_FIELDS (NaN for users not counted and for an undefined auc); with ranks also the int64 array [tnnz] of
    1-based ranks in the order of the test CSR (0 for ratings below the threshold).
    allow / candidates as evaluate_topn(): the ranks among the items that pass every filter (pcr_evaluate_ranks_filtered_model);
    a test item outside the filter is not relevant and gets rank 0."""
    U = np.ascontiguousarray(U, np.float64); V = np.ascontiguousarray(V, np.float64)
    d1, k = U.shape
    if isinstance(test, Dataset):
        tidx, tit, tval = test.csr(1)
    else:
        tidx, tit, tval = test
    tidx = np.ascontiguousarray(tidx, np.int64); tit = np.ascontiguousarray(tit, np.int32); tval = np.ascontiguousarray(tval, np.float64)
    if tidx.shape[0] != d1 + 1 or tidx[-1] != tit.shape[0] or tit.shape[0] != tval.shape[0]:
        raise ValueError(f"test: index must have d1 + 1 = {d1 + 1} entries, the last equal to len(item) = len(val)")
    idx = it = None
    if exclude is not None:
        if isinstance(exclude, Dataset):
            idx, it, _ = exclude.csr(0)
        else:
            idx, it = exclude[:2]
        idx = np.ascontiguousarray(idx, np.int64); it = np.ascontiguousarray(it, np.int32)
        if idx.shape[0] != d1 + 1 or idx[-1] != it.shape[0]:
            raise ValueError(f"exclude: index must have d1 + 1 = {d1 + 1} entries, the last equal to len(item) = {it.shape[0]}")
    if allow is not None or candidates is not None:
        f, _keep = _item_filter(allow, candidates, V.shape[0], d1)
        return _ranks_call(per_user, ranks, d1, tit.shape[0], lambda sp, pp, rp: lib().pcr_evaluate_ranks_filtered_model(
            U.ctypes.data, d1, V.ctypes.data, V.shape[0], k, None if idx is None else idx.ctypes.data, None if it is None else it.ctypes.data,
            tidx.ctypes.data, tit.ctypes.data, tval.ctypes.data, float(threshold), int(dtype), C.byref(f), sp, pp, rp, device))
    return _ranks_call(per_user, ranks, d1, tit.shape[0], lambda sp, pp, rp: lib().pcr_evaluate_ranks_model(
        U.ctypes.data, d1, V.ctypes.data, V.shape[0], k, None if idx is None else idx.ctypes.data, None if it is None else it.ctypes.data,
        tidx.ctypes.data, tit.ctypes.data, tval.ctypes.data, float(threshold), int(dtype), sp, pp, rp, device))


def sample_negatives(d2, test, train=None, n_neg=99, seed=0, include_test=True, first_user=0):
    """Candidate rows for sampled-candidate evaluation (pcr_sample_negatives, on the host): per user with test ratings, n_neg
    items drawn -- deterministically from (seed, user id) -- among the items in neither its training row nor its test row and,
    with include_test, its distinct test items; rows ascending, a user without test ratings gets an empty row.  test / train: a
    Dataset or an (index, item[, val]) tuple; train None: no training rows.  first_user: the global id of row 0 (a shard).
    Returns (index int64 [rows + 1], item int32), what evaluate_topn() / evaluate_ranks() take as candidates."""
    tidx, tit = test.csr(1)[:2] if isinstance(test, Dataset) else test[:2]
    tidx = np.ascontiguousarray(tidx, np.int64); tit = np.ascontiguousarray(tit, np.int32)
    rows = tidx.shape[0] - 1
    if rows < 0 or tidx[-1] != tit.shape[0]:
        raise ValueError("test: index must have rows + 1 entries, the last equal to len(item)")
    idx = it = None
    if train is not None:
        idx, it = train.csr(0)[:2] if isinstance(train, Dataset) else train[:2]
        idx = np.ascontiguousarray(idx, np.int64); it = np.ascontiguousarray(it, np.int32)
        if idx.shape[0] != rows + 1 or idx[-1] != it.shape[0]:
            raise ValueError(f"train: index must have rows + 1 = {rows + 1} entries, the last equal to len(item) = {it.shape[0]}")
    ptr = np.zeros(rows + 1, np.int64)
    args = (rows, int(d2), None if idx is None else idx.ctypes.data, None if it is None else it.ctypes.data, tidx.ctypes.data, tit.ctypes.data,
            int(first_user), int(n_neg), int(seed) & 0xFFFFFFFFFFFFFFFF, 1 if include_test else 0)
    _chk(lib().pcr_sample_negatives(*args, ptr.ctypes.data, None))
    item = np.empty(max(int(ptr[-1]), 1), np.int32)
    _chk(lib().pcr_sample_negatives(*args, ptr.ctypes.data, item.ctypes.data))
    return ptr, item[:int(ptr[-1])]


def _diversity_call(cutoffs, per_user, exposure, n, d2, fn):
    """Shared by evaluate_diversity() and Solver.evaluate_diversity(): fn(ncut, cutoffs_ptr, stats_ptr, per_user_ptr,
    exposure_ptr) -> status.  Returns the list of per-cutoff dicts, then the per-user table and / or the exposure when asked for."""
    cuts = np.ascontiguousarray(np.atleast_1d(np.asarray(cutoffs)), np.int32)
    ncut = int(cuts.shape[0])
    stats = (DiversityStats * max(ncut, 1))()
    pu = np.empty((n, max(ncut, 1), len(DIVERSITY_FIELDS)), np.float64) if per_user else None
    ex = np.empty((max(ncut, 1), d2), np.int64) if exposure else None
    _chk(fn(ncut, cuts.ctypes.data, C.cast(stats, C.c_void_p), None if pu is None else pu.ctypes.data, None if ex is None else ex.ctypes.data))
    out = ([{f: getattr(stats[c], f) for f, _ in DiversityStats._fields_} for c in range(ncut)],)
    if per_user:
        out += (pu,)
    if exposure:
        out += (ex,)
    return out[0] if len(out) == 1 else out


def evaluate_diversity(U, V, cutoffs=(10,), exclude=None, users=None, dtype=PCR_F64, device=0, per_user=False, exposure=False):
    """Beyond-accuracy metrics of the top max(cutoffs) lists on the GPU (pcr_evaluate_diversity_model): catalogue coverage and the
    Gini index of item exposure, novelty (mean self-information against the popularity of `exclude`'s ratings) and intra-list
    diversity (1 - mean pairwise cosine of the listed rows of V).  exclude: a Dataset (its training CSR) or an (index, item)
    pair -- exclusion and popularity -- or None; users: 0-based ids (None: all).  Returns one dict per cutoff (cutoff, users,
    users_ild, recs, items_covered, coverage, gini, novelty, ild); with per_user also the array [n, ncut, 3] of DIVERSITY_FIELDS
    (row i for users[i]; NaN novelty for an empty list, NaN ild below two items); with exposure also int64 [ncut, d2]."""
    U = np.ascontiguousarray(U, np.float64); V = np.ascontiguousarray(V, np.float64)
    d1, k = U.shape
    idx = it = None
    if exclude is not None:
        if isinstance(exclude, Dataset):
            idx, it, _ = exclude.csr(0)
        else:
            idx, it = exclude[:2]
        idx = np.ascontiguousarray(idx, np.int64); it = np.ascontiguousarray(it, np.int32)
        if idx.shape[0] != d1 + 1 or idx[-1] != it.shape[0]:
            raise ValueError(f"exclude: index must have d1 + 1 = {d1 + 1} entries, the last equal to len(item) = {it.shape[0]}")
    if users is not None:
        users = np.ascontiguousarray(users, np.int32)
    n = d1 if users is None else users.shape[0]
    return _diversity_call(cutoffs, per_user, exposure, n, V.shape[0], lambda nc, cp, sp, pp, ep: lib().pcr_evaluate_diversity_model(
        U.ctypes.data, d1, V.ctypes.data, V.shape[0], k, None if idx is None else idx.ctypes.data, None if it is None else it.ctypes.data,
        n, None if users is None else users.ctypes.data, nc, cp, int(dtype), sp, pp, ep, device))


def _csr_pair(name, csr, d1, with_val):
    """A Dataset or an (index, item[, val]) tuple as contiguous arrays of the library's types, shape-checked against d1."""
    if isinstance(csr, Dataset):
        idx, it, val = csr.csr(1 if with_val else 0)
    elif with_val:
        idx, it, val = csr
    else:
        (idx, it), val = csr[:2], None
    idx = np.ascontiguousarray(idx, np.int64); it = np.ascontiguousarray(it, np.int32)
    if with_val:
        val = np.ascontiguousarray(val, np.float64)
        if idx.shape[0] != d1 + 1 or idx[-1] != it.shape[0] or it.shape[0] != val.shape[0]:
            raise ValueError(f"{name}: index must have d1 + 1 = {d1 + 1} entries, the last equal to len(item) = len(val)")
        return idx, it, val
    if idx.shape[0] != d1 + 1 or idx[-1] != it.shape[0]:
        raise ValueError(f"{name}: index must have d1 + 1 = {d1 + 1} entries, the last equal to len(item) = {it.shape[0]}")
    return idx, it


def _cutoff_args(cutoffs, longest, what):
    """The cutoffs of evaluate_lists() / evaluate_rerank() checked as the library checks them; the last one at most `longest`."""
    cuts = np.ascontiguousarray(np.atleast_1d(np.asarray(cutoffs)), np.int32)
    if cuts.ndim != 1 or not 1 <= cuts.shape[0] <= PCR_TOPN_MAX_CUTOFFS:
        raise ValueError(f"cutoffs: 1 .. {PCR_TOPN_MAX_CUTOFFS} values")
    if cuts[0] < 1 or cuts[-1] > PCR_RECOMMEND_MAX_K or np.any(np.diff(cuts) <= 0):
        raise ValueError(f"cutoffs must be strictly ascending inside [1, {PCR_RECOMMEND_MAX_K}]")
    if longest is not None and cuts[-1] > longest:
        raise ValueError(f"the last cutoff {int(cuts[-1])} is above {what} = {longest}")
    return cuts


def _tradeoff_args(thetas, pool, cutoffs, threshold):
    """Shared by evaluate_rerank() and Solver.evaluate_rerank(): (thetas, pool, cutoffs, threshold) checked as the library checks
    them; topk = the last cutoff, pool None = _rerank_args' default."""
    cuts = _cutoff_args(cutoffs, None, None)
    th = np.ascontiguousarray(np.atleast_1d(np.asarray(thetas, np.float64)))
    if th.ndim != 1 or not 1 <= th.shape[0] <= PCR_RERANK_MAX_THETAS:
        raise ValueError(f"thetas: 1 .. {PCR_RERANK_MAX_THETAS} values")
    pool = _rerank_args(int(cuts[-1]), pool, 0.0)[1]
    for t in th:
        _rerank_args(int(cuts[-1]), pool, t)
    if np.isnan(threshold):
        raise ValueError("threshold is NaN")
    return th, pool, cuts


def _lists_result(groups, n, d2, cuts, acc, per_user, exposure, fn):
    """Shared by evaluate_lists() and the evaluate_rerank()s: fn(topn_ptr, div_ptr, per_user_topn_ptr, per_user_div_ptr,
    exposure_ptr) -> status fills `groups` sets of outputs.  Returns one dict per group: "diversity" (and, with acc, "topn") the
    lists of per-cutoff dicts of evaluate_diversity() / evaluate_topn(); with per_user "per_user_diversity" [n, ncut, 3] (and
    "per_user_topn" [n, ncut, 6], NaN rows for users without a relevant test item); with exposure "exposure" int64 [ncut, d2]."""
    ncut = int(cuts.shape[0])
    ts = (TopnStats * (groups * ncut))() if acc else None
    ds = (DiversityStats * (groups * ncut))()
    put = np.empty((groups, n, ncut, len(TOPN_FIELDS)), np.float64) if per_user and acc else None
    pud = np.empty((groups, n, ncut, len(DIVERSITY_FIELDS)), np.float64) if per_user else None
    ex = np.empty((groups, ncut, d2), np.int64) if exposure else None
    _chk(fn(None if ts is None else C.cast(ts, C.c_void_p), C.cast(ds, C.c_void_p), *(None if a is None else a.ctypes.data for a in (put, pud, ex))))
    out = []
    for g in range(groups):
        r = {"diversity": [{f: getattr(ds[g * ncut + c], f) for f, _ in DiversityStats._fields_} for c in range(ncut)]}
        if acc:
            r["topn"] = [{f: getattr(ts[g * ncut + c], f) for f, _ in TopnStats._fields_} for c in range(ncut)]
        if put is not None:
            r["per_user_topn"] = put[g]
        if pud is not None:
            r["per_user_diversity"] = pud[g]
        if ex is not None:
            r["exposure"] = ex[g]
        out.append(r)
    return out


def evaluate_lists(lists, V, d1=None, users=None, test=None, popularity=None, cutoffs=(10,), threshold=-np.inf, dtype=PCR_F64, per_user=False,
                   exposure=False, device=0):
    """The metrics of evaluate_topn() and evaluate_diversity() over lists the caller brings (pcr_evaluate_lists_model): lists
    int32 [n, L] in list order, -1 padding only at the end of a row, no item twice in a row; row i is for users[i] (None: n == d1
    and row i is user i; d1 None: n).  test: a Dataset (its test CSR) or (index, item, val), None: no accuracy part; popularity: a
    Dataset (its training CSR) or (index, item) for the novelty, None: pop = 0 -- nothing is excluded, the lists are evaluated as
    given.  The last cutoff is at most L.  Returns a dict: "diversity" and (with test) "topn", the per-cutoff dicts of
    evaluate_diversity() / evaluate_topn(); with per_user "per_user_diversity" [n, ncut, 3] and "per_user_topn" [n, ncut, 6] (all
    NaN for a user without a relevant test item); with exposure "exposure" int64 [ncut, d2]."""
    lists = np.ascontiguousarray(lists, np.int32)
    if lists.ndim != 2 or not 1 <= lists.shape[1] <= PCR_RECOMMEND_MAX_K:
        raise ValueError(f"lists must be [n, L] with L in [1, {PCR_RECOMMEND_MAX_K}]")
    V = np.ascontiguousarray(V, np.float64)
    n, L = lists.shape
    d2, k = V.shape
    d1 = n if d1 is None else int(d1)
    if users is not None:
        users = np.ascontiguousarray(users, np.int32)
        if users.shape != (n,):
            raise ValueError(f"users must have one id per list ({n})")
        if n and (users.min() < 0 or users.max() >= d1):
            raise ValueError(f"a user id is outside [0, d1 = {d1})")
    elif n != d1:
        raise ValueError(f"without users there must be d1 = {d1} lists, not {n}")
    cuts = _cutoff_args(cutoffs, L, "the list length L")
    if np.isnan(threshold):
        raise ValueError("threshold is NaN")
    pad = lists < 0
    if np.any(lists < -1) or np.any(lists >= d2):
        raise ValueError(f"a list entry is outside [0, d2 = {d2}) and not -1")
    if np.any(pad[:, :-1] & ~pad[:, 1:]):
        raise ValueError("a list has an item after its -1 padding")
    srt = np.sort(lists, axis=1)
    if np.any((srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] >= 0)):
        raise ValueError("a list holds an item twice")
    t = (None, None, None) if test is None else _csr_pair("test", test, d1, True)
    p = (None, None) if popularity is None else _csr_pair("popularity", popularity, d1, False)
    ptr = lambda a: None if a is None else a.ctypes.data
    return _lists_result(1, n, d2, cuts, test is not None, per_user, exposure, lambda tp, dp, pt, pd, ep: lib().pcr_evaluate_lists_model(
        V.ctypes.data, d2, k, d1, ptr(p[0]), ptr(p[1]), ptr(t[0]), ptr(t[1]), ptr(t[2]), n, ptr(users), L, lists.ctypes.data,
        int(cuts.shape[0]), cuts.ctypes.data, float(threshold), int(dtype), tp, pt, dp, pd, ep, device))[0]


def evaluate_rerank(U, V, thetas, pool=None, cutoffs=(10,), test=None, exclude=None, users=None, threshold=-np.inf, dtype=PCR_F64,
                    per_user=False, exposure=False, device=0):
    """The accuracy / diversity trade-off of recommend_diverse() on the GPU (pcr_evaluate_rerank_model): the catalogue is scored
    once, then for every theta of `thetas` (at most 8) the lists recommend_diverse(topk = max(cutoffs), pool, theta) returns are
    selected and evaluated as evaluate_lists() evaluates them; no list leaves the device.  test / exclude / users / dtype as
    evaluate_topn() and evaluate_diversity() (exclude also gives the popularity; test None: no accuracy part).  Returns one dict
    per theta, shaped as evaluate_lists()'s, with "theta" added."""
    th, pool, cuts = _tradeoff_args(thetas, pool, cutoffs, threshold)
    U = np.ascontiguousarray(U, np.float64); V = np.ascontiguousarray(V, np.float64)
    d1, k = U.shape
    t = (None, None, None) if test is None else _csr_pair("test", test, d1, True)
    x = (None, None) if exclude is None else _csr_pair("exclude", exclude, d1, False)
    if users is not None:
        users = np.ascontiguousarray(users, np.int32)
    n = d1 if users is None else users.shape[0]
    ptr = lambda a: None if a is None else a.ctypes.data
    out = _lists_result(int(th.shape[0]), n, V.shape[0], cuts, test is not None, per_user, exposure,
                        lambda tp, dp, pt, pd, ep: lib().pcr_evaluate_rerank_model(
                            U.ctypes.data, d1, V.ctypes.data, V.shape[0], k, ptr(x[0]), ptr(x[1]), ptr(t[0]), ptr(t[1]), ptr(t[2]), n, ptr(users),
                            int(th.shape[0]), th.ctypes.data, pool, int(cuts.shape[0]), cuts.ctypes.data, float(threshold), int(dtype),
                            tp, dp, pt, pd, ep, device))
    for r, v in zip(out, th):
        r["theta"] = float(v)
    return out


def foldin_boundaries(k=None, dtype=PCR_F64):
    """The user lengths L at which fold_in() changes its code path between L and L + 1 ratings: the bounds of its workgroup
    forms (the same for every rank and storage type)."""
    return [PCR_FOLDIN_WAVE_MAX, PCR_FOLDIN_LDS_MAX]


def _foldin_ratings(ratings):
    """(index int64, item int32, val float64) of fold_in's `ratings`: a Dataset (its training CSR) or an (index, item, val) tuple."""
    index, item, val = ratings.csr(0) if isinstance(ratings, Dataset) else ratings
    index = np.ascontiguousarray(index, np.int64); item = np.ascontiguousarray(item, np.int32); val = np.ascontiguousarray(val, np.float64)
    if index.ndim != 1 or index.shape[0] < 1 or item.shape != val.shape or item.ndim != 1:
        raise ValueError("ratings: (index[n + 1], item[nnz], val[nnz])")
    if index[-1] != item.shape[0]:
        raise ValueError(f"ratings: the last index entry must equal len(item) = {item.shape[0]}")
    return index, item, val


def _foldin_call(n, k, U0, per_user, fn):
    """Shared by fold_in() and Solver.fold_in(): the U0 / output buffers around fn(U0 pointer, U_out pointer, stats pointer,
    per_user pointer); returns (U_new, stats dict[, per_user])."""
    if U0 is not None:
        U0 = np.ascontiguousarray(U0, np.float64)
        if U0.shape != (n, k):
            raise ValueError(f"U0 must be [n, k] = [{n}, {k}]")
    out = np.empty((n, k), np.float64)
    st = FoldinStats()
    pu = np.empty((n, len(PCR_FOLDIN_FIELDS)), np.float64) if per_user else None
    _chk(fn(None if U0 is None else U0.ctypes.data, out.ctypes.data, C.addressof(st), None if pu is None else pu.ctypes.data))
    stats = {f: getattr(st, f) for f, _ in FoldinStats._fields_}
    return (out, stats, pu) if per_user else (out, stats)


def fold_in(V, ratings, lam, solver_type=PCR_SOLVER_PCRPP, U0=None, steps=10, stepsize=1.0, cg_max_iter=None, cg_tol=None, dtype=PCR_F64,
            device=0, per_user=False):
    """Factors for users the model was not trained on, on the GPU (pcr_fold_in_model): with V fixed, each user's
    lambda/2 |u|^2 + pairwise squared hinge loss is minimised by up to `steps` Newton steps (CG + line search) from U0 (None:
    zeros); a user stops early when its gradient is below the reference's threshold (CONVERGED) or when no line-search try
    improves it (STALLED: u stays where it was).  ratings: a Dataset (its training CSR) or an (index, item, val) tuple over V's
    items.  Returns (U_new float64 [n, k], stats dict[, per_user float64 [n, 6] of PCR_FOLDIN_FIELDS])."""
    V = np.ascontiguousarray(V, np.float64)
    if V.ndim != 2:
        raise ValueError("V must be [d2, k]")
    index, item, val = _foldin_ratings(ratings)
    n, k = index.shape[0] - 1, V.shape[1]
    p = Parameter(solver_type=int(solver_type), k=k, stepsize=float(stepsize), precision=int(dtype), device=int(device), **{"lambda": float(lam)})
    if cg_max_iter is not None:
        p.cg_max_iter = int(cg_max_iter)
    if cg_tol is not None:
        p.cg_tol = float(cg_tol)
    return _foldin_call(n, k, U0, per_user, lambda u0, uo, sp, pp: lib().pcr_fold_in_model(
        C.byref(p), V.ctypes.data, V.shape[0], n, index.ctypes.data, item.ctypes.data, val.ctypes.data, u0, int(steps), uo, sp, pp))


def recommend_new_users(V, ratings, lam, topk, solver_type=PCR_SOLVER_PCRPP, U0=None, steps=10, stepsize=1.0, cg_max_iter=None, cg_tol=None,
                        dtype=PCR_F64, device=0):
    """Top-K lists for users the model was not trained on: fold_in(), then recommend(U_new, V, topk, exclude=ratings) -- the
    ratings the users were folded in on are left out.  Returns (items, scores, U_new, stats)."""
    index, item, val = _foldin_ratings(ratings)
    U_new, stats = fold_in(V, (index, item, val), lam, solver_type=solver_type, U0=U0, steps=steps, stepsize=stepsize, cg_max_iter=cg_max_iter,
                           cg_tol=cg_tol, dtype=dtype, device=device)
    items, scores = recommend(U_new, V, topk, exclude=(index, item), dtype=dtype, device=device)
    return items, scores, U_new, stats


def explain_boundaries():
    """The row lengths R at which explain() changes its code path between R and R + 1 ratings -- the bounds of its workgroup forms
    (fold_in()'s) and the first multiples of its rating chunk -- and the list lengths at which it starts another tile: a dict
    with "rows" and "lists"."""
    rows = sorted({PCR_FOLDIN_WAVE_MAX, EXPLAIN_CHUNK, PCR_FOLDIN_LDS_MAX})
    return {"rows": rows, "lists": [EXPLAIN_TILE * t for t in range(1, PCR_EXPLAIN_MAX_L // EXPLAIN_TILE + 1)]}


def _explain_call(n, lists, top, weights, per_pair, per_user, fn, stats_type=ExplainStats, user_fields=PCR_EXPLAIN_USER_FIELDS):
    """Shared by explain(), explain_ridge() and the Solver methods: the list / weight / output buffers around fn(weights pointer, L,
    lists pointer, E, expl_item, expl_contrib, per_pair, per_user, stats pointers); returns (items int32 [n, L, E], contrib float64
    [n, L, E], stats dict[, per_pair float64 [n, L, 4]][, per_user float64 [n, len(user_fields)]])."""
    lists = np.ascontiguousarray(lists, np.int32)
    if lists.ndim != 2 or lists.shape[0] != n:
        raise ValueError(f"lists must be [n, L] with n = {n}")
    L, E = int(lists.shape[1]), int(top)
    if weights is not None:
        weights = np.ascontiguousarray(weights, np.float64)
        if weights.shape != (n,):
            raise ValueError(f"weights must hold {n} values")
    Lb, Eb = max(L, 1), min(max(E, 1), 1024)
    items = np.empty((n, Lb, Eb), np.int32); contrib = np.empty((n, Lb, Eb), np.float64)
    pp = np.empty((n, Lb, len(PCR_EXPLAIN_PAIR_FIELDS)), np.float64) if per_pair else None
    pu = np.empty((n, len(user_fields)), np.float64) if per_user else None
    st = stats_type()
    _chk(fn(None if weights is None else weights.ctypes.data, L, lists.ctypes.data, E, items.ctypes.data, contrib.ctypes.data,
            None if pp is None else pp.ctypes.data, None if pu is None else pu.ctypes.data, C.addressof(st)))
    out = (items, contrib, {f: getattr(st, f) for f, _ in stats_type._fields_})
    return out + ((pp,) if per_pair else ()) + ((pu,) if per_user else ())


def explain(V, ratings, U, lists, lam, top=5, solver_type=PCR_SOLVER_PCRPP, weights=None, dtype=PCR_F64, device=0, per_pair=False,
            per_user=False):
    """Why each listed item scores as it does for a user, on the GPU (pcr_explain_model): the score v_j . u split exactly into one
    signed contribution e_p(j) per item of the user's training row plus a residual that vanishes at a converged row.
    ratings: the users' training rows, a Dataset or an (index, item, val) tuple over V's items; U [n, k] their rows; lists [n, L]
    item ids with -1 padding at the end; top: the contributors reported per listed item, by descending contribution (entries
    <= 0 included: cut at the sign); weights [n]: per-user loss weights c_u (the user is explained at lam / c_u).
    Returns (items int32 [n, L, top] of rated item ids (-1: no more ratings), contrib float64 [n, L, top], stats dict
    [, per_pair float64 [n, L, 4] of PCR_EXPLAIN_PAIR_FIELDS, NaN on padding][, per_user float64 [n, 3] of PCR_EXPLAIN_USER_FIELDS])."""
    V = np.ascontiguousarray(V, np.float64); U = np.ascontiguousarray(U, np.float64)
    if V.ndim != 2 or U.ndim != 2 or U.shape[1] != V.shape[1]:
        raise ValueError("V must be [d2, k] and U [n, k]")
    index, item, val = _foldin_ratings(ratings)
    n, k = index.shape[0] - 1, V.shape[1]
    if U.shape[0] != n:
        raise ValueError(f"U must hold one row per user of ratings ({n})")
    p = Parameter(solver_type=int(solver_type), k=k, precision=int(dtype), device=int(device), **{"lambda": float(lam)})
    return _explain_call(n, lists, top, weights, per_pair, per_user, lambda wp, L, lp, E, ip, cp, pp, up, sp: lib().pcr_explain_model(
        C.byref(p), V.ctypes.data, V.shape[0], n, index.ctypes.data, item.ctypes.data, val.ctypes.data, U.ctypes.data, wp, L, lp, E, ip, cp, pp, up,
        sp))


def explain_ridge_boundaries(k):
    """The row lengths R at which explain_ridge() changes its code path between R and R + 1 ratings at rank k -- no ratings /
    some, the first multiples of the 16 ratings its Gram build stages at a time, and of its rating chunk -- and the list lengths at
    which it starts another tile: a dict with "rows" and "lists".  The kernel has one workgroup form for every length and rank."""
    rows = sorted({0, EXPLAIN_RIDGE_STAGE, 2 * EXPLAIN_RIDGE_STAGE, EXPLAIN_CHUNK, 2 * EXPLAIN_CHUNK})
    return {"rows": rows, "lists": [EXPLAIN_TILE * t for t in range(1, PCR_EXPLAIN_MAX_L // EXPLAIN_TILE + 1)]}


def _explain_ridge_call(n, lists, top, per_pair, per_user, fn):
    return _explain_call(n, lists, top, None, per_pair, per_user, lambda wp, L, lp, E, ip, cp, pp, up, sp: fn(L, lp, E, ip, cp, pp, up, sp),
                         stats_type=ExplainRidgeStats, user_fields=PCR_EXPLAIN_RIDGE_USER_FIELDS)


def explain_ridge(F, ratings, U, lists, lam, top=5, weighted=True, nonneg=False, dtype=PCR_F64, device=0, per_pair=False, per_user=False):
    """Why each listed item scores as it does for a squared-loss (CCDR1 / ridge) row, on the GPU (pcr_explain_ridge_model): with
    A = F[I] the user's rated rows, mu = lam * len (weighted) or lam, and G = A^T A + mu I, the exact minimiser is u* = G^-1 A^T r
    and v_j . u* = sum_p r_p (v_{i_p} . G^-1 v_j): one signed contribution per rated item.  score = v_j . u for the given row u,
    residual = v_j . (u - u*).  nonneg: the system is restricted to the coordinates where the row is > 0 (a row trained with -N 1
    or returned by fold_in_nnls).  U [n, k]: the rows to explain, or None: the minimiser itself (residual exactly 0; not with
    nonneg).  ratings, lists, top and the result as explain(); F = U of a model with an item-major CSR explains item rows by their
    raters.  Returns (items int32 [n, L, top], contrib float64 [n, L, top], stats dict[, per_pair float64 [n, L, 4] of
    PCR_EXPLAIN_PAIR_FIELDS][, per_user float64 [n, 5] of PCR_EXPLAIN_RIDGE_USER_FIELDS])."""
    F = np.ascontiguousarray(F, np.float64)
    if F.ndim != 2:
        raise ValueError("F must be [rows, k]")
    index, item, val = _foldin_ratings(ratings)
    n, k = index.shape[0] - 1, F.shape[1]
    if U is not None:
        U = np.ascontiguousarray(U, np.float64)
        if U.shape != (n, k):
            raise ValueError(f"U must be [n, k] = [{n}, {k}] (or None: the exact minimiser is explained)")
    elif nonneg:
        raise ValueError("nonneg needs the rows U: the free set is read from them")
    return _explain_ridge_call(n, lists, top, per_pair, per_user, lambda L, lp, E, ip, cp, pp, up, sp: lib().pcr_explain_ridge_model(
        F.ctypes.data, F.shape[0], k, float(lam), 1 if weighted else 0, 1 if nonneg else 0, int(dtype), int(device), n, index.ctypes.data,
        item.ctypes.data, val.ctypes.data, None if U is None else U.ctypes.data, L, lp, E, ip, cp, pp, up, sp))


def itemfold_boundaries(k=None, dtype=PCR_F64):
    """The rater counts R at which fold_in_items() changes its code path between R and R + 1 raters: the bounds of its workgroup
    forms (the same for every rank and storage type)."""
    return [PCR_ITEMFOLD_WAVE_MAX, PCR_ITEMFOLD_LDS_MAX]


def rater_scores_boundaries():
    """The training-row lengths L at which fold_in_items()' rater table changes its workgroup form between L and L + 1 ratings."""
    return [PCR_ITEMFOLD_SCORES_WAVE_MAX]


def _itemfold_call(n, k, V0, per_item, fn):
    """Shared by fold_in_items() and Solver.fold_in_items(): the V0 / output buffers around fn(V0 pointer, V_out pointer, stats
    pointer, per_item pointer); returns (rows, stats dict[, per_item])."""
    if V0 is not None:
        V0 = np.ascontiguousarray(V0, np.float64)
        if V0.shape != (n, k):
            raise ValueError(f"V0 must be [n, k] = [{n}, {k}]")
    out = np.empty((n, k), np.float64)
    st = ItemfoldStats()
    pi = np.empty((n, len(PCR_ITEMFOLD_FIELDS)), np.float64) if per_item else None
    _chk(fn(None if V0 is None else V0.ctypes.data, out.ctypes.data, C.addressof(st), None if pi is None else pi.ctypes.data))
    stats = {f: getattr(st, f) for f, _ in ItemfoldStats._fields_}
    return (out, stats, pi) if per_item else (out, stats)


def fold_in_items(U, V, train, new_items, lam, solver_type=PCR_SOLVER_PCRPP, V0=None, steps=10, stepsize=1.0, cg_max_iter=None, cg_tol=None,
                  dtype=PCR_F64, device=0, per_item=False):
    """Rows of V for items a PrimalCR / PrimalCR++ model was not trained on, on the GPU (pcr_fold_in_items_model): with U and the
    trained V fixed, each new item's lambda/2 |v|^2 + the pairwise squared hinge loss of its ratings against its raters' training
    rows is minimised by up to `steps` Newton steps (CG + line search) from V0 (None: zeros); statuses as fold_in()'s.  New items
    are independent of each other: a pair of two new items rated by the same user is not modelled.
    train: the training ratings of U's users, a Dataset (its training CSR) or an (index, item, val) tuple over V's items.
    new_items: (index[n + 1], user, val), item-major: the raters of each new item and their ratings.
    Returns (rows float64 [n, k], stats dict[, per_item float64 [n, 8] of PCR_ITEMFOLD_FIELDS]); np.vstack([V, rows]) serves the
    new items through recommend() and the evaluations as items d2 .. d2 + n - 1."""
    U = np.ascontiguousarray(U, np.float64); V = np.ascontiguousarray(V, np.float64)
    if U.ndim != 2 or V.ndim != 2 or U.shape[1] != V.shape[1]:
        raise ValueError("U must be [d1, k] and V [d2, k]")
    tindex, titem, tval = _foldin_ratings(train)
    if tindex.shape[0] - 1 != U.shape[0]:
        raise ValueError(f"train must hold one row per user of U ({U.shape[0]})")
    index, user, val = _foldin_ratings(new_items)
    n, k = index.shape[0] - 1, V.shape[1]
    p = Parameter(solver_type=int(solver_type), k=k, stepsize=float(stepsize), precision=int(dtype), device=int(device), **{"lambda": float(lam)})
    if cg_max_iter is not None:
        p.cg_max_iter = int(cg_max_iter)
    if cg_tol is not None:
        p.cg_tol = float(cg_tol)
    return _itemfold_call(n, k, V0, per_item, lambda v0, vo, sp, pp: lib().pcr_fold_in_items_model(
        C.byref(p), U.ctypes.data, U.shape[0], V.ctypes.data, V.shape[0], tindex.ctypes.data, titem.ctypes.data, tval.ctypes.data,
        n, index.ctypes.data, user.ctypes.data, val.ctypes.data, v0, int(steps), vo, sp, pp))


def ridge_form(n, k):
    """The form fold_in_ridge() solves a user of n ratings in at rank k (include/primalcr.h): PCR_RIDGE_DUAL for n <= k and
    n <= PCR_RIDGE_DIRECT_MAX, PCR_RIDGE_PRIMAL for n > k when k padded to 16 is <= PCR_RIDGE_DIRECT_MAX, PCR_RIDGE_CG otherwise."""
    if n <= k and n <= PCR_RIDGE_DIRECT_MAX:
        return PCR_RIDGE_DUAL
    if n > k and (k + 15) // 16 * 16 <= PCR_RIDGE_DIRECT_MAX:
        return PCR_RIDGE_PRIMAL
    return PCR_RIDGE_CG


def ridge_boundaries(k):
    """The user lengths L at which fold_in_ridge() changes its form between L and L + 1 ratings at rank k."""
    top = max(int(k), PCR_RIDGE_DIRECT_MAX) + 1
    return [L for L in range(top) if ridge_form(L, k) != ridge_form(L + 1, k)]


def _ridge_call(n, k, per_user, fn):
    """Shared by fold_in_ridge() and Solver.fold_in_ridge(): the buffers around fn(U_out pointer, stats pointer, per_user
    pointer); returns (rows, stats dict[, per_user])."""
    out = np.empty((n, k), np.float64)
    st = RidgeStats()
    pu = np.empty((n, len(PCR_RIDGE_FIELDS)), np.float64) if per_user else None
    _chk(fn(out.ctypes.data, C.addressof(st), None if pu is None else pu.ctypes.data))
    stats = {f: getattr(st, f) for f, _ in RidgeStats._fields_}
    return (out, stats, pu) if per_user else (out, stats)


def fold_in_ridge(F, ratings, lam, weighted=True, dtype=PCR_F64, device=0, per_user=False):
    """Squared-loss factors for rows a model was not trained on, on the GPU (pcr_fold_in_ridge_model): with the factor matrix F
    [rows, k] fixed, each new user's row is the exact minimiser of |r - F[I] u|^2 + mu |u|^2 over its ratings r on rows I of F,
    with mu = lam * len(r) (weighted: CCDR1's regulariser, solver type 0) or mu = lam (weighted=False: the plain ridge).
    ratings: a Dataset (its training CSR) or an (index, item, val) tuple over F's rows, as fold_in() takes.
    New users: F = V and the users' ratings over the items.  New ITEMS: F = U and the item-major CSR (row j: the users who rated
    item j and their ratings); the rows returned are rows of V.
    Returns (rows float64 [n, k], stats dict[, per_user float64 [n, 6] of PCR_RIDGE_FIELDS]); loss and obj are evaluated at the
    returned rows, which are rounded to `dtype`."""
    F = np.ascontiguousarray(F, np.float64)
    if F.ndim != 2:
        raise ValueError("F must be [rows, k]")
    index, item, val = _foldin_ratings(ratings)
    n, k = index.shape[0] - 1, F.shape[1]
    return _ridge_call(n, k, per_user, lambda uo, sp, pp: lib().pcr_fold_in_ridge_model(
        F.ctypes.data, F.shape[0], k, float(lam), 1 if weighted else 0, int(dtype), int(device), n, index.ctypes.data, item.ctypes.data,
        val.ctypes.data, uo, sp, pp))


def recommend_new_users_ridge(V, ratings, lam, topk, weighted=True, dtype=PCR_F64, device=0):
    """Top-K lists for users a squared-loss model was not trained on: fold_in_ridge(), then recommend(U_new, V, topk,
    exclude=ratings) -- the ratings the users were folded in on are left out.  Returns (items, scores, U_new, stats)."""
    index, item, val = _foldin_ratings(ratings)
    U_new, stats = fold_in_ridge(V, (index, item, val), lam, weighted=weighted, dtype=dtype, device=device)
    items, scores = recommend(U_new, V, topk, exclude=(index, item), dtype=dtype, device=device)
    return items, scores, U_new, stats


def conf_form(n, k, implicit=False):
    """The form fold_in_conf() solves a user of n ratings in at rank k (include/primalcr.h), a function of (n, k, alpha > 0) alone:
    ridge_form(n, k) for alpha == 0; for alpha > 0 (implicit) PCR_RIDGE_PRIMAL at every n while k padded to 16 is
    <= PCR_RIDGE_DIRECT_MAX -- the alpha G term makes the system k x k whatever the length -- and PCR_RIDGE_CG beyond."""
    if not implicit:
        return ridge_form(n, k)
    return PCR_RIDGE_PRIMAL if (k + 15) // 16 * 16 <= PCR_RIDGE_DIRECT_MAX else PCR_RIDGE_CG


def conf_block(n, k, implicit=False):
    """The workgroup width fold_in_conf() solves that user on: 256 threads for the CG form, beyond PCR_RIDGE_WAVE_MAX ratings and
    for an implicit primal system of more than 4 x 4 tiles (k padded to 16 > 64), else one wave (64)."""
    if conf_form(n, k, implicit) == PCR_RIDGE_CG or n > PCR_RIDGE_WAVE_MAX:
        return 256
    return 256 if implicit and (k + 15) // 16 * 16 > 64 else 64


def conf_boundaries(k, implicit=False):
    """The user lengths L at which fold_in_conf() changes its form or its workgroup width between L and L + 1 ratings at rank k."""
    top = max(int(k), PCR_RIDGE_DIRECT_MAX) + 1
    key = lambda n: (conf_form(n, k, implicit), conf_block(n, k, implicit))
    return [L for L in range(top) if key(L) != key(L + 1)]


def _conf_weights(weights, nnz):
    if weights is None:
        return None
    w = np.ascontiguousarray(weights, np.float64)
    if w.shape != (nnz,):
        raise ValueError(f"weights must hold one weight per rating ({nnz})")
    return w


def fold_in_conf(F, ratings, lam, weights=None, alpha=0.0, weighted=True, dtype=PCR_F64, device=0, per_user=False):
    """fold_in_ridge() under the objective of a model trained with rating weights (Solver.set_rating_weights) and / or implicit
    feedback (Solver.set_implicit), on the GPU (pcr_fold_in_conf_model): with F [rows, k] fixed and G = F^T F, each row is the
    exact minimiser of  sum_p c_p (r_p - F[I_p].u)^2 + alpha (u^T G u - sum_p (F[I_p].u)^2) + mu |u|^2  with mu = lam * (sum_p c_p
    + alpha (rows - len)) (weighted) or mu = lam.  weights: one c_p > 0 per rating in the ratings' own order (None: ones); alpha
    >= 0: the weight of every unrated cell, a rating 0.  weights=None and alpha=0 is fold_in_ridge(), bit for bit.  New ITEMS:
    F = U and the item-major CSR.  Returns (rows float64 [n, k], stats dict[, per_user float64 [n, 6] of PCR_RIDGE_FIELDS]); loss
    and obj are evaluated at the returned rows, which are rounded to `dtype`."""
    F = np.ascontiguousarray(F, np.float64)
    if F.ndim != 2:
        raise ValueError("F must be [rows, k]")
    index, item, val = _foldin_ratings(ratings)
    n, k = index.shape[0] - 1, F.shape[1]
    w = _conf_weights(weights, item.shape[0])
    return _ridge_call(n, k, per_user, lambda uo, sp, pp: lib().pcr_fold_in_conf_model(
        F.ctypes.data, F.shape[0], k, float(lam), 1 if weighted else 0, float(alpha), int(dtype), int(device), n, index.ctypes.data,
        item.ctypes.data, val.ctypes.data, None if w is None else w.ctypes.data, uo, sp, pp))


def recommend_new_users_conf(V, ratings, lam, topk, weights=None, alpha=0.0, weighted=True, dtype=PCR_F64, device=0):
    """Top-K lists for users a weighted / implicit squared-loss model was not trained on: fold_in_conf(), then recommend(U_new, V,
    topk, exclude=ratings).  Returns (items, scores, U_new, stats)."""
    index, item, val = _foldin_ratings(ratings)
    U_new, stats = fold_in_conf(V, (index, item, val), lam, weights=weights, alpha=alpha, weighted=weighted, dtype=dtype, device=device)
    items, scores = recommend(U_new, V, topk, exclude=(index, item), dtype=dtype, device=device)
    return items, scores, U_new, stats


def nnls_form(k):
    """The form fold_in_nnls() takes at rank k (include/primalcr.h), a function of k alone: PCR_NNLS_DIRECT when k padded to 16 is
    <= PCR_RIDGE_DIRECT_MAX, PCR_NNLS_CG beyond."""
    return PCR_NNLS_DIRECT if (k + 15) // 16 * 16 <= PCR_RIDGE_DIRECT_MAX else PCR_NNLS_CG


def _nnls_call(n, k, per_user, fn):
    """Shared by fold_in_nnls() and Solver.fold_in_nnls(): the buffers around fn(U_out pointer, stats pointer, per_user pointer);
    returns (rows, stats dict[, per_user])."""
    out = np.empty((n, k), np.float64)
    st = NnlsStats()
    pu = np.empty((n, len(PCR_NNLS_FIELDS)), np.float64) if per_user else None
    _chk(fn(out.ctypes.data, C.addressof(st), None if pu is None else pu.ctypes.data))
    stats = {f: getattr(st, f) for f, _ in NnlsStats._fields_}
    return (out, stats, pu) if per_user else (out, stats)


def fold_in_nnls(F, ratings, lam, weighted=True, dtype=PCR_F64, device=0, per_user=False):
    """Non-negative factors for rows a model was not trained on, on the GPU (pcr_fold_in_nnls_model): fold_in_ridge()'s problem
    under u >= 0, the constraint of a CCDR1 model trained with -N 1 -- each row is the exact minimiser of
    |r - F[I] u|^2 + mu |u|^2 over u >= 0, found by block principal pivoting around exact solves.  Arguments as fold_in_ridge().
    Returns (rows float64 [n, k], every entry >= 0, stats dict[, per_user float64 [n, 7] of PCR_NNLS_FIELDS]); loss and obj are
    evaluated at the returned rows, which are rounded to `dtype`."""
    F = np.ascontiguousarray(F, np.float64)
    if F.ndim != 2:
        raise ValueError("F must be [rows, k]")
    index, item, val = _foldin_ratings(ratings)
    n, k = index.shape[0] - 1, F.shape[1]
    return _nnls_call(n, k, per_user, lambda uo, sp, pp: lib().pcr_fold_in_nnls_model(
        F.ctypes.data, F.shape[0], k, float(lam), 1 if weighted else 0, int(dtype), int(device), n, index.ctypes.data, item.ctypes.data,
        val.ctypes.data, uo, sp, pp))


def recommend_new_users_nnls(V, ratings, lam, topk, weighted=True, dtype=PCR_F64, device=0):
    """Top-K lists for users a non-negative model was not trained on: fold_in_nnls(), then recommend(U_new, V, topk,
    exclude=ratings) -- the ratings the users were folded in on are left out.  Returns (items, scores, U_new, stats)."""
    index, item, val = _foldin_ratings(ratings)
    U_new, stats = fold_in_nnls(V, (index, item, val), lam, weighted=weighted, dtype=dtype, device=device)
    items, scores = recommend(U_new, V, topk, exclude=(index, item), dtype=dtype, device=device)
    return items, scores, U_new, stats


def exposure_stats(x):
    """The closing arithmetic of one exposure row (pcr_exposure_stats): dict(recs, items_covered, coverage, gini)."""
    x = np.ascontiguousarray(x, np.int64)
    if x.ndim != 1:
        raise ValueError("exposure_stats: one exposure row (d2 counts)")
    recs, cov, coverage, gini = C.c_int64(), C.c_int64(), C.c_double(), C.c_double()
    _chk(lib().pcr_exposure_stats(x.ctypes.data, x.shape[0], recs, cov, coverage, gini))
    return {"recs": recs.value, "items_covered": cov.value, "coverage": coverage.value, "gini": gini.value}


def comm_unique_id() -> bytes:
    buf = C.create_string_buffer(128)
    _chk(lib().pcr_comm_unique_id(buf))
    return buf.raw


class Dataset:
    """load() + convert(): util.cpp:6-25, util.cpp:219-274."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def load(cls, path, cache=None, threads=0):
        """cache: path of the binary side-car (read if it matches the text files, else rebuilt)."""
        h = C.c_void_p()
        if cache is None and threads > 0:
            _chk(lib().pcr_dataset_load_mt(os.fsencode(path), threads, C.byref(h)))
        elif cache is None:
            _chk(lib().pcr_dataset_load(os.fsencode(path), C.byref(h)))
        else:
            _chk(lib().pcr_dataset_load_cached(os.fsencode(path), threads, os.fsencode(cache), C.byref(h)))
        return cls(h)

    @classmethod
    def load_cache(cls, cache):
        h = C.c_void_p()
        _chk(lib().pcr_dataset_load_cache(os.fsencode(cache), C.byref(h)))
        return cls(h)

    def save_cache(self, cache):
        _chk(lib().pcr_dataset_save_cache(self._h, os.fsencode(cache)))

    @classmethod
    def from_triplets(cls, d1, d2, user, item, val, tuser=None, titem=None, tval=None):
        user = np.ascontiguousarray(user, np.int32); item = np.ascontiguousarray(item, np.int32)
        val = np.ascontiguousarray(val, np.float64)
        tn = 0 if tuser is None else len(tuser)
        if tn:
            tuser = np.ascontiguousarray(tuser, np.int32); titem = np.ascontiguousarray(titem, np.int32)
            tval = np.ascontiguousarray(tval, np.float64)
            targs = (tuser.ctypes.data, titem.ctypes.data, tval.ctypes.data)
        else:
            targs = (None, None, None)
        h = C.c_void_p()
        _chk(lib().pcr_dataset_from_triplets(d1, d2, len(user), user.ctypes.data, item.ctypes.data, val.ctypes.data,
                                             tn, *targs, C.byref(h)))
        return cls(h)

    @classmethod
    def from_csr(cls, d1, d2, index, item, val, tindex=None, titem=None, tval=None):
        """From arrays already in the SparseMat layout (index int64[d1+1], item int32 ascending per user, val float64)."""
        index = np.ascontiguousarray(index, np.int64); item = np.ascontiguousarray(item, np.int32)
        val = np.ascontiguousarray(val, np.float64)
        targs = (None, None, None)
        if tindex is not None:
            tindex = np.ascontiguousarray(tindex, np.int64); titem = np.ascontiguousarray(titem, np.int32)
            tval = np.ascontiguousarray(tval, np.float64)
            targs = (tindex.ctypes.data, titem.ctypes.data, tval.ctypes.data)
        h = C.c_void_p()
        _chk(lib().pcr_dataset_from_csr(d1, d2, index.ctypes.data, item.ctypes.data, val.ctypes.data, *targs, C.byref(h)))
        return cls(h)

    @classmethod
    def from_ratings(cls, R):
        if hasattr(R, "index"):                       # synth.CsrRatings (the C++ generator): no triplet round trip
            return cls.from_csr(R.d1, R.d2, R.index, R.item, R.val, R.tindex, R.titem, R.tval)
        return cls.from_triplets(R.d1, R.d2, R.user, R.item, R.val, R.tuser, R.titem, R.tval)

    def dims(self):
        a, b, c, d = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        _chk(lib().pcr_dataset_dims(self._h, a, b, c, d))
        return a.value, b.value, c.value, d.value

    def csr(self, which=0):
        d1, d2, nnz, tnnz = self.dims()
        n = nnz if which == 0 else tnnz
        idx = np.empty(d1 + 1, np.int64); item = np.empty(max(n, 1), np.int64); val = np.empty(max(n, 1), np.float64)
        _chk(lib().pcr_dataset_csr(self._h, which, idx.ctypes.data, item.ctypes.data, val.ctypes.data))
        return idx, item[:n], val[:n]

    def count_pairs(self, solver_type=PCR_SOLVER_PCRPP):
        return lib().pcr_dataset_count_pairs(self._h, solver_type)

    def user_pairs(self, solver_type=PCR_SOLVER_PCRPP):
        """|Omega_u| per user under the solver's level bucketing (int64, d1 entries); its sum is count_pairs."""
        pairs = np.zeros(max(self.dims()[0], 1), np.int64)
        _chk(lib().pcr_dataset_user_pairs(self._h, solver_type, pairs.ctypes.data))
        return pairs[:self.dims()[0]]

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.pcr_dataset_free(self._h)
            self._h = None


def user_weights(ds: Dataset, scheme=PCR_WEIGHT_PAIRS, solver_type=PCR_SOLVER_PCRPP):
    """Per-user loss weights for Solver.set_user_weights by scheme: PCR_WEIGHT_UNIFORM (all 1), PCR_WEIGHT_PAIRS (every user
    with a comparable pair carries the same mass: sum w_u |Omega_u| = |Omega|) or PCR_WEIGHT_RATINGS (sum w_u n_u = nnz)."""
    d1 = ds.dims()[0]
    w = np.ones(max(d1, 1), np.float64)
    _chk(lib().pcr_user_weights(ds._h, solver_type, scheme, w.ctypes.data))
    return w[:d1]


def match_weights(ds: Dataset, user, item, w):
    """(user, item, weight) triplets, ids 0-based and in any order, -> the weights in Dataset.csr() order (pcr_dataset_match_weights).
    Every training rating must be named exactly once."""
    user = np.ascontiguousarray(user, np.int32); item = np.ascontiguousarray(item, np.int32); w = np.ascontiguousarray(w, np.float64)
    if not (user.ndim == 1 and user.shape == item.shape == w.shape):
        raise ValueError("user, item and weight must be vectors of one length")
    out = np.zeros(max(ds.dims()[2], 1), np.float64)
    _chk(lib().pcr_dataset_match_weights(ds._h, user.shape[0], user.ctypes.data, item.ctypes.data, w.ctypes.data, out.ctypes.data))
    return out[:ds.dims()[2]]


def rating_weights_popularity(ds: Dataset, gamma):
    """Per-rating weights for Solver.set_rating_weights, in Dataset.csr() order: w_z = (n_max / n_item(z))^gamma, the inverse of a
    power-law propensity in the item's popularity (gamma = 0: ones).  Not normalised: the weighted objective does not need it."""
    nnz = ds.dims()[2]
    w = np.ones(max(nnz, 1), np.float64)
    _chk(lib().pcr_rating_weights_popularity(ds._h, float(gamma), w.ctypes.data))
    return w[:nnz]


class Solver:
    """Device solver: the reference's pcrpp()/pcr() and their building blocks on one MI355X."""

    def __init__(self, ds: Dataset, param: Parameter, rank=0, nranks=1, shard=None):
        """shard = (first_user, d1_total): ds holds ONLY this rank's users (pcr_solver_create_shard)."""
        self.ds, self.param, self.rank, self.nranks = ds, param, rank, nranks
        self.d1, self.d2, self.nnz, self.tnnz = ds.dims()
        self.k = param.k
        h = C.c_void_p()
        if shard is None:
            _chk(lib().pcr_solver_create(ds._h, C.byref(param), rank, nranks, C.byref(h)))
        else:
            _chk(lib().pcr_solver_create_shard(ds._h, C.byref(param), rank, nranks, int(shard[0]), int(shard[1]), C.byref(h)))
            self.d1 = int(shard[1])
        self._h = h
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        _chk(lib().pcr_solver_shard(h, a, b, c))
        self.first_user, self.n_users, self.nnz_local = a.value, b.value, c.value

    def set_ccd_params(self, params=None, **kw):
        """CCDR1 (solver type 0): a CcdParameter, or its fields as keywords (maxinneriter, eps, do_nmf)."""
        p = params if params is not None else CcdParameter(**kw)
        _chk(lib().pcr_solver_set_ccd_params(self._h, C.byref(p)))

    def comm_init(self, uid: bytes):
        buf = C.create_string_buffer(uid, 128)
        _chk(lib().pcr_solver_comm_init(self._h, buf))

    def comm_init_p2p(self, shm_name: str):
        """Direct peer-to-peer exchange (every rank of the node calls it with the same '/name')."""
        _chk(lib().pcr_solver_comm_init_p2p(self._h, shm_name.encode()))

    def counter(self, name):
        v = C.c_double()
        _chk(lib().pcr_solver_counter(self._h, name.encode(), v))
        return v.value

    def setup_phases(self):
        """[(phase, ms)] of pcr_solver_create, in order."""
        out, i = [], 0
        name, ms = C.c_char_p(), C.c_double()
        while lib().pcr_solver_setup_phase(self._h, i, C.byref(name), C.byref(ms)) == 0:
            out.append((name.value.decode(), ms.value)); i += 1
        return out

    def ustep_classes(self):
        """Profile slot names of the U step's length classes on this rank."""
        buf = C.create_string_buffer(4096)
        _chk(lib().pcr_solver_ustep_classes(self._h, buf, 4096))
        return [n for n in buf.value.decode().split(",") if n]

    def class_row_gathers(self):
        """{U-step class slot: rows of V it has gathered since the solver was created} (needs tuned(count_rows=1))."""
        return {n: self.counter("ustep_row_gathers/" + n) for n in self.ustep_classes()}

    def comm_nranks(self):
        return lib().pcr_solver_comm_nranks(self._h)

    def set_local_only(self, on=True):
        _chk(lib().pcr_solver_set_local_only(self._h, int(on)))

    def set_factors(self, U=None, V=None):
        U = None if U is None else np.ascontiguousarray(U, np.float64)
        V = None if V is None else np.ascontiguousarray(V, np.float64)
        _chk(lib().pcr_solver_set_factors(self._h, None if U is None else U.ctypes.data,
                                          None if V is None else V.ctypes.data))

    def get_factors(self):
        U = np.zeros((self.d1, self.k)); V = np.zeros((self.d2, self.k))
        _chk(lib().pcr_solver_get_factors(self._h, U.ctypes.data, V.ctypes.data))
        return U, V

    def set_factors_local(self, U_local=None, V=None):
        """U_local: this rank's n_users x k rows only."""
        U = None if U_local is None else np.ascontiguousarray(U_local, np.float64)
        V = None if V is None else np.ascontiguousarray(V, np.float64)
        if U is not None and U.shape != (self.n_users, self.k):
            raise ValueError(f"U_local must be {self.n_users} x {self.k}")
        _chk(lib().pcr_solver_set_factors_local(self._h, None if U is None else U.ctypes.data, None if V is None else V.ctypes.data))

    def set_user_weights(self, w=None, local=False):
        """Per-user loss weights c_u > 0 (PrimalCR / PrimalCR++): the solver then minimises sum_u c_u L_u + lambda/2 (|U|^2 + |V|^2).
        w: one weight per user of the job (with local=True: this rank's n_users only); None returns to the unweighted problem."""
        fn = lib().pcr_solver_set_user_weights_local if local else lib().pcr_solver_set_user_weights
        if w is None:
            _chk(fn(self._h, None))
            self.user_weights = None
            return
        w = np.ascontiguousarray(w, np.float64)
        want = self.n_users if local else self.d1
        if w.shape != (want,):
            raise ValueError(f"w must hold {want} weights")
        _chk(fn(self._h, w.ctypes.data))
        self.user_weights = w.copy()                        # (Solver.explain's default; the library's entry reads the caller's)

    def set_rating_weights(self, w=None):
        """Per-rating confidence weights c_z > 0 (CCDR1): the solver then minimises sum_z c_z (r_z - u_i . v_j)^2 + lambda (sum_i W_i
        |u_i|^2 + sum_j W_j |v_j|^2), W = a row's sum of c_z.  w: a vector of nnz weights in Dataset.csr() order, or a (user, item,
        weight) tuple of vectors (0-based ids, any order, every training rating exactly once), or None for the unweighted problem.
        Ends a running training like set_factors; the weights survive set_factors and set_ccd_params."""
        if w is None:
            _chk(lib().pcr_solver_set_rating_weights(self._h, None))
            return
        if isinstance(w, tuple):
            if len(w) != 3:
                raise ValueError("a tuple must be (user, item, weight)")
            w = match_weights(self.ds, *w)
        w = np.ascontiguousarray(w, np.float64)
        if w.shape != (self.nnz,):
            raise ValueError(f"w must hold {self.nnz} weights")
        _chk(lib().pcr_solver_set_rating_weights(self._h, w.ctypes.data))

    def set_implicit(self, alpha):
        """Implicit feedback (CCDR1): every unrated cell becomes a rating 0 of weight alpha > 0, in the loss and in the regulariser
        (W = a row's total weight, the unrated cells included); with set_rating_weights(1 + a * count) and alpha = 1 this is the
        confidence model of Hu, Koren and Volinsky.  alpha: finite and >= 0, stored in the solver's precision; 0 returns to the
        explicit kernels.  Ends a running training like set_factors; survives set_factors, set_ccd_params and set_rating_weights."""
        _chk(lib().pcr_solver_set_implicit(self._h, float(alpha)))

    def get_factors_local(self):
        U = np.zeros((self.n_users, self.k)); V = np.zeros((self.d2, self.k))
        _chk(lib().pcr_solver_get_factors_local(self._h, U.ctypes.data, V.ctypes.data))
        return U, V

    def comp_m(self, want=True):
        m = np.empty(max(self.nnz_local, 1)) if want else None
        _chk(lib().pcr_comp_m(self._h, None if m is None else m.ctypes.data))
        return None if m is None else m[:self.nnz_local]

    def objective(self):
        o = C.c_double()
        _chk(lib().pcr_objective(self._h, o))
        return o.value

    def obtain_g(self):
        g = np.empty((self.d2, self.k))
        _chk(lib().pcr_obtain_g(self._h, g))
        return g

    def compute_Ha(self, a):
        a = np.ascontiguousarray(a, np.float64)
        Ha = np.empty((self.d2, self.k))
        _chk(lib().pcr_compute_Ha(self._h, a, Ha))
        return Ha

    def solve_delta(self, g):
        g = np.ascontiguousarray(g, np.float64)
        d = np.empty((self.d2, self.k)); it = C.c_int()
        _chk(lib().pcr_solve_delta(self._h, g, d, it))
        return d, it.value

    def update_V(self):
        o = C.c_double(); info = (C.c_int * 3)()
        _chk(lib().pcr_update_V(self._h, o, info))
        return o.value, dict(cg=info[0], ls=info[1], accepted=info[2])

    def update_U(self):
        o = C.c_double(); info = (C.c_int64 * 2)()
        _chk(lib().pcr_update_U(self._h, o, info))
        return o.value, dict(cg=info[0], ls=info[1])

    def evaluate(self, which=0, ndcg_k=10):
        e, n = C.c_double(), C.c_double()
        _chk(lib().pcr_evaluate(self._h, which, ndcg_k, e, n))
        return e.value, n.value

    def train(self, log=None):
        """pcrpp()/pcr()/ccdr1(): returns (per-iteration records, log lines)."""
        hist = (IterStats * (self.param.maxiter + 1))()
        lines = []

        def _cb(_ctx, s):
            lines.append(s.decode())
            if log:
                log(s.decode())
        cb = _LOG_FN(_cb)
        _chk(lib().pcr_train(self._h, C.cast(cb, C.c_void_p), None, hist))
        recs = [{k: getattr(h, k) for k, _ in IterStats._fields_} for h in hist]
        return recs, lines

    def iterate(self, n):
        """n outer iterations (V step + U step; for CCDR1 all k ranks), no evaluation, one host round trip each; returns their
        records."""
        hist = (IterStats * max(n, 1))()
        _chk(lib().pcr_iterate(self._h, n, hist))
        return [{k: getattr(h, k) for k, _ in IterStats._fields_} for h in hist[:n]]

    def profile(self, on=True, period=1):
        """Per-kernel HIP-event timing; period > 1 times every period-th launch of each kernel."""
        _chk(lib().pcr_profile_enable(self._h, (period if period > 1 else 1) if on else 0))

    def profile_reset(self):
        _chk(lib().pcr_profile_reset(self._h))

    def profile_get(self, name):
        ms, n = C.c_double(), C.c_int64()
        _chk(lib().pcr_profile_get(self._h, name.encode(), ms, n))
        return ms.value, n.value

    def profile_launches(self, name):
        """Launches of the slot since the last reset, timed or not."""
        n = C.c_int64()
        _chk(lib().pcr_profile_launches(self._h, name.encode(), n))
        return n.value

    def profile_scope(self, name):
        """(ratings, users) one launch of the slot covers on this rank."""
        a, b = C.c_int64(), C.c_int64()
        _chk(lib().pcr_profile_scope(self._h, name.encode(), a, b))
        return a.value, b.value

    def profile_all(self):
        """{slot name: (total ms, launches)} of every kernel timed so far."""
        buf = C.create_string_buffer(4096)
        _chk(lib().pcr_profile_list(self._h, buf, 4096))
        names = [n for n in buf.value.decode().split(",") if n]
        return {n: self.profile_get(n) for n in names}

    def recommend(self, topk=10, users=None, exclude_train=True, allow=None, candidates=None):
        """Top-K items per user from the device factors (pcr_recommend), in the solver's storage type.  users: GLOBAL 0-based
        ids of this rank's shard (None: all of them, in order).  allow / candidates as recommend() (pcr_recommend_filtered).
        Returns (items int32 [n, topk], scores float64 [n, topk])."""
        if users is not None:
            users = np.ascontiguousarray(users, np.int32)
        n = self.n_users if users is None else users.shape[0]
        items = np.empty((n, max(int(topk), 1)), np.int32); scores = np.empty((n, max(int(topk), 1)), np.float64)
        if allow is not None or candidates is not None:
            f, _keep = _item_filter(allow, candidates, self.d2, n)
            _chk(lib().pcr_recommend_filtered(self._h, n, None if users is None else users.ctypes.data, int(topk),
                                              PCR_REC_EXCLUDE_TRAIN if exclude_train else 0, C.byref(f), items.ctypes.data, scores.ctypes.data))
            return items, scores
        _chk(lib().pcr_recommend(self._h, n, None if users is None else users.ctypes.data, int(topk),
                                 PCR_REC_EXCLUDE_TRAIN if exclude_train else 0, items.ctypes.data, scores.ctypes.data))
        return items, scores

    def recommend_diverse(self, topk=10, pool=None, theta=0.5, users=None, exclude_train=True):
        """MMR re-ranked top-K lists from the device factors (pcr_recommend_diverse), in the solver's storage type; arguments
        and result as recommend_diverse(), users as Solver.recommend()."""
        topk, pool, theta = _rerank_args(topk, pool, theta)
        if users is not None:
            users = np.ascontiguousarray(users, np.int32)
        n = self.n_users if users is None else users.shape[0]
        items = np.empty((n, topk), np.int32); scores = np.empty((n, topk), np.float64)
        _chk(lib().pcr_recommend_diverse(self._h, n, None if users is None else users.ctypes.data, topk, pool, theta,
                                         PCR_REC_EXCLUDE_TRAIN if exclude_train else 0, items.ctypes.data, scores.ctypes.data))
        return items, scores

    def recommend_capped(self, topk=10, groups=None, cap=1, pool=None, users=None, exclude_train=True, allow=None):
        """Group-capped top-K lists from the device factors (pcr_recommend_capped), in the solver's storage type; arguments and
        result as recommend_capped(), users as Solver.recommend().  The stats are this rank's own counts."""
        topk, pool, groups, cap = _cap_args(topk, pool, groups, cap, None if self is None else self.d2)
        if users is not None:
            users = np.ascontiguousarray(users, np.int32)
        n = self.n_users if users is None else users.shape[0]
        f, _keep = _item_filter(allow, None, self.d2, n)
        items = np.empty((n, topk), np.int32); scores = np.empty((n, topk), np.float64); status = np.empty(n, np.uint8)
        st = CapStats()
        _chk(lib().pcr_recommend_capped(self._h, n, None if users is None else users.ctypes.data, topk, pool, groups.ctypes.data, cap,
                                        PCR_REC_EXCLUDE_TRAIN if exclude_train else 0, None if allow is None else C.byref(f),
                                        items.ctypes.data, scores.ctypes.data, status.ctypes.data, C.byref(st)))
        return _cap_result(items, scores, status, st)

    def evaluate_topn(self, cutoffs=(10,), threshold=-np.inf, exclude_train=True, per_user=False, allow=None, candidates=None):
        """Full-catalogue top-N evaluation of this shard's users against the solver's test ratings (pcr_evaluate_topn); the
        result as evaluate_topn(), per_user rows for the shard's users.  N ranks with a communicator: the totals of all ranks
        (every rank must call); local-only shards: their own partials.  allow / candidates as evaluate_topn(), one candidate
        row per user of the shard (pcr_evaluate_topn_filtered)."""
        if allow is not None or candidates is not None:
            f, _keep = _item_filter(allow, candidates, self.d2, self.n_users)
            return _topn_call(cutoffs, per_user, self.n_users, lambda nc, cp, sp, pp: lib().pcr_evaluate_topn_filtered(
                self._h, nc, cp, float(threshold), PCR_REC_EXCLUDE_TRAIN if exclude_train else 0, C.byref(f), sp, pp))
        return _topn_call(cutoffs, per_user, self.n_users, lambda nc, cp, sp, pp: lib().pcr_evaluate_topn(
            self._h, nc, cp, float(threshold), PCR_REC_EXCLUDE_TRAIN if exclude_train else 0, sp, pp))

    def evaluate_ranks(self, threshold=-np.inf, exclude_train=True, per_user=False, ranks=False, allow=None, candidates=None):
        """Exact full-catalogue rank metrics of this shard's users against the solver's test ratings (pcr_evaluate_ranks); the
        result as evaluate_ranks(), per_user rows and ranks for the shard's users / test ratings.  N ranks with a communicator:
        the totals of all ranks (every rank must call); local-only shards: their own partials.  allow / candidates as
        evaluate_ranks(), one candidate row per user of the shard (pcr_evaluate_ranks_filtered)."""
        tnnz = 0
        if ranks:
            tidx = self.ds.csr(1)[0]                     # (a shard's own data set starts at its first user)
            lo = 0 if tidx.shape[0] - 1 == self.n_users else self.first_user
            tnnz = int(tidx[lo + self.n_users] - tidx[lo])
        if allow is not None or candidates is not None:
            f, _keep = _item_filter(allow, candidates, self.d2, self.n_users)
            return _ranks_call(per_user, ranks, self.n_users, tnnz, lambda sp, pp, rp: lib().pcr_evaluate_ranks_filtered(
                self._h, float(threshold), PCR_REC_EXCLUDE_TRAIN if exclude_train else 0, C.byref(f), sp, pp, rp))
        return _ranks_call(per_user, ranks, self.n_users, tnnz, lambda sp, pp, rp: lib().pcr_evaluate_ranks(
            self._h, float(threshold), PCR_REC_EXCLUDE_TRAIN if exclude_train else 0, sp, pp, rp))

    def evaluate_diversity(self, cutoffs=(10,), users=None, exclude_train=True, per_user=False, exposure=False):
        """Beyond-accuracy metrics of this shard's users from the device factors (pcr_evaluate_diversity); the result as
        evaluate_diversity(), popularity from the solver's training ratings.  users: GLOBAL 0-based ids of this rank's shard
        (None: all of them, in order).  N ranks with a communicator: the totals of all ranks (every rank must call);
        local-only shards: their own partials."""
        if users is not None:
            users = np.ascontiguousarray(users, np.int32)
        n = self.n_users if users is None else users.shape[0]
        return _diversity_call(cutoffs, per_user, exposure, n, self.d2, lambda nc, cp, sp, pp, ep: lib().pcr_evaluate_diversity(
            self._h, n, None if users is None else users.ctypes.data, nc, cp, PCR_REC_EXCLUDE_TRAIN if exclude_train else 0, sp, pp, ep))

    def evaluate_rerank(self, thetas, pool=None, cutoffs=(10,), users=None, threshold=-np.inf, exclude_train=True, per_user=False,
                        exposure=False):
        """The accuracy / diversity trade-off of Solver.recommend_diverse() from the device factors (pcr_evaluate_rerank): one
        scoring sweep, then per theta the re-ranked lists and their metrics against the solver's test ratings; the result as
        evaluate_rerank().  users: GLOBAL 0-based ids of this rank's shard (None: all of them, in order).  N ranks with a
        communicator: the totals of all ranks (every rank must call); local-only shards: their own partials."""
        th, pool, cuts = _tradeoff_args(thetas, pool, cutoffs, threshold)
        if users is not None:
            users = np.ascontiguousarray(users, np.int32)
        n = self.n_users if users is None else users.shape[0]
        out = _lists_result(int(th.shape[0]), n, self.d2, cuts, True, per_user, exposure, lambda tp, dp, pt, pd, ep: lib().pcr_evaluate_rerank(
            self._h, n, None if users is None else users.ctypes.data, int(th.shape[0]), th.ctypes.data, pool, int(cuts.shape[0]),
            cuts.ctypes.data, float(threshold), PCR_REC_EXCLUDE_TRAIN if exclude_train else 0, tp, dp, pt, pd, ep))
        for r, v in zip(out, th):
            r["theta"] = float(v)
        return out

    def fold_in(self, ratings, U0=None, steps=10, per_user=False):
        """Factors for users this solver was not trained on, against its device V (pcr_fold_in), in its storage type and with its
        parameters (lambda, solver type, stepsize, CG knobs); arguments and result as fold_in().  Local to the rank; the
        solver's factors and training state are not touched."""
        index, item, val = _foldin_ratings(ratings)
        n = index.shape[0] - 1
        return _foldin_call(n, self.k, U0, per_user, lambda u0, uo, sp, pp: lib().pcr_fold_in(
            self._h, n, index.ctypes.data, item.ctypes.data, val.ctypes.data, u0, int(steps), uo, sp, pp))

    def fold_in_items(self, new_items, train=None, V0=None, steps=10, per_item=False):
        """Rows of V for items this solver was not trained on, against its device U and V (pcr_fold_in_items), in its storage type
        and with its parameters; new_items and the result as fold_in_items().  train (None: the Dataset the solver was created
        from) supplies the rating values and must be that data set.  Needs every user on the rank (a shard solver: PcrError);
        nothing of the solver is written."""
        ds = self.ds if train is None else train
        if not isinstance(ds, Dataset):
            raise ValueError("train must be a Dataset (the one the solver was created from)")
        index, user, val = _foldin_ratings(new_items)
        n = index.shape[0] - 1
        return _itemfold_call(n, self.k, V0, per_item, lambda v0, vo, sp, pp: lib().pcr_fold_in_items(
            self._h, ds._h, n, index.ctypes.data, user.ctypes.data, val.ctypes.data, v0, int(steps), vo, sp, pp))

    def explain(self, lists, users=None, train=None, top=5, weights=None, per_pair=False, per_user=False):
        """Why each listed item scores as it does for this solver's users, from its device U and V (pcr_explain), in its storage
        type and with its lambda and solver type; lists, top and the result as explain().  users: GLOBAL 0-based ids (None: all
        of them, in order).  train (None: the Dataset the solver was created from) supplies the rows and their rating values and
        must be that data set.  weights [n]: None takes the weights last given to set_user_weights(w) for these users -- remembered here
        in Python, the library's entry never reads the solver's own; weights given with local=True (fewer than d1 of them) are NOT
        taken, nor is anything after set_user_weights(None): the call then runs unweighted, so pass weights explicitly there.  Needs
        every user on the rank (a shard solver: PcrError); nothing of the solver is written."""
        ds = self.ds if train is None else train
        if not isinstance(ds, Dataset):
            raise ValueError("train must be a Dataset (the one the solver was created from)")
        if users is not None:
            users = np.ascontiguousarray(users, np.int32)
        n = self.n_users if users is None else users.shape[0]
        mine = getattr(self, "user_weights", None)
        if weights is None and mine is not None and mine.shape[0] == self.d1:
            weights = mine if users is None else mine[users]
        return _explain_call(n, lists, top, weights, per_pair, per_user, lambda wp, L, lp, E, ip, cp, pp, up, sp: lib().pcr_explain(
            self._h, ds._h, n, None if users is None else users.ctypes.data, wp, L, lp, E, ip, cp, pp, up, sp))

    def explain_ridge(self, lists, users=None, train=None, top=5, weighted=True, nonneg=False, per_pair=False, per_user=False):
        """Why each listed item scores as it does for this solver's users as squared-loss rows, from its device U and V
        (pcr_explain_ridge), in its storage type and with its lambda; CCDR1 is the intended solver, any single-rank one runs;
        lists, top, weighted, nonneg and the result as explain_ridge().  users: GLOBAL 0-based ids (None: all of them, in order).
        train (None: the Dataset the solver was created from) supplies the rows and their rating values and must be that data
        set.  nonneg is the caller's: -N is not read from the solver.  A multi-rank or shard solver: PcrError; nothing of the solver
        is written."""
        ds = self.ds if train is None else train
        if not isinstance(ds, Dataset):
            raise ValueError("train must be a Dataset (the one the solver was created from)")
        if users is not None:
            users = np.ascontiguousarray(users, np.int32)
        n = self.n_users if users is None else users.shape[0]
        return _explain_ridge_call(n, lists, top, per_pair, per_user, lambda L, lp, E, ip, cp, pp, up, sp: lib().pcr_explain_ridge(
            self._h, ds._h, n, None if users is None else users.ctypes.data, 1 if weighted else 0, 1 if nonneg else 0, L, lp, E, ip, cp, pp, up,
            sp))

    def fold_in_ridge(self, ratings, weighted=True, per_user=False):
        """Squared-loss factors for users this solver was not trained on, against its device V (pcr_fold_in_ridge), in its storage
        type and with its lambda; any solver type, CCDR1 included; arguments and result as fold_in_ridge().  Local to the rank;
        nothing of the solver is written."""
        index, item, val = _foldin_ratings(ratings)
        n = index.shape[0] - 1
        return _ridge_call(n, self.k, per_user, lambda uo, sp, pp: lib().pcr_fold_in_ridge(
            self._h, 1 if weighted else 0, n, index.ctypes.data, item.ctypes.data, val.ctypes.data, uo, sp, pp))

    def fold_in_conf(self, ratings, weights=None, alpha=None, weighted=True, per_user=False):
        """fold_in_conf() for users this solver was not trained on, against its device V (pcr_fold_in_conf), in its storage type
        and with its lambda; alpha=None takes the solver's own setting (set_implicit; counter "ccd_implicit"; 0 on a solver type
        that has none).  Local to the rank; nothing of the solver is written."""
        index, item, val = _foldin_ratings(ratings)
        n = index.shape[0] - 1
        w = _conf_weights(weights, item.shape[0])
        if alpha is None:                                   # (the counter exists on a CCDR1 solver only: no setting, no alpha)
            v = C.c_double()
            a = v.value if lib().pcr_solver_counter(self._h, b"ccd_implicit", v) == 0 else 0.0
        else:
            a = float(alpha)
        return _ridge_call(n, self.k, per_user, lambda uo, sp, pp: lib().pcr_fold_in_conf(
            self._h, 1 if weighted else 0, a, n, index.ctypes.data, item.ctypes.data, val.ctypes.data, None if w is None else w.ctypes.data, uo,
            sp, pp))

    def fold_in_nnls(self, ratings, weighted=True, per_user=False):
        """Non-negative factors for users this solver was not trained on, against its device V (pcr_fold_in_nnls), in its storage
        type and with its lambda; any solver type; arguments and result as fold_in_nnls().  Local to the rank; nothing of the
        solver is written."""
        index, item, val = _foldin_ratings(ratings)
        n = index.shape[0] - 1
        return _nnls_call(n, self.k, per_user, lambda uo, sp, pp: lib().pcr_fold_in_nnls(
            self._h, 1 if weighted else 0, n, index.ctypes.data, item.ctypes.data, val.ctypes.data, uo, sp, pp))

    def sync(self):
        _chk(lib().pcr_solver_sync(self._h))

    def close(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.pcr_solver_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()
