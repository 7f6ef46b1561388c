"""primalcr_amd -- MI355X-native PrimalCR / PrimalCR++ collaborative-ranking solver.

The product is ``primalcr_amd/lib/libprimalcr.so`` (hand-written HIP for gfx950 behind the C
ABI of ``include/primalcr.h``) plus the drop-in CLIs ``primalcr_amd/bin/omp-pmf-train`` and
``omp-pmf-predict`` and ``omp-pmf-recommend``.  This package is the thin host-side mirror of the reference's solver
interface (``pmf.h``) over that C ABI via ctypes -- used by tests and ``bench.py``.

There is no CPU fallback: importing works without a GPU (host-side helpers such as the loader
and ``initial`` are usable), but every training entry point raises ``PcrError`` when the HIP
library or a GPU is missing.
"""
from .api import (PCR_F32, PCR_F64, PCR_REC_EXCLUDE_TRAIN, PCR_RECOMMEND_MAX_K, PCR_TOPN_MAX_CUTOFFS, PCR_RERANK_MAX_THETAS, PCR_SOLVER_CCDR1, PCR_SOLVER_PCR, PCR_SOLVER_PCRPP, CcdParameter, Dataset, Parameter, PcrError,
                  Solver, comm_unique_id, initial, initial_col, initial_rows, lib, lib_path, use_library, model_load, model_save, partition_users, predict, recommend, recommend_diverse, recommend_capped, CapStats, PCR_CAP_EXACT, PCR_CAP_POOL_EXHAUSTED, evaluate_topn, TOPN_FIELDS, evaluate_ranks, RankStats, RANK_FIELDS, sample_negatives, PCR_RANK_STAGE, PCR_CAND_RANK_STAGE, evaluate_diversity, DiversityStats, DIVERSITY_FIELDS, exposure_stats, evaluate_lists, evaluate_rerank, tune, tuned, fold_in, recommend_new_users, foldin_boundaries, FoldinStats, PCR_FOLDIN_FIELDS,
                  PCR_FOLDIN_CONVERGED, PCR_FOLDIN_STEP_CAP, PCR_FOLDIN_STALLED, PCR_FOLDIN_WAVE_MAX, PCR_FOLDIN_LDS_MAX,
                  fold_in_ridge, recommend_new_users_ridge, ridge_boundaries, ridge_form, fold_in_conf, recommend_new_users_conf, conf_boundaries, conf_block, conf_form, RidgeStats, PCR_RIDGE_FIELDS, PCR_RIDGE_DUAL, PCR_RIDGE_PRIMAL, PCR_RIDGE_CG, PCR_RIDGE_OK, PCR_RIDGE_SINGULAR, PCR_RIDGE_CG_CAP, PCR_RIDGE_WAVE_MAX, PCR_RIDGE_DIRECT_MAX,
                  fold_in_nnls, recommend_new_users_nnls, nnls_form, NnlsStats, PCR_NNLS_FIELDS, PCR_NNLS_DIRECT, PCR_NNLS_CG, PCR_NNLS_OK, PCR_NNLS_SINGULAR, PCR_NNLS_CAP, PCR_NNLS_PIVOT_CAP,
                  fold_in_items, itemfold_boundaries, rater_scores_boundaries, ItemfoldStats, PCR_ITEMFOLD_FIELDS, PCR_ITEMFOLD_WAVE_MAX, PCR_ITEMFOLD_LDS_MAX,
                  PCR_ITEMFOLD_SCORES_WAVE_MAX, user_weights, match_weights, rating_weights_popularity, PCR_WEIGHT_UNIFORM, PCR_WEIGHT_PAIRS, PCR_WEIGHT_RATINGS,
                  explain, explain_boundaries, ExplainStats, PCR_EXPLAIN_MAX_L, PCR_EXPLAIN_MAX_E, PCR_EXPLAIN_PAIR_FIELDS, PCR_EXPLAIN_USER_FIELDS, EXPLAIN_TILE, EXPLAIN_CHUNK,
                  explain_ridge, explain_ridge_boundaries, ExplainRidgeStats, PCR_EXPLAIN_RIDGE_USER_FIELDS)

__all__ = ["PCR_F32", "PCR_F64", "PCR_REC_EXCLUDE_TRAIN", "PCR_RECOMMEND_MAX_K", "PCR_TOPN_MAX_CUTOFFS", "PCR_RERANK_MAX_THETAS", "PCR_SOLVER_CCDR1", "PCR_SOLVER_PCR", "PCR_SOLVER_PCRPP", "CcdParameter", "Dataset", "Parameter", "PcrError",
           "Solver", "comm_unique_id", "initial", "initial_col", "initial_rows", "lib", "lib_path", "use_library", "model_load", "model_save", "partition_users", "predict", "recommend", "recommend_diverse", "recommend_capped", "CapStats", "PCR_CAP_EXACT", "PCR_CAP_POOL_EXHAUSTED", "evaluate_topn", "TOPN_FIELDS", "evaluate_ranks", "RankStats", "RANK_FIELDS", "sample_negatives", "PCR_RANK_STAGE", "PCR_CAND_RANK_STAGE", "evaluate_diversity", "DiversityStats", "DIVERSITY_FIELDS", "exposure_stats", "evaluate_lists", "evaluate_rerank", "tune", "tuned", "fold_in", "recommend_new_users", "foldin_boundaries", "FoldinStats",
           "PCR_FOLDIN_FIELDS", "PCR_FOLDIN_CONVERGED", "PCR_FOLDIN_STEP_CAP", "PCR_FOLDIN_STALLED", "PCR_FOLDIN_WAVE_MAX", "PCR_FOLDIN_LDS_MAX",
           "fold_in_ridge", "recommend_new_users_ridge", "ridge_boundaries", "ridge_form", "fold_in_conf", "recommend_new_users_conf", "conf_boundaries", "conf_block", "conf_form", "RidgeStats", "PCR_RIDGE_FIELDS", "PCR_RIDGE_DUAL", "PCR_RIDGE_PRIMAL", "PCR_RIDGE_CG", "PCR_RIDGE_OK", "PCR_RIDGE_SINGULAR", "PCR_RIDGE_CG_CAP", "PCR_RIDGE_WAVE_MAX", "PCR_RIDGE_DIRECT_MAX",
           "fold_in_nnls", "recommend_new_users_nnls", "nnls_form", "NnlsStats", "PCR_NNLS_FIELDS", "PCR_NNLS_DIRECT", "PCR_NNLS_CG", "PCR_NNLS_OK", "PCR_NNLS_SINGULAR", "PCR_NNLS_CAP", "PCR_NNLS_PIVOT_CAP",
           "fold_in_items", "itemfold_boundaries", "rater_scores_boundaries", "ItemfoldStats", "PCR_ITEMFOLD_FIELDS", "PCR_ITEMFOLD_WAVE_MAX", "PCR_ITEMFOLD_LDS_MAX",
           "PCR_ITEMFOLD_SCORES_WAVE_MAX", "user_weights", "match_weights", "rating_weights_popularity", "PCR_WEIGHT_UNIFORM", "PCR_WEIGHT_PAIRS", "PCR_WEIGHT_RATINGS",
           "explain", "explain_boundaries", "ExplainStats", "PCR_EXPLAIN_MAX_L", "PCR_EXPLAIN_MAX_E", "PCR_EXPLAIN_PAIR_FIELDS", "PCR_EXPLAIN_USER_FIELDS", "EXPLAIN_TILE", "EXPLAIN_CHUNK",
           "explain_ridge", "explain_ridge_boundaries", "ExplainRidgeStats", "PCR_EXPLAIN_RIDGE_USER_FIELDS"]
