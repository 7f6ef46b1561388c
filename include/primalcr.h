/*
 * primalcr.h -- C ABI of libprimalcr.so: the MI355X-native PrimalCR / PrimalCR++
 * training path (hand-written HIP for gfx950) behind the reference's solver API.
 *
 * Drop-in boundary.  The reference's solver entry points are
 *     extern "C" void pcrpp(smat_t&, mat_t&, mat_t&, testset_t&, parameter&)  pmf.h:52-56, pcrpp.cpp:841
 *     extern "C" void pcr  (smat_t&, mat_t&, mat_t&, testset_t&, parameter&)  pmf.h:54,    pcr.cpp:616
 * whose arguments are C++ references to STL classes -- not a real C ABI.  This
 * header is the genuine C ABI for the same step: plain pointers and sizes, caller
 * owned factor buffers (fp64, row-major, exactly the reference's mat_t payload),
 * integer status codes (the reference returns void and never reports errors).
 * INTEGRATION.md shows the few lines a maintainer adds to pmf-train.cpp to call it.
 *
 * Every entry point cites the reference interface it replaces (file:line relative
 * to the reference checkout).
 *
 * Conventions
 *   - all matrices row-major, 0-based; U is d1 x k (users), V is d2 x k (items)
 *   - ratings: user-major CSR in the reference's SparseMat layout (util.h:390-413):
 *     index[d1+1], item[nnz] (SparseMat::rows), val[nnz] (SparseMat::vals)
 *   - return value 0 = success, negative = error; pcr_last_error() has the text
 *   - functions marked [host] never touch the GPU
 *   - functions marked [device] need a gfx950 GPU and FAIL (never fall back to a
 *     CPU path) when none is usable
 */
#ifndef PRIMALCR_H
#define PRIMALCR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCR_OK               0
#define PCR_ERR_ARG         -1
#define PCR_ERR_IO          -2
#define PCR_ERR_NOMEM       -3
#define PCR_ERR_DEVICE      -4   /* no usable GPU / HIP runtime error            */
#define PCR_ERR_COMM        -5   /* RCCL error                                    */
#define PCR_ERR_STATE       -6   /* call order (e.g. obtain_g before comp_m)      */
#define PCR_ERR_UNSUPPORTED -7

/* solver ids: pmf.h:6  enum {CCDR1, PCR, PCRPP} */
#define PCR_SOLVER_CCDR1  0   /* CCD++ rank-one, squared loss (ccd-r1.cpp:97-212); one rank only */
#define PCR_SOLVER_PCR    1
#define PCR_SOLVER_PCRPP  2

/* storage type of U, V, m and the CG vectors on the device.  Prefix sums,
 * objectives, dot products and sweep coefficients are ALWAYS accumulated in fp64. */
#define PCR_F32 0
#define PCR_F64 1

/* mirrors class parameter (pmf.h:9-49) for the fields the PCR/PCR++ path reads,
 * plus device-side extensions */
typedef struct pcr_params {
    int solver_type;   /* pmf.h:32  default PCRPP (2)                             */
    int k;             /* pmf.h:33  rank, default 10                              */
    int threads;       /* pmf.h:38  default 4; host threads of loaders only       */
    int maxiter;       /* pmf.h:35  default 10                                    */
    double lambda;     /* pmf.h:37  default 5000                                  */
    int do_predict;    /* pmf.h:45  default 1                                     */
    int verbose;       /* pmf.h:46                                                */
    double stepsize;   /* pmf.h:28  default 1.0 (reset every step, pcrpp.cpp:877) */
    int ndcg_k;        /* pmf.h:29  default 10                                    */
    /* extensions */
    int precision;     /* PCR_F32 (default) | PCR_F64                             */
    int device;        /* HIP device ordinal, default 0                           */
    /* truncated-Newton knobs: the reference hard-codes 10 CG iterations at
     * most and a residual tolerance of 1 % of ||g|| for both half steps
     * (pcrpp.cpp:340,344 / :632,636).  cg_max_iter = r with a small cg_tol turns the U
     * step into an exact Newton step.  The defaults reproduce the reference.   */
    int cg_max_iter;   /* default 10                                              */
    double cg_tol;     /* default 0.01                                            */
} pcr_params;

/* pmf.h:27-48 parameter::parameter() */
void pcr_params_default(pcr_params *p);                                   /* [host] */

/* The CCDR1 solver's own settings (pcr_params stays as it is, so that callers built against it keep working).
 * Set with pcr_solver_set_ccd_params before pcr_train / pcr_iterate. */
typedef struct pcr_ccd_params {
    int maxinneriter;  /* pmf.h:36  default 5     (-T)                                  */
    double eps;        /* pmf.h:39  default 1e-3  (-e): inner stop at fundec < fundec_max * eps */
    int do_nmf;        /* pmf.h:47  default 0     (-N): non-negative factors            */
} pcr_ccd_params;
void pcr_ccd_params_default(pcr_ccd_params *p);                           /* [host] */

const char *pcr_last_error(void);                                         /* [host] */
const char *pcr_version(void);                                            /* [host] */

/* ------------------------------------------------------------------------- */
/* host data path                                                            */
/* ------------------------------------------------------------------------- */

/* util.cpp:80-93 initial(): N(0,1) from a default-seeded std::default_random_engine
 * through std::normal_distribution<double>; a fresh engine per call.  The same values bit for bit; above 4 M of them
 * produced by several host threads (the engine is an LCG: a range of tries starts at a state that modular
 * exponentiation gives directly, and libstdc++'s polar method takes exactly four draws per try). */
int pcr_initial(double *X, int64_t n, int64_t k);                         /* [host] */
/* rows [row0, row0 + nrows) of what pcr_initial(., n, k) would produce, into X (nrows x k): where an output lands
 * depends on how many tries were accepted before it, so the tries before row0 are still evaluated (in parallel, without
 * their sqrt / log) -- for a rank that holds only its own users' rows of a large U. */
int pcr_initial_rows(double *X, int64_t n, int64_t k, int64_t row0, int64_t nrows);   /* [host] */
/* util.cpp:95-101 initial_col(): the row-major n x k values 0.1 * drand48(), drawn in order, bit for bit, from glibc's
 * UNSEEDED drand48 stream (state 0: a = 0x5DEECE66D, c = 0xB, m = 2^48, value = X / 2^48).  The generator is the library's own
 * (libc's drand48 state is global to the process and is never touched); above 2 M values several host threads draw ranges
 * that start at states computed by jump-ahead. */
int pcr_initial_col(double *X, int64_t n, int64_t k);                     /* [host] */

typedef struct pcr_dataset pcr_dataset;   /* training CSR + test CSR, host memory */

/* util.cpp:6-25 load() + util.h:197-271 smat_t::load + util.h:360-371
 * testset_t::load + util.cpp:219-274 convert(): reads <dir>/meta and the rating
 * files it names. */
int pcr_dataset_load(const char *dir, pcr_dataset **out);                 /* [host] */
/* the same with `threads` host threads (the CLI passes -n; 0 = up to 16) for every stage: the rating files are mapped, cut at
 * line boundaries and parsed piece by piece into the CSR's own arrays; a file ordered by (user, item) -- what the reference's
 * data sets are -- needs no further data movement, any other order goes through a bucketed counting sort; the test set's
 * rows follow the reference's scan (util.cpp:250-274: the row of the largest user id seen so far, ending at the first
 * id that is no user). */
int pcr_dataset_load_mt(const char *dir, int threads, pcr_dataset **out); /* [host] */
/* Binary side-car of a loaded data set (the reference re-parses the text with fgets/sscanf and re-sorts on
 * every run, util.cpp:6-25, util.h:197-271).  pcr_dataset_save_cache writes the converted CSRs (train + test) to
 * `path`; pcr_dataset_load_cache reads them back (PCR_ERR_IO if the file is missing, truncated or of another version).
 * pcr_dataset_load_cached(dir, threads, cache, out) = load_cache(cache) when the cache exists AND records the same
 * size and modification time of <dir>/meta and of the rating files it names, else load_mt(dir) followed by a best-effort
 * save_cache(cache) (an unwritable cache path is not an error).  The text formats stay the only input format. */
int pcr_dataset_save_cache(const pcr_dataset *ds, const char *path);      /* [host] */
int pcr_dataset_load_cache(const char *path, pcr_dataset **out);          /* [host] */
int pcr_dataset_load_cached(const char *dir, int threads, const char *cache, pcr_dataset **out);   /* [host] */
/* same conversion from in-memory 0-based triplets (train in any order; test must
 * be user-sorted, util.cpp:259-261).  tnnz may be 0. */
int pcr_dataset_from_triplets(int64_t d1, int64_t d2,
                              int64_t nnz, const int32_t *user, const int32_t *item, const double *val,
                              int64_t tnnz, const int32_t *tuser, const int32_t *titem, const double *tval,
                              pcr_dataset **out);                          /* [host] */
/* the same from arrays already in the reference's SparseMat layout (util.h:390-413, what convert() leaves,
 * util.cpp:219-274): index[d1+1], item[nnz] ascending inside a user, val[nnz]; the test CSR (tindex may be NULL) is
 * taken as given. */
int pcr_dataset_from_csr(int64_t d1, int64_t d2, const int64_t *index, const int32_t *item, const double *val,
                         const int64_t *tindex, const int32_t *titem, const double *tval, pcr_dataset **out);   /* [host] */
void pcr_dataset_free(pcr_dataset *ds);                                    /* [host] */
/* sizes: d1, d2, nnz (train), tnnz (test entries assigned by convert()) */
int pcr_dataset_dims(const pcr_dataset *ds, int64_t *d1, int64_t *d2, int64_t *nnz, int64_t *tnnz);
/* copy the CSR out (which: 0 = train, 1 = test); any pointer may be NULL */
int pcr_dataset_csr(const pcr_dataset *ds, int which, int64_t *index, int64_t *item, double *val);
/* #Omega = #{(i,j,k): R_ij > R_ik} after the solver's level bucketing (lround for
 * PrimalCR++, pcrpp.cpp:41; raw doubles for PrimalCR, pcr.cpp:23) */
int64_t pcr_dataset_count_pairs(const pcr_dataset *ds, int solver_type);   /* [host] */
/* The same count user by user: pairs[u] = |Omega_u|, the number of terms of user u's loss (pcrpp.cpp:361-412 / pcr.cpp:5-44 sum
 * over exactly these pairs), d1 entries, under the same level bucketing; their sum is pcr_dataset_count_pairs. */
int pcr_dataset_user_pairs(const pcr_dataset *ds, int solver_type, int64_t *pairs /* d1 */);   /* [host] */

/* Per-user loss weights c_u > 0 for PrimalCR / PrimalCR++ (no counterpart in the reference, whose objective pcrpp.cpp:361-412
 * gives every user weight one): min sum_u c_u L_u + lambda/2 (|U|^2 + |V|^2).  pcr_user_weights fills w (d1 entries) by scheme:
 *   PCR_WEIGHT_UNIFORM   w_u = 1
 *   PCR_WEIGHT_PAIRS     w_u = (|Omega| / #{u: |Omega_u| > 0}) / |Omega_u|, and 1 where |Omega_u| = 0: every user with a
 *                        comparable pair carries the same mass, sum_u w_u |Omega_u| = |Omega|
 *   PCR_WEIGHT_RATINGS   w_u = (nnz / #{u: n_u > 0}) / n_u, and 1 where n_u = 0: sum_u w_u n_u = nnz
 * Both normalising schemes keep the total mass of the unweighted problem, so lambda keeps its scale.  Another scheme, or
 * solver_type 0, is PCR_ERR_ARG. */
#define PCR_WEIGHT_UNIFORM 0
#define PCR_WEIGHT_PAIRS   1
#define PCR_WEIGHT_RATINGS 2
int pcr_user_weights(const pcr_dataset *ds, int solver_type, int scheme, double *w /* d1 */);   /* [host] */

/* Per-rating weights for pcr_solver_set_rating_weights (CCDR1), in the order of pcr_dataset_csr(ds, 0, ...).
 * pcr_dataset_match_weights puts n (user, item, weight) triplets, ids 0-based as pcr_dataset_from_triplets takes them and in any
 * order, into that order: w_csr[z] = the weight of the triplet that names training rating z.  PCR_ERR_ARG, the first offender
 * named in pcr_last_error: a triplet that is no training rating, a training rating named twice, one left without a weight.
 * pcr_rating_weights_popularity: w_z = (n_max / n_item(z))^gamma, n_item = the item's training ratings, n_max the largest of them
 * -- the inverse of a power-law propensity; gamma = 0 gives ones; a gamma that is not finite is PCR_ERR_ARG.  Not normalised: a
 * common factor on all weights leaves the minimiser where it is. */
int pcr_dataset_match_weights(const pcr_dataset *ds, int64_t n, const int32_t *user, const int32_t *item, const double *w,
                              double *w_csr /* nnz */);                    /* [host] */
int pcr_rating_weights_popularity(const pcr_dataset *ds, double gamma, double *w_csr /* nnz */);   /* [host] */

/* A rating file on its own (omp-pmf-predict's test file: pmf-predict.cpp:52-55 reads "user item rating" triples until fscanf
 * fails, no meta file).  count: the file's non-blank lines.  read: at most n entries by `threads` host threads (0 = up to 16),
 * ids 0-based, val may be NULL; the input ends at the first malformed entry: *n_read entries stand before it (the reference's
 * loop never ends on such a line: it tests `!= EOF`, pmf-predict.cpp:56). */
int pcr_rating_file_count(const char *path, int64_t *n);                   /* [host] */
int pcr_rating_file_read(const char *path, int threads, int64_t n, int32_t *user, int32_t *item, double *val,
                         int64_t *n_read);                                 /* [host] */

/* pmf-train.cpp:297-310 + util.cpp:30-51 save_mat_t(U^T,false); save_mat_t(V^T,false):
 * "long d1, long k, d1*k doubles, long d2, long k, d2*k doubles" */
int pcr_model_save(const char *path, const double *U, int64_t d1, const double *V, int64_t d2, int64_t k);
/* pmf-predict.cpp:49-50 + util.cpp:56-79 load_mat_t(fp,true) twice.
 * Call with U = V = NULL to query the sizes first. */
int pcr_model_load(const char *path, int64_t *d1, int64_t *d2, int64_t *k, double *U, double *V);

/* nnz-balanced contiguous user ranges for nparts GPUs: bounds[nparts+1] */
int pcr_partition_users(const int64_t *index, int64_t d1, int nparts, int64_t *bounds);   /* [host] */

/* ------------------------------------------------------------------------- */
/* device solver                                                             */
/* ------------------------------------------------------------------------- */

/* Launch knobs.  The reference has none (its only scheduling choice is `#pragma omp ... schedule(dynamic,500)`,
 * pcrpp.cpp:825); the device solver chooses its launch configuration from the shape of the shard, and these
 * key/value pairs override single choices -- for the parity tests (every configuration must give the same trajectory)
 * and for A/B measurements.  The table belongs to the CALLING THREAD: pcr_solver_create snapshots the creating thread's
 * pairs into the solver (nothing is read later, nothing is shared between threads, so solver handles stay re-entrant);
 * value NULL removes a key; unknown keys are PCR_ERR_ARG.
 * No environment variable is read anywhere on the product path.  (The ROCm runtime has one prerequisite of its own for
 * pcr_solver_comm_init_p2p / RCCL across processes on hosts whose driver only supports dmabuf IPC:
 * HSA_ENABLE_IPC_MODE_LEGACY=0 in the environment of every rank.)
 *   ustep_mode      1 = latency form of k_ustep for every long class, 2 = throughput form (default: by user count, more than CUs/4
 *                   users = throughput)
 *   cluster_k       4 (default) or 1: workgroups per clustered long user;  cluster_users: how many users get clusters
 *   ubins           "cap:block:resident,..." length classes of the U step below 1024 ratings
 *   ustep_newton    1 = EXACT Newton U step: users of at most 1024 ratings (ranks up to 112) get their direction from the
 *                   explicit r x r Hessian, built on the matrix cores and factored by Cholesky (k_unewton); every other user's CG runs
 *                   to convergence.  Leaves the reference's truncated-CG trajectory on purpose; default 0
 *   vblock_users    n > 0 = BLOCKED-USER V step: the n users with the most ratings (those that rate at least a sixteenth
 *                   of the items) take their share of every Hessian-vector product's two rating-parallel products as dense GEMMs on
 *                   the matrix cores (k_vblock_b, k_vblock_hp) and stay out of the sparse kernels' plan; same results to summation-
 *                   order rounding; default 0
 *   ustep_gram      dual (Gram-matrix on MFMA) U step for users with at most that many ratings (<= 128; default 0 = off)
 *   spmm_tiles, spmm_chunk, sddmm_csc   tiling of the rating-parallel kernels (user tiles per XCD group, ratings per lane group, the
 *                   CG's SDDMM over the tile-major CSC: chosen from the shard's shape)
 *   window_cache    0 = sweeps search their hinge windows instead of caching them (the form users with more than 9 levels take)
 *   prepare_merged  1 / 0 = both LDS classes of k_prepare in one launch, or one launch per length class side by side
 *                   (default: merged below 4 M ratings per shard)
 *   resort_window   half-width D of the nearly-sorted fast path of the per-user sorts (k_prepare, k_ustep's line search): a user
 *                   whose ratings moved by at most D positions since the previous sorted state is re-sorted by windowed rank
 *                   counting (verified; else the full bitonic network); default 8, 0 = always the full network, at most 64
 *   lanes           concurrent streams for length classes (1 = none: the layout a process ends up with when every side stream
 *                   shares a hardware queue with the solver's);  pipeline: 0 = host round trip after every U step
 *   allreduce_chunks N = item ranges of the SpMM whose all-reduces overlap the next range's SpMM (default 1: one all-reduce per
 *                   vector on the solver's stream; opt-in, meant for vectors of 16 MB and more -- about one range per 4 MB)
 *   p2p_ll          peer-to-peer communicator: vectors of at most this many MB (and the objective's scalars) take the device-driven
 *                   exchange (one kernel per rank, flags inside the 8-byte words, no host barrier); larger ones the host-synchronised
 *                   reduce-scatter / all-gather; default 16, 0 = host-synchronised always.  (If any rank cannot allocate
 *                   fine-grained device memory for its exchange boxes, EVERY rank takes the host-synchronised path.)
 *   p2p_timeout_ms  wall-clock deadline of one device-driven exchange (default 20000): a rank whose peers do not arrive in time
 *                   reports PCR_ERR_COMM, poisons its answers (no rank consumes a made-up sum) and raises the job's error flag
 *   p2p_queue_budget   hardware queues one device maps at once for all its processes (default 24: gfx950 under the kernel driver's
 *                   scheduler; 8 of them are left to processes this job cannot see).  Only matters when several ranks SHARE a device
 *                   (a rehearsal): every rank publishes the queues its process holds; past the budget kernels of different processes
 *                   no longer run side by side (0.5 us -> 7-11 ms per dependent hand-off, tools/ubench/queue_budget_probe.hip), so
 *                   the device-driven exchange is switched off for the whole job (host-synchronised exchange, one line on stderr)
 *   recommend_select  0 = pcr_recommend's kernel without its streaming selection (the GEMM and the sweep alone; the lists come back
 *                   empty): tools/exp_recommend.py times the selection's share with it; default 1
 *   ranks_batch_users  test hook: at most this many counted users per batch of pcr_evaluate_ranks (rounded up to whole
 *                   workgroups of 64; 0 = the natural batch, which holds a million users and more); read at every call
 *   sample_threads  test hook: the host threads of pcr_sample_negatives (0 = the set-up default); its rows do not depend on it;
 *                   read at every call
 *   rerank_lds      the form of pcr_recommend_diverse's selection kernel: 0 (default) = the streaming form (the pool's rows of V
 *                   are re-read from L2 every round; the faster one at every shape measured), 1 = the LDS form (the pool's rows
 *                   staged once per user) whenever one wave's image fits a workgroup's 160 KiB; both forms implement the same
 *                   contract, the tests hold them to each other; read at every call
 *   ridge_form      "cg" = pcr_fold_in_ridge / pcr_fold_in_ridge_model take the CG form for every user (the A/B arm of the direct
 *                   forms, and a test hook); "auto" (default) = the form rule; read when the call's plan is made.  pcr_fold_in_conf /
 *                   pcr_fold_in_conf_model read the same knob
 *   nnls_form      "cg" = pcr_fold_in_nnls / pcr_fold_in_nnls_model take the CG form at every rank (the A/B arm of the direct
 *                   form, and a test hook); "auto" (default) = the form rule; read when the call's plan is made
 *   itemfold_table_bytes  test hook: the cap of pcr_fold_in_items' rater table (scores + levels) in bytes; a call whose unique
 *                   raters exceed it runs in batches of items (results do not depend on it); default 2^30; read at every call
 *   count_rows      1 = the U-step kernels count the rows of V they gather (pcr_solver_counter; a diagnostic that
 *                   costs the short-user classes 10-20 %, so off by default)
 *   debug           1 = print launch decisions to stderr
 *   plan_key64      test hook: 1 = the set-up's (tile, item) sort keys in 64 bits -- the form an item side beyond 2^32 / tiles takes anyway
 *   win16, ustep_win_lds   test hooks: 0 = the forms shards with very long users take anyway -- 32-bit window-cache entries (a user
 *                   of 65536 ratings or more), k_ustep reading the window cache from global memory (a class whose LDS is full) --
 *                   forced on small data so that the fuzz tests cover them
 * (Knobs of experiments that are closed -- stream placements, serial classes, cluster hand-off without fences, window-cache
 * widths and copies, sweep load depth, clusters of two -- are gone with their code paths; NOTES.md keeps the numbers.)
 *   fault_cluster_member   test hook: one member of every workgroup cluster leaves early (the launch must report
 *                   PCR_ERR_DEVICE through the bounded hand-off wait instead of hanging)
 *   fault_p2p_skip  test hook: this rank never launches its n-th device-driven exchange (its peers must time out, poison their
 *                   answers and fail with PCR_ERR_COMM; nobody may hang or consume garbage)
 *   fault_p2p_coarse   test hook: this rank behaves as if fine-grained memory were unavailable (all ranks must fall back to the
 *                   host-synchronised exchange together)
 * Stream layout: the solver creates its stream and a high-priority stream, then creates side streams one by one and MEASURES
 * (a few ms each at creation; pcr_tune("debug") prints it) which of them share a hardware queue with the solver's stream (they are
 * not used as lanes; it stops at three lanes, usually after four or five streams) and which lanes share its command-processor PIPE (queues on one pipe share workgroup dispatch and throttle each
 * other): such a lane is placed last, and a high-priority stream that landed on the solver's pipe is replaced.  So the layout
 * no longer depends on how many streams the host application created before the solver; results never did. */
int pcr_tune(const char *key, const char *value);                          /* [host] */

typedef struct pcr_solver pcr_solver;

/* Optional: initialise the HIP runtime for `device` and load the library's code object now (otherwise the first
 * pcr_solver_create does both, ~0.2-0.3 s).  Thread-safe with the [host] functions: a host application can call it on a
 * second thread while it parses its input (omp-pmf-train does: the reference has nothing to overlap, pmf-train.cpp:247-266). */
int pcr_device_warmup(int device);                                         /* [device] */

/* Upload this rank's user shard (rank 0 of 1 = everything) and allocate the
 * device state.  Replaces convert(R), convert(T) at pcrpp.cpp:850-851. */
int pcr_solver_create(const pcr_dataset *ds, const pcr_params *p, int rank, int nranks,
                      pcr_solver **out);                                   /* [device] */
/* The same for a job whose rating set no single process holds (configs[4]: 700 M ratings over 8 GPUs): `ds_local` contains
 * ONLY this rank's users, renumbered from 0 -- users [first_user, first_user + d1(ds_local)) of a job with d1_total users; the
 * host application chooses the ranges (pcr_partition_users on the per-user counts) so that they tile [0, d1_total) in rank
 * order.  Its test set must be empty on every rank or on none.  Replaces the same call sites as pcr_solver_create;
 * the user loop being sharded is pcrpp.cpp:825-833. */
int pcr_solver_create_shard(const pcr_dataset *ds_local, const pcr_params *p, int rank, int nranks,
                            int64_t first_user, int64_t d1_total, pcr_solver **out);   /* [device] */
void pcr_solver_destroy(pcr_solver *s);

/* RCCL bootstrap for nranks > 1 (one process per GPU): rank 0 obtains an id
 * (128 bytes), the host application broadcasts it, every rank calls comm_init. */
int pcr_comm_unique_id(void *id128);                                       /* [device] */
int pcr_solver_comm_init(pcr_solver *s, const void *id128);                /* [device] */
/* The direct peer-to-peer alternative for the ranks of ONE node (replaces the omp atomics of
 * pcrpp.cpp:240-243, :323-327 across GPUs): every rank exposes an exchange buffer through HIP IPC; an all-reduce is a
 * reduce-scatter + all-gather that sums in rank order (every rank obtains the same bits).  Vectors up to 16 MB and the
 * scalars are exchanged by ONE kernel per rank with the flags inside the exchanged 8-byte words (no host involvement);
 * larger vectors through reads of the peers' buffers over xGMI between host barriers over a POSIX shared-memory control
 * block, whose error flag also releases the peers of a rank that failed.  Every rank calls this with the same name ("/something", shm_open);
 * no id exchange is needed.  Use either this or pcr_solver_comm_init. */
int pcr_solver_comm_init_p2p(pcr_solver *s, const char *shm_name);         /* [device] */
/* ranks the solver's communicator reports (ncclCommCount / the p2p control block); 1 without a communicator */
int pcr_solver_comm_nranks(pcr_solver *s);
/* diagnostic counters, cumulative since the solver was created:
 *   "ustep_row_gathers"  rows of V the U steps gathered (per user: 1 for the gradient + 2 per CG iteration + 1 per
 *                        line-search try, times its rating count; all ranks; counted only under pcr_tune("count_rows")) --
 *                        the U step's gather rate = this x k x sizeof(storage type) / its wall time */
/*   "ustep_row_gathers/<slot>"  the same count for ONE length class of the U step on THIS rank (<slot> = its profile slot
 *                        name, e.g. "ustep/256.512"; pcr_solver_ustep_classes lists them, comma-separated) */
int pcr_solver_counter(pcr_solver *s, const char *name, double *value);
int pcr_solver_ustep_classes(pcr_solver *s, char *buf, int64_t cap);
/* Where pcr_solver_create's wall time went -- the unit the reference spends in convert() (util.cpp:219-274) and this library in
 * uploads, the set-up built on the device and the stream probes: phase i (0, 1, ...) of the creation, in order; *name points
 * into the solver (valid until it is destroyed).  PCR_ERR_ARG past the last phase.  omp-pmf-train --timing prints the list. */
int pcr_solver_setup_phase(const pcr_solver *s, int i, const char **name, double *ms);
/* Shard-local mode for a solver created with nranks > 1 and no communicator: every collective
 * becomes a no-op, so pcr_obtain_g / pcr_compute_Ha / pcr_objective return THIS SHARD'S PARTIAL
 * (rank 0 carries the lambda term).  Lets a host application combine shards itself, and lets one
 * process verify the sharding of N ranks on a single GPU. */
int pcr_solver_set_local_only(pcr_solver *s, int on);

/* CCDR1 (solver type 0) only: maxinneriter, eps, do_nmf, taken as given like the reference's -T / -e / -N (maxinneriter <= 0: no
 * inner iteration, every rank only re-forms its residual); PCR_ERR_STATE on another solver */
int pcr_solver_set_ccd_params(pcr_solver *s, const pcr_ccd_params *p);

/* first local user and number of local users of this rank's shard */
int pcr_solver_shard(const pcr_solver *s, int64_t *first_user, int64_t *n_users, int64_t *nnz_local);

/* factors: host fp64 <-> device.  U is the FULL d1 x k matrix; each rank reads /
 * writes only its own rows [first_user, first_user+n_users). V is d2 x k. */
int pcr_solver_set_factors(pcr_solver *s, const double *U, const double *V);
int pcr_solver_get_factors(pcr_solver *s, double *U, double *V);
/* the same with U_local = this rank's n_users x k rows only (what a rank created by pcr_solver_create_shard holds) */
int pcr_solver_set_factors_local(pcr_solver *s, const double *U_local, const double *V);
int pcr_solver_get_factors_local(pcr_solver *s, double *U_local, double *V);

/* Per-user loss weights (PrimalCR / PrimalCR++; the reference's update_V_new pcrpp.cpp:415-444 and update_u_new :779-815 are
 * the case c_u = 1): w holds one weight per user of the JOB (d1 entries; each rank reads only its own users'), w_local this
 * rank's n_users entries only, as with set_factors / set_factors_local.  NULL returns to the unweighted problem.  Every weight
 * read must be finite and > 0, else PCR_ERR_ARG and the solver keeps what it had.  From then on pcr_objective, pcr_obtain_g,
 * pcr_compute_Ha, pcr_solve_delta, pcr_update_V, pcr_update_U, pcr_train, pcr_iterate and pcr_iter_stats.obj are those of
 *     min sum_u c_u L_u(U, V) + lambda/2 (|U|^2 + |V|^2):
 * the V side's gradient and Hessian-vector products are sum_u c_u (user u's share), and user u's Newton step is the
 * unweighted step with lambda / c_u -- so a trained user's row is what pcr_fold_in returns for that user with lambda / c_u.
 * pcr_evaluate and the serving entries never see the loss and are unchanged.  May be called at any point between entry
 * points: the solver synchronises, drops the objective sums a pipelined loop had queued and continues from the weighted
 * objective at the current factors (the sorted state of the last pcr_comp_m stays valid).
 * PCR_ERR_UNSUPPORTED (reason in pcr_last_error): a CCDR1 solver; a solver created under pcr_tune "ustep_newton",
 * "ustep_gram" or "vblock_users", whose optional kernels do not carry weights. */
int pcr_solver_set_user_weights(pcr_solver *s, const double *w /* d1 of the job */);        /* [device] */
int pcr_solver_set_user_weights_local(pcr_solver *s, const double *w_local /* n_users */);  /* [device] */

/* Per-rating confidence weights for CCDR1 (solver type 0; the reference's ccd-r1.cpp is the case c = 1): one weight c_z, finite
 * and > 0, per training rating z = (i, j), in the order of pcr_dataset_csr(ds, 0, ...).  From then on pcr_train / pcr_iterate solve
 *     min sum_z c_z (r_z - u_i . v_j)^2 + lambda (sum_i W_i |u_i|^2 + sum_j W_j |v_j|^2),   W = the sum of c_z over the row's ratings
 * (the reference regularises by lambda times the rating count, ccd-r1.cpp:151,157: W is that count with weights, so a rating of
 * weight 2 is the rating present twice and a common factor on all weights leaves the minimiser where it is).  The rank-one update of
 * a non-empty column is g = sum c x r, h = lambda W + sum c x^2, new = g / h, fundec = h (old - new)^2; the printed loss / obj / reg
 * and pcr_iter_stats.obj are the weighted ones; the stopping rule, the test rmse and pcr_evaluate do not see weights.  The weights
 * are stored in the solver's precision (rounded as the ratings are): each must be finite and > 0 as given and as stored, else
 * PCR_ERR_ARG and the solver keeps what it had.  NULL returns to the unweighted kernels.  Like pcr_solver_set_factors the call ends
 * a running training (the next pcr_train / pcr_iterate begins from the current U); weights survive pcr_solver_set_factors and
 * pcr_solver_set_ccd_params.  pcr_solver_counter "ccd_rating_weights" is 1 while weights are set.  Fold-in, explanations and the
 * model file do not carry weights.  PCR_ERR_UNSUPPORTED on a PrimalCR / PrimalCR++ solver (those take pcr_solver_set_user_weights). */
int pcr_solver_set_rating_weights(pcr_solver *s, const double *w /* nnz, in the order of pcr_dataset_csr(ds, 0, ...) */);   /* [device] */

/* Implicit feedback for CCDR1 (solver type 0): alpha > 0 is the weight of every UNRATED cell, whose target is 0.  From then on
 * pcr_train / pcr_iterate solve
 *     min sum_{z in Omega} c_z (r_z - u_i . v_j)^2 + alpha sum_{(i,j) not in Omega} (u_i . v_j)^2 + lambda (sum_i W_i |u_i|^2 + sum_j W_j |v_j|^2),
 *     W_i = (the sum of c_z over user i's ratings) + alpha (d2 - n_i),  W_j likewise with d1 - n_j
 * (c_z = the weights of pcr_solver_set_rating_weights, 1 when none are set): an unrated cell is exactly a rating 0 of weight alpha, in
 * the regulariser too.  With rating weights 1 + a * count and alpha = 1 this is the confidence model of Hu, Koren and Volinsky.
 * The d1 x d2 cells are never formed; while alpha is set the solver keeps two fp64 predictions per training rating on
 * the device (16 bytes per rating, beside the two residual copies).  Every column is updated, an empty user or item too: training
 * starts from V = 0, so its minimiser is exactly 0, and its step from the initial value counts in the stopping rule.  The printed loss / obj / reg and pcr_iter_stats.obj are those of this objective; the stopping rule, the test rmse,
 * pcr_evaluate and "ccd_residual_mismatch" are unchanged.  alpha must be finite and >= 0; it is stored in the solver's precision
 * and, when > 0 as given, must be > 0 as stored; else PCR_ERR_ARG and the solver keeps what it had.  0 returns to the explicit
 * kernels.  Like pcr_solver_set_factors the call ends a running training; the setting survives pcr_solver_set_factors,
 * pcr_solver_set_ccd_params and pcr_solver_set_rating_weights (and they survive it).  pcr_solver_counter "ccd_implicit" is the
 * stored alpha (0 when off).  Fold-in, explanations and the model file do not carry alpha.  PCR_ERR_UNSUPPORTED on a PrimalCR /
 * PrimalCR++ solver. */
int pcr_solver_set_implicit(pcr_solver *s, double alpha);   /* [device] */

/* pcrpp.cpp:17-35 comp_m_new (pcr.cpp:47 comp_m): m = u_i . v_j for every rating,
 * from the current device U, V; also builds the per-user (level, m)-sorted state
 * the sweeps use.  m_out (local nnz, CSR order) may be NULL. */
int pcr_comp_m(pcr_solver *s, double *m_out);
/* pcrpp.cpp:361-412 objective_new (pcr.cpp:5 objective) at the state of the last
 * pcr_comp_m: all-rank sum incl. lambda/2 (|U|^2 + |V|^2). */
int pcr_objective(pcr_solver *s, double *obj);
/* pcrpp.cpp:140-249 obtain_g_new (pcr.cpp:102 obtain_g): g (d2 x k) */
int pcr_obtain_g(pcr_solver *s, double *g);
/* pcrpp.cpp:252-332 compute_Ha_new (pcr.cpp:167 compute_Ha): a, Ha are d2 x k */
int pcr_compute_Ha(pcr_solver *s, const double *a, double *Ha);
/* pcrpp.cpp:335-358 solve_delta_new (pcr.cpp:248): CG on H delta = g */
int pcr_solve_delta(pcr_solver *s, const double *g, double *delta, int *cg_iters);
/* pcrpp.cpp:415-444 update_V_new (pcr.cpp:279): one Newton step on V.
 * info[0] = CG iterations, info[1] = line-search evaluations, info[2] = accepted */
int pcr_update_V(pcr_solver *s, double *now_obj, int *info);
/* pcrpp.cpp:818-838 update_U_new (pcr.cpp:587): one Newton step per user.
 * info[0] = total CG iterations, info[1] = total line-search evaluations */
int pcr_update_U(pcr_solver *s, double *now_obj, int64_t *info);
/* util.cpp:434-542 compute_pairwise_error_ndcg on the train (which=0) or test
 * (which=1) ratings with the current device factors */
int pcr_evaluate(pcr_solver *s, int which, int ndcg_k, double *pairwise_err, double *ndcg);

/* what the reference prints per iteration (pcrpp.cpp:859-890) */
typedef struct pcr_iter_stats {
    double obj;
    double train_err, train_ndcg, test_err, test_ndcg;
    double seconds;                 /* cumulative, clock scope of pcrpp.cpp:874-881 */
    int64_t cg_v, ls_v, cg_u, ls_u; /* executed inner-iteration counts              */
} pcr_iter_stats;
/* On a CCDR1 solver one record per OUTER iteration (record 0 of pcr_train is zero): obj = the objective after its last rank,
 * test_err / test_ndcg = the last evaluation (pcr_train with do_predict), seconds = device time of the CCDR1 kernels since the
 * start of training, carried across pcr_iterate calls (the reference's Htime + Wtime + Rtime, ccd-r1.cpp:200), cg_v = inner iterations executed, cg_u = ranks executed
 * (both cumulative since the start of training); train_err, train_ndcg, ls_v, ls_u = 0. */

typedef void (*pcr_log_fn)(void *ctx, const char *line);

/* CCDR1 (solver type 0): pcr_train = ccd-r1.cpp:97-212 ccdr1() from the current U, with V zeroed as the reference does; one
 * line per rank (ccd-r1.cpp:196-206) when verbose, evaluated on the test set when do_predict.  pcr_iterate runs n more outer
 * iterations without evaluation (starting a training run first if none is under way; pcr_solver_set_factors ends it).  The
 * PrimalCR-only entry points (comp_m, objective, obtain_g, compute_Ha, solve_delta, update_V, update_U) return PCR_ERR_STATE.
 * pcr_solver_counter(s, "ccd_residual_mismatch") counts the positions where the residual's user-major and item-major copies
 * differ (always 0).  Profile slots: ccd/init, ccd/begin, ccd/vsweep, ccd/usweep, ccd/decide, ccd/resid, ccd/final. */
/* pcrpp.cpp:841-901 pcrpp() / pcr.cpp:616-704 pcr(): the whole training loop
 * from the current device factors.  Emits the reference's log lines through
 * `log` (NULL = stdout, rank 0 only; a callback is invoked on EVERY rank of a multi-rank job with the
 * same lines).  hist may be NULL, else holds maxiter+1 records. */
int pcr_train(pcr_solver *s, pcr_log_fn log, void *log_ctx, pcr_iter_stats *hist);
/* The body of that loop (pcrpp.cpp:869-895: update_V_new, update_U_new, no evaluation) n times from the current state,
 * with one host round trip per iteration: the U step is queued without waiting for it and its objective is read back
 * together with the next iteration's line search.  out (may be NULL) receives n records: obj, seconds (cumulative
 * device time of the loop), inner-iteration counts.  pcr_train uses it when do_predict == 0 and log == NULL. */
int pcr_iterate(pcr_solver *s, int n, pcr_iter_stats *out);

/* pmf-predict.cpp:56-64: pred[z] = U[user[z]] . V[item[z]] for n (0-based) pairs */
int pcr_predict(const double *U, int64_t d1, const double *V, int64_t d2, int64_t k,
                int64_t n, const int32_t *user, const int32_t *item, double *pred,
                int device);                                               /* [device] */

/* ------------------------------------------------------------------------- */
/* top-K recommendation (no reference counterpart: pmf-predict.cpp scores     */
/* known pairs only)                                                          */
/* ------------------------------------------------------------------------- */
/* For each requested user u: the K items j of highest score s(u, j) = U[u] . V[j], computed on the device.
 *   Order       descending computed score; equal computed scores by ascending item id (in every code path, merges of
 *               partial lists included), so results are exactly checkable.
 *   Exclusion   with exclusion on, every item of u's TRAINING CSR row is left out (duplicated (user, item) pairs allowed);
 *               test ratings are never excluded.
 *   Padding     a user with fewer than K eligible items: the row ends with item -1 and score -INFINITY.
 *   Precision   fp64 factors are scored in fp64; fp32 factors with f32 inputs and f32 accumulation (the score is a fixed,
 *               k-ordered chain of f32 fmas).  Scores come back as double.
 *   Determinism a score depends on (u, j) alone -- not on the other users of the call, their order or the launch grid; two
 *               identical calls return bitwise-identical output.
 *   Limit       1 <= K <= PCR_RECOMMEND_MAX_K; anything out of range is PCR_ERR_ARG before any device work.
 * Output: items[n * K] (0-based ids, int32) and scores[n * K], row i for users[i].
 * PCR_RECOMMEND_MAX_K = 1024: the selection stages a user's list in LDS next to 16 x 64 candidate slots per wave (24 KB per
 * wave in fp64 at K = 1024, four waves per workgroup); larger K would leave one workgroup per CU. */
#define PCR_RECOMMEND_MAX_K 1024
#define PCR_REC_EXCLUDE_TRAIN 1   /* pcr_recommend flag: leave out the solver's own training ratings */

/* Standalone, like pcr_predict: U (d1 x k) and V (d2 x k) are host fp64 factors in model-file layout.  index[d1 + 1] / item
 * (the training CSR, 0-based, index[0] = 0, monotone) give the exclusion; index = item = NULL: none.  users[n] are 0-based
 * ids (NULL: users 0 .. n-1, n <= d1).  dtype PCR_F32 rounds the factors to f32 and scores them in f32, PCR_F64 scores in
 * fp64.  Arguments (ids inside the model, CSR shape) are checked on the host before any device is looked for. */
int pcr_recommend_model(const double *U, int64_t d1, const double *V, int64_t d2, int64_t k,
                        const int64_t *index, const int32_t *item,
                        int64_t n, const int32_t *users, int topk, int dtype,
                        int32_t *items, double *scores, int device);       /* [device] */
/* The same on a live solver's device factors (any solver type), in its storage type, on its stream; training state is not
 * touched (training that continues afterwards gives bitwise the same factors).  users[n] are GLOBAL 0-based ids of this
 * rank's shard (NULL: all of the shard's users in order, n = its n_users); a user outside the shard is PCR_ERR_ARG.
 * flags: PCR_REC_EXCLUDE_TRAIN.  Profile slots: recommend/score, recommend/merge. */
int pcr_recommend(pcr_solver *s, int64_t n, const int32_t *users, int topk, int flags,
                  int32_t *items, double *scores);                         /* [device] */

/* ------------------------------------------------------------------------- */
/* filtered recommendation: top-K among allowed items and candidate lists     */
/* ------------------------------------------------------------------------- */
/* The recommendation above restricted to a catalogue-wide eligibility set (in stock, a category, a market), to a candidate
 * list per user (re-ranking a retrieval stage; "one held-out item against 99 sampled negatives" is candidates followed by
 * pcr_evaluate_lists_model), or to both.  Everything the block above promises holds unchanged: the order rule, the padding
 * with (-1, -INFINITY), the precision, the determinism, 1 <= K <= PCR_RECOMMEND_MAX_K.  In addition:
 *   Eligible items   of user u: all items, or the items of u's candidate row when cand_ptr is given; of those, the items
 *                    whose allow[j] is nonzero (allow NULL: all of them) that are not in u's training row when exclusion is
 *                    on.  The filters intersect.  The list is the K best eligible items.
 *   Same bits        s(u, j) is bit for bit the score pcr_recommend / pcr_recommend_model computes for the pair, in fp32 and
 *                    in fp64: a filtered list is exactly the unfiltered full ranking with the ineligible entries struck
 *                    out.  It does not depend on the other users of the call, their order, the launch grid or the order of
 *                    the ids inside a candidate row.
 *   Limits           K and d2 as pcr_recommend; a candidate row may have any length.
 *   Errors           f == NULL, or a filter with allow and cand_ptr both NULL, is PCR_ERR_ARG (pcr_recommend is the entry
 *                    without a filter; the message says so).  Also PCR_ERR_ARG: cand_ptr[0] != 0 or cand_ptr not monotone,
 *                    cand_ptr without cand_item, a candidate id outside [0, d2), an id twice in one row; the message names
 *                    the entry and the user.  All are found on the host before any device is looked for.
 * Profile slots (of the solver entry): recommend/score + recommend/merge for an allow set alone, recommend/candidates (one
 * launch per user batch, the whole selection) whenever candidate lists are given. */
typedef struct pcr_item_filter {
    const uint8_t *allow;      /* [d2], nonzero = eligible for every user; NULL: every item */
    const int64_t *cand_ptr;   /* [n + 1], cand_ptr[0] = 0, monotone; row i belongs to users[i]; NULL: no candidate lists */
    const int32_t *cand_item;  /* 0-based item ids, any order within a row, no id twice in a row */
} pcr_item_filter;
/* Standalone: every argument but f as pcr_recommend_model. */
int pcr_recommend_filtered_model(const double *U, int64_t d1, const double *V, int64_t d2, int64_t k,
                                 const int64_t *index, const int32_t *item,
                                 int64_t n, const int32_t *users, int topk, int dtype, const pcr_item_filter *f,
                                 int32_t *items, double *scores, int device);        /* [device] */
/* On a live solver of any type, as pcr_recommend: users[n] are GLOBAL ids of this rank's shard (NULL: all of them, n = its
 * n_users, and cand_ptr has n_users + 1 entries); nothing is exchanged and the training state is not touched. */
int pcr_recommend_filtered(pcr_solver *s, int64_t n, const int32_t *users, int topk, int flags,
                           const pcr_item_filter *f, int32_t *items, double *scores); /* [device] */

/* ------------------------------------------------------------------------- */
/* full-catalogue top-N evaluation (no reference counterpart: util.cpp's       */
/* evaluator ranks a user's own test items among themselves)                  */
/* ------------------------------------------------------------------------- */
/* Every user with held-out ratings is scored against the whole catalogue, its top K = cutoffs[ncut - 1] list is selected and
 * the ranking metrics are reduced at each cutoff -- on the device; no list leaves it.  For a user u and a cutoff c:
 *   Relevant set R_u   the DISTINCT items j with a test rating (u, j, v), v >= threshold; an item that occurs several times in
 *                      u's test row counts once, with its largest rating.  threshold = -INFINITY: every test item; NaN is
 *                      PCR_ERR_ARG.  Exclusion does not change R_u: a test item that also sits in u's training row stays in
 *                      R_u with exclusion on, although it can never be listed.
 *   Graded gain        g(j) = pow(2.0, v_max) - 1.0 (the existing evaluator's gain).
 *   List L_u           exactly the list pcr_recommend / pcr_recommend_model returns with the same factors, dtype, K and
 *                      exclusion; padding (-1) is never relevant.
 *   Discount           d(i) = 1.0 / log2((double)(i + 2)) at position i = 0, 1, ...
 *   Counted users      |R_u| >= 1; the others are not scored at all.
 *   Per user           hits = |L_u[0..c) & R_u|, precision = hits / c, recall = hits / |R_u|,
 *                      ap = (sum over i < c, L_u[i] in R_u, of hits_{<=i} / (i + 1)) / min(c, |R_u|),
 *                      ndcg = sum_{i < c, L_u[i] in R_u} d(i) / sum_{i < min(c, |R_u|)} d(i),
 *                      ndcg_graded = sum_{i < c, L_u[i] in R_u} g(L_u[i]) d(i) / sum_{i < min(c, |R_u|)} g_desc[i] d(i)
 *                      (g_desc: R_u's gains in descending order), defined only when that ideal DCG is > 0.
 *   Summary per cutoff means over counted users (users), hit_rate = share of them with hits > 0, hits summed; ndcg_graded is
 *                      averaged over its own count (users_graded).  A denominator of 0 gives a mean of 0.
 *   Determinism        per-user values depend on (u, its list, its test row) alone; sums run in a fixed order over users in
 *                      ascending id; two identical calls are bitwise identical.
 * cutoffs[ncut]: 1 <= ncut <= PCR_TOPN_MAX_CUTOFFS, strictly ascending, each in [1, PCR_RECOMMEND_MAX_K].
 * per_user (optional, NULL: not written): [rows][ncut][6] = hits, precision, recall, ap, ndcg, ndcg_graded; uncounted users
 * (all six) and an undefined ndcg_graded are NaN. */
#define PCR_TOPN_MAX_CUTOFFS 8
typedef struct pcr_topn_stats {
    int     cutoff;
    int64_t users, users_graded, hits;
    double  precision, recall, hit_rate, map, ndcg, ndcg_graded;
} pcr_topn_stats;
/* Standalone: the factors, dtype and exclusion CSR as pcr_recommend_model; tindex[d1 + 1] / titem / tval the test CSR (0-based,
 * tindex[0] = 0, monotone, items in any order within a row).  rows = d1.  Arguments are checked on the host before any device
 * is looked for. */
int pcr_evaluate_topn_model(const double *U, int64_t d1, const double *V, int64_t d2, int64_t k,
                            const int64_t *index, const int32_t *item,
                            const int64_t *tindex, const int32_t *titem, const double *tval,
                            int ncut, const int *cutoffs, double threshold, int dtype,
                            pcr_topn_stats *stats, double *per_user, int device);     /* [device] */
/* On a live PCR, PCR++ or CCDR1 solver: its device factors and storage type, the test ratings it was created with, flags
 * PCR_REC_EXCLUDE_TRAIN as pcr_recommend; training state is not touched.  rows = the shard's n_users (per_user row i = user
 * first_user + i).  N ranks: stats are the totals over the communicator's ranks (every rank must call); local-only shards
 * (no communicator) return their own partials.  The relevance tables are built once per (threshold, cutoffs) and kept.
 * Profile slots: recommend/score, and recommend/metrics (the merge with the metrics fused in, and the reduction). */
int pcr_evaluate_topn(pcr_solver *s, int ncut, const int *cutoffs, double threshold, int flags,
                      pcr_topn_stats *stats, double *per_user);                        /* [device] */

/* ------------------------------------------------------------------------- */
/* exact full-catalogue rank metrics: AUC, MRR, mean (percentile) rank (no    */
/* reference counterpart)                                                     */
/* ------------------------------------------------------------------------- */
/* Where in the whole catalogue every held-out item lands -- what the top-N metrics cannot see below position K.  Every counted
 * user is scored against the whole catalogue on the device; no score leaves it.  For a user u:
 *   Score s(u, j)      exactly the score pcr_recommend computes for the same factors and dtype (bit for bit: the same fixed
 *                      k-ordered chain).
 *   Order              a BEFORE b when s(u, a) > s(u, b), or the scores are equal and a < b (the order of a recommended list).
 *   Relevant set R_u   as in the top-N evaluation: the distinct items with a test rating >= threshold; counted users are those
 *                      with |R_u| >= 1, in ascending order.  NaN threshold is PCR_ERR_ARG.
 *   Non-relevant N_u   all items, minus R_u, minus (with exclusion on) the items of u's training row.
 *   Rank               for j in R_u:  rank_u(j) = 1 + #{i in N_u : i before j} + #{j' in R_u : j' before j}   (an integer >= 1),
 *                      the position of j when N_u and R_u together are sorted by the order.  A held-out item is always a
 *                      candidate, also when it sits in u's training row too.  With train and test disjoint, rank_u(j) is the
 *                      position of j in an unbounded pcr_recommend list, and rank_u(j) <= K exactly when j is in the top-K list.
 *   Per user           first_rank = min_j rank_u(j);  rr = 1 / first_rank;  mean_rank = (sum_j rank_u(j)) / |R_u|;
 *                      auc = #{(j, i) : j in R_u, i in N_u, j before i} / (|R_u| |N_u|), NaN when N_u is empty;
 *                      mpr = (sum_j (rank_u(j) - 1)) / (|R_u| (|N_u| + |R_u| - 1)), the mean of the percentile ranks
 *                      (rank_u(j) - 1) / (|N_u| + |R_u| - 1); 0 when that denominator is 0.
 *                      Each is ONE fp64 division of two exactly represented integers (the sums and products are formed as
 *                      integers first), so a caller can reproduce every value exactly from ranks[].
 *   Summary            users, users_auc (users with a defined auc), relevant = sum |R_u|, and the means over the counted users
 *                      mrr, mean_rank, mpr and (over users_auc) auc.  A denominator of 0 gives a mean of 0.  No order
 *                      statistics over users (a median rank).
 *   Determinism        as the top-N evaluation: per-user values depend on (u, its rows) alone, the sums over users run in a
 *                      fixed order, two identical calls are bitwise identical.
 * per_user (optional, NULL: not written): [rows][PCR_RANK_FIELDS] = first_rank, rr, mean_rank, auc, mpr; uncounted users (all
 * five) and an undefined auc are NaN.
 * ranks (optional, NULL: not written): [tnnz] in the order of the test CSR: rank_u(titem[z]) for every test rating with
 * tval[z] >= threshold (every occurrence of a duplicated item gets the item's rank), 0 for the others. */
#define PCR_RANK_FIELDS 5
typedef struct pcr_rank_stats {
    int64_t users, users_auc, relevant;
    double  mrr, mean_rank, auc, mpr;
} pcr_rank_stats;
/* Standalone: arguments and host-side checks as pcr_evaluate_topn_model (rows = d1; tnnz = tindex[d1]); everything is checked
 * on the host before any device is looked for. */
int pcr_evaluate_ranks_model(const double *U, int64_t d1, const double *V, int64_t d2, int64_t k,
                             const int64_t *index, const int32_t *item,
                             const int64_t *tindex, const int32_t *titem, const double *tval,
                             double threshold, int dtype,
                             pcr_rank_stats *stats, double *per_user, int64_t *ranks, int device);   /* [device] */
/* On a live PCR, PCR++ or CCDR1 solver, as pcr_evaluate_topn: its device factors, storage type and stream, the test ratings
 * it was created with (ranks[]: the shard's test ratings in their CSR order), flags PCR_REC_EXCLUDE_TRAIN; training state is
 * not touched.  rows = the shard's n_users.  N ranks: stats are the totals over the communicator's ranks (every rank must
 * call); local-only shards return their own partials.  The relevance table is built once per threshold and kept.
 * Profile slots: ranks/relscore (the relevant items' scores and their sort), ranks/count (the counting sweep), ranks/finish. */
int pcr_evaluate_ranks(pcr_solver *s, double threshold, int flags,
                       pcr_rank_stats *stats, double *per_user, int64_t *ranks);                   /* [device] */

/* ------------------------------------------------------------------------- */
/* filtered evaluation: top-N and rank metrics within allowed items and       */
/* candidate rows (no reference counterpart)                                  */
/* ------------------------------------------------------------------------- */
/* The two evaluations above restricted by a pcr_item_filter f (unchanged; see "filtered recommendation"): sampled-candidate
 * evaluation (a user's held-out items against N sampled negatives: HR@10, NDCG@10, MRR, AUC over 1 + 99 candidates; the rows come
 * from pcr_sample_negatives below) and evaluation within a catalogue subset.  For a user u let F_u be the items of u's candidate
 * row (cand_ptr NULL: all items) whose allow[j] is nonzero (allow NULL: all of them); the filters intersect.
 *   Relevant set     R_u^f = R_u & F_u, R_u exactly as in the two blocks above (distinct items, rating >= threshold, the largest
 *                    rating kept).  The filter restricts the relevant set; training exclusion still does not.  Counted users are
 *                    those with |R_u^f| >= 1, in ascending order; the others are not scored.
 *   Top-N            L_u is exactly the list pcr_recommend_filtered(_model) returns for the same factors, dtype, K = the last
 *                    cutoff, exclusion and filter.  Every formula of pcr_evaluate_topn applies with R_u^f in place of R_u; a list
 *                    shorter than a cutoff is padded, padding is never relevant, precision = hits / c as before.
 *   Ranks            N_u^f = F_u minus R_u^f minus (with exclusion on) u's training row.  rank_u(j), first_rank, rr, mean_rank,
 *                    auc, mpr and the summary are those of pcr_evaluate_ranks with R_u^f and N_u^f.  A relevant item inside F_u
 *                    is always ranked, also when it sits in the training row (the existing rule).  Each quotient remains one fp64
 *                    division of exact integers.  ranks[] is 0 for test ratings below the threshold and for those whose item is
 *                    outside F_u.
 *   Scores, order    bit for bit those of pcr_recommend, through the same chain; ties by ascending id.
 *   Determinism      as the unfiltered entries: integer histogram adds commute, the sums over users run in a fixed order, two
 *                    identical calls are bitwise identical.
 *   Rows             model entries: cand_ptr has d1 + 1 entries, one row per user of the model; solver entries: n_users + 1, in
 *                    the shard's order.  Rows of uncounted users are checked and otherwise ignored.  A row may have any length
 *                    and |R_u^f| has no cap.
 *   Errors           f == NULL, or a filter with nothing in it, is PCR_ERR_ARG (the message points at pcr_evaluate_topn /
 *                    pcr_evaluate_ranks); the filter's own errors are those of pcr_recommend_filtered with this entry's name.
 *                    Everything is checked on the host before any device is looked for.
 * Every other argument and output is that of the unfiltered entry of the same name.  The solver entries reduce across the
 * communicator as the unfiltered ones do, leave the training state alone and do not touch the solver's cached unfiltered
 * relevance tables: filtered tables are built per call.
 * PCR_CAND_RANK_STAGE: with candidate rows the rank metrics stage a relevant row of up to this many entries in LDS and search
 * longer ones in global memory (the full sweep's own stage length is 32); results do not depend on it.
 * Profile slots (of the solver entries): top-N -- recommend/score + recommend/metrics for an allow set alone,
 * recommend/candidates_metrics (selection and metrics in one launch per user batch) + recommend/metrics (the reduction) with
 * candidate rows; ranks -- ranks/relscore, ranks/finish and ranks/count (allow alone) or ranks/candidates (candidate rows). */
#define PCR_CAND_RANK_STAGE 64
int pcr_evaluate_topn_filtered_model(const double *U, int64_t d1, const double *V, int64_t d2, int64_t k,
                                     const int64_t *index, const int32_t *item,
                                     const int64_t *tindex, const int32_t *titem, const double *tval,
                                     int ncut, const int *cutoffs, double threshold, int dtype, const pcr_item_filter *f,
                                     pcr_topn_stats *stats, double *per_user, int device);           /* [device] */
int pcr_evaluate_topn_filtered(pcr_solver *s, int ncut, const int *cutoffs, double threshold, int flags,
                               const pcr_item_filter *f, pcr_topn_stats *stats, double *per_user);   /* [device] */
int pcr_evaluate_ranks_filtered_model(const double *U, int64_t d1, const double *V, int64_t d2, int64_t k,
                                      const int64_t *index, const int32_t *item,
                                      const int64_t *tindex, const int32_t *titem, const double *tval,
                                      double threshold, int dtype, const pcr_item_filter *f,
                                      pcr_rank_stats *stats, double *per_user, int64_t *ranks, int device);   /* [device] */
int pcr_evaluate_ranks_filtered(pcr_solver *s, double threshold, int flags, const pcr_item_filter *f,
                                pcr_rank_stats *stats, double *per_user, int64_t *ranks);            /* [device] */

/* Candidate rows for the sampled protocol, on the host, deterministically: row u is the ascending union of sampled negatives
 * of user u and, with include_test, u's distinct test items.  With uint64 wrapping arithmetic
 *   mix(x):  x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;  x *= 0x94D049BB133111EB;  x ^= x >> 31
 *   key(u)  = mix(seed + 0x9E3779B97F4A7C15 * (u + 1))                         (u: the GLOBAL user id, first_user + row)
 *   draw t  = 0, 1, 2, ...:   j_t = mix(key(u) + 0x9E3779B97F4A7C15 * (t + 1)) % d2
 * The pool P_u is every item in neither u's training row (index / item, both NULL: no training rows) nor its test row -- every
 * test item is left out, whatever its rating.  m = min(n_neg, |P_u|).  m == |P_u|: the whole pool is taken.  Otherwise, if
 * 2 m <= |P_u|, the first m distinct draws that fall in P_u are taken; otherwise the first |P_u| - m such draws are LEFT OUT and
 * the rest of the pool is taken.  A user without test ratings gets an empty row.  The result does not depend on the number of
 * host threads or on how users are sharded.
 * rows: the users index / tindex describe (row i is user first_user + i).  Two calls: with cand_item NULL, cand_ptr[rows + 1]
 * receives the row pointer; with cand_item given (cand_ptr[rows] entries), both are written.  The sizing call draws nothing: a row's length is
 * min(n_neg, |P_u|) plus, with include_test, its distinct test items.  n_neg >= 0. */
int pcr_sample_negatives(int64_t rows, int64_t d2, const int64_t *index, const int32_t *item,
                         const int64_t *tindex, const int32_t *titem, int64_t first_user, int64_t n_neg, uint64_t seed,
                         int include_test, int64_t *cand_ptr, int32_t *cand_item);

/* ------------------------------------------------------------------------- */
/* beyond-accuracy top-N metrics: catalogue coverage, Gini index of item      */
/* exposure, novelty, intra-list diversity (no reference counterpart)         */
/* ------------------------------------------------------------------------- */
/* What the recommended lists look like, whatever the held-out ratings say: whether every user gets the same popular items and
 * how varied one user's list is.  The lists are selected, walked and reduced on the device; no list leaves it and no test set
 * is involved.  For every requested user u and cutoff c (cutoffs as in the top-N evaluation):
 *   List L_u           exactly the list pcr_recommend / pcr_recommend_model returns with the same factors, dtype and exclusion
 *                      and K = cutoffs[ncut - 1]; len(u, c) = the number of non-padding entries among the first c.
 *   Users              users[n] as in pcr_recommend (NULL: all users, in order); an id listed twice counts twice; every
 *                      requested user is counted, also with len = 0.
 *   Exposure           x_c[j] = the number of requested users with j in L_u[0..c): integers.
 *   From exposure      recs_c = sum_j x_c[j];  items_covered_c = #{j : x_c[j] > 0};  coverage_c = items_covered_c / d2 (one
 *                      fp64 division);  gini_c = (sum_{i = 1..d2} (2 i - d2 - 1) x_(i)) / (d2 recs_c) with x_(1) <= ... <= x_(d2)
 *                      the exposure sorted ascending: numerator and denominator are formed as 128-bit integers, each is
 *                      converted to double once, then one division; 0 when recs_c = 0.
 *   Popularity         pop[j] = the number of training-CSR entries with item j over all d1 users (duplicated pairs counted);
 *                      info[j] = log2((double)(d1 + 1) / (double)(pop[j] + 1)), built once on the host in fp64.
 *   Novelty            novelty(u, c) = (sum_{i < len} info[L_u[i]]) / len; NaN when len = 0.
 *   ILD                ild(u, c) = 1 - (sum_{a < b < len} cos(L_u[a], L_u[b])) / (len (len - 1) / 2), cos(a, b) = v^_a . v^_b,
 *                      v^_j = V[j] / |V[j]| in fp64 from the factors as the dtype stores them (f32-rounded for PCR_F32); a
 *                      row of norm 0 has v^_j = 0.  NaN when len < 2.  Always accumulated in fp64.
 *   Summary per cutoff users (n), users_ild (users with a defined ild), recs, items_covered, coverage, gini, novelty (mean over
 *                      the users with len >= 1), ild (mean over users_ild).  A denominator of 0 gives 0.
 *   Determinism        as the top-N evaluation: per-user values depend on (u, its list, V) alone; exposure is built with
 *                      integer adds, so it does not depend on their order; the sums over users run in a fixed order (the order
 *                      of users[]); two identical calls are bitwise identical.
 * per_user (optional, NULL: not written): [n][ncut][PCR_DIVERSITY_FIELDS] = len, novelty, ild; row i is for users[i].
 * exposure (optional, NULL: not written): int64 [ncut][d2] = x_c[j]. */
#define PCR_DIVERSITY_FIELDS 3
typedef struct pcr_diversity_stats {
    int     cutoff;
    int64_t users, users_ild, recs, items_covered;
    double  coverage, gini, novelty, ild;
} pcr_diversity_stats;
/* The closing arithmetic above for ONE cutoff's exposure row x[d2] (every entry >= 0): recs, items_covered, coverage, gini.
 * Both device entries use it; a caller who sums the exposure rows of local-only shards finishes the job with it.
 * PCR_ERR_ARG for a NULL row, d2 < 1, a negative entry or a row whose sum exceeds INT64_MAX (recs could not hold it). */
int pcr_exposure_stats(const int64_t *exposure, int64_t d2, int64_t *recs, int64_t *items_covered,
                       double *coverage, double *gini);                                             /* [host] */
/* Standalone: the factors, dtype, users[n] and host-side checks as pcr_recommend_model, the cutoff checks of
 * pcr_evaluate_topn_model; everything is checked on the host before any device is looked for.  index / item (the training
 * CSR) give both the exclusion and the popularity; NULL: no exclusion and pop = 0. */
int pcr_evaluate_diversity_model(const double *U, int64_t d1, const double *V, int64_t d2, int64_t k,
                                 const int64_t *index, const int32_t *item,
                                 int64_t n, const int32_t *users, int ncut, const int *cutoffs, int dtype,
                                 pcr_diversity_stats *stats, double *per_user, int64_t *exposure, int device);   /* [device] */
/* On a live PCR, PCR++ or CCDR1 solver: its device factors, storage type and stream; users[n] are GLOBAL ids of this rank's
 * shard as in pcr_recommend (NULL: all of the shard's users, n = its n_users); flags PCR_REC_EXCLUDE_TRAIN.  Popularity comes
 * from the solver's training ratings (whether or not they are excluded) with d1 = the job's total; training state is not
 * touched.  N ranks with a communicator: pop, exposure and the per-user sums are all-reduced and every rank returns the totals
 * (every rank must call; an RCCL communicator -- on a peer-to-peer communicator the entry is PCR_ERR_UNSUPPORTED, its fp64
 * exchange being a 64-double slot); a local-only shard returns its own partials, with pop from its own ratings.
 * Profile slots: recommend/score, and recommend/diversity (the row norms, the merge with the metrics fused in, the reductions). */
int pcr_evaluate_diversity(pcr_solver *s, int64_t n, const int32_t *users, int ncut, const int *cutoffs, int flags,
                           pcr_diversity_stats *stats, double *per_user, int64_t *exposure);                 /* [device] */

/* ------------------------------------------------------------------------- */
/* MMR diversity re-ranking of the top-K lists (no reference counterpart)      */
/* ------------------------------------------------------------------------- */
/* Greedy re-ranking by Maximal Marginal Relevance (Carbonell and Goldstein): topk items are taken one by one from a pool of the
 * user's `pool` best items, each time the one that is relevant and unlike what the list already holds.  Selected on the device;
 * only the re-ranked lists leave it.  For each requested user u, with 1 <= topk <= pool <= PCR_RECOMMEND_MAX_K and
 * 0 <= theta <= 1:
 *   Pool P_u           exactly the list pcr_recommend / pcr_recommend_model returns for the same factors, dtype, exclusion and
 *                      K = pool, without its padding: len entries (j_i, s_i), i = 0 .. len - 1, in the recommendation order,
 *                      the scores the same bits.
 *   Arithmetic         everything below is fp64; s_i is the computed score converted to double (exact, from f32 as well).
 *   Range              smin = min_i s_i, R = max_i s_i - smin, and R = 1 when that difference is 0.
 *   Cosine             cos(a, b) = v^_a . v^_b with v^_j = V[j] inv[j]; inv[j] = 1 / |V[j]| is taken from the factors as the dtype
 *                      stores them and is 0 for a zero row (the ILD's inv above, the same kernel).  Neither the order of the
 *                      k-term sum nor the place of the two factors inv[a] inv[b] (inside or outside the sum) is part of the
 *                      contract; the error is bounded as the ILD's, about (k + 2) 2^-52.
 *   Greedy rule        S starts empty.  At step t = 0 .. min(topk, len) - 1, for every pool entry i not yet taken:
 *                      m_i = (1 - theta) (s_i - smin) - (theta R) c_i with c_i = max_{a in S} cos(j_i, j_a), and c_i = 0 while S
 *                      is empty.  The entry with the largest m_i is taken; equal m_i go to the smaller pool position i.  (The
 *                      usual (1 - theta) rel - theta max sim with min-max-normalised relevance, multiplied through by R: the
 *                      order does not depend on the scale of the scores and no division is involved.)
 *   Output             items[n * topk] and scores[n * topk] in the order taken; the scores are the items' original s_i; a row
 *                      shorter than topk ends with (-1, -INFINITY).
 *   Consequences       theta = 0 returns bit for bit pcr_recommend's top-topk list, for any pool >= topk; the first entry is
 *                      always pool position 0; pool == topk returns a permutation of pcr_recommend's list.
 *   Determinism        a row depends on (u, its pool, V) alone -- not on the other users, the order of users[], batches or
 *                      splits; two identical calls are bitwise identical; no floating-point atomics.
 *   Errors             a NaN theta, theta outside [0, 1], topk < 1, pool < topk, pool > PCR_RECOMMEND_MAX_K and every argument
 *                      error of pcr_recommend_model are PCR_ERR_ARG, reported before any device is looked for; the message
 *                      names the entry. */
int pcr_recommend_diverse_model(const double *U, int64_t d1, const double *V, int64_t d2, int64_t k,
                                const int64_t *index, const int32_t *item, int64_t n, const int32_t *users,
                                int topk, int pool, double theta, int dtype,
                                int32_t *items, double *scores, int device);                          /* [device] */
/* On a live PCR, PCR++ or CCDR1 solver, as pcr_recommend: its device factors, storage type and stream; users[n] are GLOBAL ids
 * of this rank's shard (NULL: all of them); flags PCR_REC_EXCLUDE_TRAIN; training state is not touched.  Per user, nothing is
 * exchanged: it works on every communicator and on local-only shards.
 * Profile slots: recommend/score, and recommend/rerank (the row norms, the merge with the selection fused in). */
int pcr_recommend_diverse(pcr_solver *s, int64_t n, const int32_t *users, int topk, int pool, double theta,
                          int flags, int32_t *items, double *scores);                                 /* [device] */

/* ------------------------------------------------------------------------- */
/* group-capped top-K lists: at most `cap` items of one group (no reference    */
/* counterpart)                                                               */
/* ------------------------------------------------------------------------- */
/* "At most two items of the same artist / brand / seller / genre in a list": topk items are taken in recommendation order from
 * a pool of the user's `pool` best items, skipping an item once its group is full.  Selected on the device; only the capped lists
 * and one status byte per user leave it.  The library knows no item metadata: the caller brings group[d2], one int32 per item
 * -- any non-negative values are group ids, they need not be dense; a negative value means the item belongs to no group and is
 * never capped.  cap >= 1; 1 <= topk <= pool <= PCR_RECOMMEND_MAX_K.  For each requested user u:
 *   Pool P_u           exactly the list pcr_recommend_filtered(_model) returns for the same factors, dtype, exclusion, allow set
 *                      and K = pool, without its padding (without an allow set: pcr_recommend(_model)'s list): L entries
 *                      (j_i, s_i), i = 0 .. L - 1, in the recommendation order, the scores the same bits.
 *   Rule               walk the pool in order; entry i is kept iff group[j_i] < 0 or fewer than cap earlier pool entries (kept
 *                      or not) have the same group id.  (Counting kept entries only gives the same lists: once a group is full
 *                      every later entry of it is dropped anyway.)  Integer compares only.
 *   Output             items[n * topk] and scores[n * topk]: the first topk kept entries in pool order, each with its original
 *                      s_i converted to double; a row shorter than topk ends with (-1, -INFINITY).
 *   Status             status[n], one uint8 per requested user (NULL: not written): PCR_CAP_EXACT when the row holds topk items
 *                      or L < pool (the pool is the user's whole eligible catalogue); PCR_CAP_POOL_EXHAUSTED otherwise: a full
 *                      pool ran out before topk items were kept, and a larger pool may continue the list.  A PCR_CAP_EXACT row
 *                      is bit for bit the group-capped top-topk of the user's whole eligible catalogue (an entry's fate depends
 *                      on the entries before it alone, and the pool is a prefix of the catalogue in recommendation order); a
 *                      PCR_CAP_POOL_EXHAUSTED row is a prefix of that list.
 *   Summary            stats (NULL: not written): users = n, exact / exhausted = the users of either status, short_rows = the
 *                      rows with fewer than topk items, kept = the items listed in all rows.
 *   Consequences       with every group id negative, or all group ids distinct, or cap >= pool, the result is pcr_recommend's
 *                      top-topk list bit for bit and every status is PCR_CAP_EXACT; the first kept entry is always pool position
 *                      0; with cap = 1 and a single group every non-empty pool gives exactly one item.
 *   Determinism        a row depends on (u, its pool, group, cap) alone -- not on the other users, the order of users[], batches
 *                      or item splits; two identical calls are bitwise identical; no floating-point arithmetic at all.
 *   Filter             f (NULL: none) as in pcr_recommend_filtered: an allow set restricts the pool.  Candidate rows (cand_ptr)
 *                      are PCR_ERR_UNSUPPORTED; a filter with nothing in it is PCR_ERR_ARG (pass NULL).
 *   Errors             group == NULL, cap < 1, topk < 1, pool < topk, pool > PCR_RECOMMEND_MAX_K and every argument error of
 *                      pcr_recommend_filtered_model are PCR_ERR_ARG, reported on the host before any device is looked for; the
 *                      message names the entry.  Without a device: PCR_ERR_DEVICE. */
#define PCR_CAP_EXACT          0
#define PCR_CAP_POOL_EXHAUSTED 1
typedef struct pcr_cap_stats {
    int64_t users, exact, exhausted, short_rows, kept;
} pcr_cap_stats;
int pcr_recommend_capped_model(const double *U, int64_t d1, const double *V, int64_t d2, int64_t k,
                               const int64_t *index, const int32_t *item, int64_t n, const int32_t *users,
                               int topk, int pool, const int32_t *group, int cap, int dtype, const pcr_item_filter *f,
                               int32_t *items, double *scores, uint8_t *status, pcr_cap_stats *stats,
                               int device);                                                           /* [device] */
/* On a live PCR, PCR++ or CCDR1 solver, as pcr_recommend: its device factors, storage type and stream; users[n] are GLOBAL ids
 * of this rank's shard (NULL: all of them); flags PCR_REC_EXCLUDE_TRAIN; training state is not touched.  stats are this rank's
 * own counts: per user, nothing is exchanged, so it works on every communicator and on local-only shards.
 * Profile slots: recommend/score, and recommend/cap (the merge with the selection fused in). */
int pcr_recommend_capped(pcr_solver *s, int64_t n, const int32_t *users, int topk, int pool, const int32_t *group,
                         int cap, int flags, const pcr_item_filter *f, int32_t *items, double *scores,
                         uint8_t *status, pcr_cap_stats *stats);                                      /* [device] */

/* ------------------------------------------------------------------------- */
/* evaluating given and re-ranked lists (no reference counterpart)            */
/* ------------------------------------------------------------------------- */
/* The metrics of "full-catalogue top-N evaluation" and of "beyond-accuracy top-N metrics" above, definition for definition,
 * over lists the caller brings -- a business-rule filter, another model's output, an A/B arm -- instead of lists the library
 * selects itself: L_u = the given list.  The lists go to the device once; both sets of metrics are reduced there.
 *   Lists              lists[n][L], 1 <= L <= PCR_RECOMMEND_MAX_K, int32, row i in list order for users[i] (NULL: n == d1 and
 *                      row i is user i): 0-based item ids, the non-padding entries first, -1 padding only after them, no id
 *                      twice in a row.  len(u, c) = the number of non-padding entries among the first c.
 *   Cutoffs            as in the top-N evaluation, with cutoffs[ncut - 1] <= L; positions from the last cutoff on belong to no
 *                      metric.
 *   Relevant sets      R_u, the gains and the discounts as in the top-N evaluation, from the test CSR tindex / titem / tval (all
 *                      three NULL: no accuracy part; then topn and per_user_topn must be NULL, and with a test CSR topn is
 *                      required).
 *   Popularity         index / item (the training CSR) give pop[] alone; NULL: pop = 0.  Exclusion is not this entry's
 *                      business: a listed item that also sits in the user's training row is evaluated as listed.
 *   Counted users      div counts every requested user; topn counts the requested users with |R_u| >= 1; a user id given twice
 *                      counts twice in both.
 *   Determinism        as the two evaluations above: per-user rows depend on (the list, the test row, V) alone and are, on the
 *                      list pcr_recommend returns, bit for bit those of pcr_evaluate_topn / pcr_evaluate_diversity; the sums
 *                      over users run in a fixed order (the order of users[]); no floating-point atomics.
 *   Errors             PCR_ERR_ARG, found on the host before any device is looked for, the message naming the entry: a list
 *                      entry outside [0, d2) that is not -1, a non-padding entry after a -1, an id twice in one list, L outside
 *                      [1, PCR_RECOMMEND_MAX_K], a user outside [0, d1), cutoffs[ncut - 1] > L, and the CSR and cutoff errors of
 *                      pcr_evaluate_topn_model / pcr_evaluate_diversity_model.
 * topn[ncut], div[ncut]: the summaries.  per_user_topn (optional): [n][ncut][6] as pcr_evaluate_topn's, row i for users[i], all
 * NaN for an uncounted user.  per_user_div (optional): [n][ncut][PCR_DIVERSITY_FIELDS].  exposure (optional): int64 [ncut][d2].
 * Profile slot (of the solver entry below): recommend/listmetrics. */
int pcr_evaluate_lists_model(const double *V, int64_t d2, int64_t k, int64_t d1,
                             const int64_t *index, const int32_t *item,
                             const int64_t *tindex, const int32_t *titem, const double *tval,
                             int64_t n, const int32_t *users, int L, const int32_t *lists,
                             int ncut, const int *cutoffs, double threshold, int dtype,
                             pcr_topn_stats *topn, double *per_user_topn,
                             pcr_diversity_stats *div, double *per_user_div, int64_t *exposure, int device);   /* [device] */
/* The accuracy / diversity trade-off of the MMR re-ranking: one scoring sweep, then for each of the nth values of theta the
 * re-ranked lists and their metrics -- no list leaves the device.
 *   Arguments          topk = cutoffs[ncut - 1] <= pool <= PCR_RECOMMEND_MAX_K; 1 <= nth <= PCR_RERANK_MAX_THETAS; every theta in
 *                      [0, 1] and not NaN; equal thetas are allowed.
 *   Lists              for thetas[t] the list of user u is exactly what pcr_recommend_diverse(_model) returns for (topk, pool,
 *                      thetas[t]) with the same factors, dtype and exclusion; the metrics are those of pcr_evaluate_lists_model
 *                      on these lists, bit for bit per user.  With thetas[t] == 0 the per-user rows are therefore those of
 *                      pcr_evaluate_topn / pcr_evaluate_diversity at the same cutoffs.  One result does not depend on which
 *                      other thetas are in the call.
 *   Model entry        the test CSR is optional as above; index / item (the training CSR) give exclusion and popularity, as in
 *                      pcr_evaluate_diversity_model.  Every argument error is PCR_ERR_ARG before any device is looked for.
 * topn: [nth][ncut] (NULL: no accuracy part), div: [nth][ncut]; per_user_topn [nth][n][ncut][6], per_user_div
 * [nth][n][ncut][PCR_DIVERSITY_FIELDS] and exposure [nth][ncut][d2] are optional. */
#define PCR_RERANK_MAX_THETAS 8
int pcr_evaluate_rerank_model(const double *U, int64_t d1, const double *V, int64_t d2, int64_t k,
                              const int64_t *index, const int32_t *item,
                              const int64_t *tindex, const int32_t *titem, const double *tval,
                              int64_t n, const int32_t *users, int nth, const double *thetas, int pool,
                              int ncut, const int *cutoffs, double threshold, int dtype,
                              pcr_topn_stats *topn, pcr_diversity_stats *div,
                              double *per_user_topn, double *per_user_div, int64_t *exposure, int device);   /* [device] */
/* On a live PCR, PCR++ or CCDR1 solver: its device factors, storage type and stream, its test ratings (topn NULL: no accuracy
 * part) and its training ratings (exclusion under PCR_REC_EXCLUDE_TRAIN, popularity always); users[n] are GLOBAL ids of this
 * rank's shard (NULL: all of them); training state is not touched.  N ranks with an RCCL communicator: pop, exposure and the
 * sums are all-reduced and every rank returns the totals (every rank must call); on a peer-to-peer communicator the entry is
 * PCR_ERR_UNSUPPORTED, as pcr_evaluate_diversity; a local-only shard returns its own partials.
 * Profile slots: recommend/score (once per user batch, whatever nth is), recommend/rerank (the selection, nth times per batch)
 * and recommend/listmetrics (the row norms, the metrics of the lists, the reductions). */
int pcr_evaluate_rerank(pcr_solver *s, int64_t n, const int32_t *users, int nth, const double *thetas, int pool,
                        int ncut, const int *cutoffs, double threshold, int flags,
                        pcr_topn_stats *topn, pcr_diversity_stats *div,
                        double *per_user_topn, double *per_user_div, int64_t *exposure);                     /* [device] */

/* ------------------------------------------------------------------------- */
/* fold-in: factors for users the model was not trained on (no reference      */
/* counterpart: the reference can only retrain)                               */
/* ------------------------------------------------------------------------- */
/* Given a handful of ratings of each of n new users, their rows of U are found on the device with V fixed: per user,
 * lambda/2 |u|^2 + sum over the user's comparable pairs of hinge^2 is strictly convex in u, and one workgroup runs the user's
 * whole optimisation -- up to `steps` Newton steps, each a gradient, a truncated CG and a line search -- in one launch
 * (k_foldin).  Each user is independent.  Starting from u = U0[i] rounded to the storage type, a step does:
 *   1 State at u       m = V_I u in the storage type, sorted by (level, m); loss and prev_obj = lambda/2 |u|^2 + loss.  Levels as
 *                      in training (lround buckets for PrimalCR++, the dense rank of the raw double for PrimalCR; the windows
 *                      strict for PrimalCR, inclusive for PrimalCR++).
 *   2 End test         the gradient g and gn2 = |g|^2.  The user ends CONVERGED, u unchanged, when it has no rating, when
 *                      gn2 < 1e-4 (the reference's absolute threshold, pcrpp.cpp:787), or when the solver is PrimalCR and the
 *                      user has fewer than two levels (pcr.cpp:552).
 *   3 Newton step      exactly update_u_new (pcrpp.cpp:779-815) / update_u (pcr.cpp:523-585): CG from delta = 0, at most
 *                      cg_max_iter iterations, tolerance cg_tol |g|; the line search from stepsize, halving, at most 20
 *                      evaluations under strict <, each with fresh scores and a fresh sort.
 *   4 Accepted try     u becomes that point ROUNDED TO THE STORAGE TYPE (as the training loop stores it); one more step taken.
 *   5 No try accepted  the user ends STALLED and u IS LEFT AS IT WAS BEFORE THIS STEP.  This departs on purpose from the training
 *                      loop, which moves to the last tried point: a serving call never returns a point worse
 *                      than the one it was given, and never spends another 20 sorts on a user at its noise floor (long users
 *                      often cannot reach the absolute threshold of 2).
 *   6 Step cap         after `steps` accepted steps the user ends STEP_CAP.
 *   Inputs             index[n + 1] / item / val: the new users' ratings as a CSR over the model's items.  Rows need not be
 *                      item-ascending (a sorted copy is made: sums run in ascending item order); the same item twice in a row
 *                      is two ratings, as in training.  U0 [n][k] (NULL: zeros).  steps >= 1.
 *   Outputs            U_out [n][k]: the storage-type values widened.  per_user (optional) [n][PCR_FOLDIN_FIELDS] = steps taken,
 *                      CG iterations, line-search evaluations, obj = lambda/2 |u|^2 + loss at the returned u, gnorm2 = |g|^2 at
 *                      the last point where the gradient was evaluated (the returned u for CONVERGED, else the start of the last
 *                      step), status.  stats (optional): the counts and sums over the users; obj is added in user order.
 *   Determinism        a user's row and statistics depend on its ratings, V and the parameters alone -- not on the other users,
 *                      its position, batches or the launch grid: the workgroup form is chosen by the user's length, every sum
 *                      has a fixed order, no atomics touch results, nothing is exchanged between workgroups and every loop has
 *                      a static bound.  Two identical calls are bitwise identical.
 *   Errors             PCR_ERR_ARG before any device is looked for, the message naming the entry: an item id outside [0, d2), a
 *                      rating that is not finite, index[0] != 0 or a non-monotone index, steps < 1, a null V / U_out, a solver
 *                      type other than 0, 1, 2.  Whatever the level builder refuses (a user with more than 65535 levels) is
 *                      PCR_ERR_UNSUPPORTED, as is solver type 0: the squared-loss fold-in of CCDR1 is a ridge solve, not this.
 * Workgroup forms by user length (a user's form never depends on the call): one wave up to PCR_FOLDIN_WAVE_MAX ratings; 256
 * threads with the per-rating arrays in LDS up to PCR_FOLDIN_LDS_MAX; 512 threads with them in global scratch beyond.  Every
 * pass gathers the user's rows of V from L2. */
#define PCR_FOLDIN_FIELDS 6
#define PCR_FOLDIN_CONVERGED 0
#define PCR_FOLDIN_STEP_CAP  1
#define PCR_FOLDIN_STALLED   2
#define PCR_FOLDIN_WAVE_MAX  64
#define PCR_FOLDIN_LDS_MAX   2048
typedef struct pcr_foldin_stats {
    int64_t users, converged, step_cap, stalled;
    int64_t steps, cg, ls;
    double  obj;
} pcr_foldin_stats;
/* Standalone: V (d2 x k) host fp64 in model-file layout; k, lambda, solver_type, stepsize, cg_max_iter, cg_tol, precision and
 * device are read from p. */
int pcr_fold_in_model(const pcr_params *p, const double *V, int64_t d2, int64_t n,
                      const int64_t *index, const int32_t *item, const double *val,
                      const double *U0, int steps, double *U_out,
                      pcr_foldin_stats *stats, double *per_user);                                  /* [device] */
/* On a live PCR or PCR++ solver: its device V, storage type and parameters, on its stream (a CCDR1 solver: PCR_ERR_STATE).  V is
 * replicated on every rank, so the call is local: nothing is exchanged and any rank may call it alone.  The solver's factors and
 * training state are not touched.  Profile slot: foldin/newton. */
int pcr_fold_in(pcr_solver *s, int64_t n, const int64_t *index, const int32_t *item, const double *val,
                const double *U0, int steps, double *U_out,
                pcr_foldin_stats *stats, double *per_user);                                        /* [device] */

/* ------------------------------------------------------------------------- */
/* ridge fold-in: squared-loss factors for rows the model was not trained on  */
/* (CCDR1 models; no reference counterpart: the reference can only retrain)   */
/* ------------------------------------------------------------------------- */
/* Given a fixed factor matrix F (rows x k) and the ratings of n new users as a CSR over F's rows, each user's row is the exact
 * minimiser of the squared loss with F fixed.  For a user with ratings r on rows I (len of them), A = F[I] (len x k):
 *     minimise |r - A u|^2 + mu |u|^2,    mu = lambda len (weighted != 0: CCDR1's regulariser, ccd-r1.cpp's loss + lambda reg with
 *     reg = sum over rows of nnz_row |u|^2) or mu = lambda (weighted == 0: the plain ridge, for models trained elsewhere).
 * One workgroup solves one user in fp64 (rows of the storage type are widened as they are read; Gram matrices on
 * v_mfma_f64_16x16x4_f64 for both storage types) and rounds the row to the storage type on store.  The same entry folds in new
 * ITEMS: F = U and the item-major ratings (a CSR over U's rows).
 *   Forms              a function of the user's length len and the rank k alone, never of the batch, the position or the grid:
 *                        DUAL    len <= k and len <= PCR_RIDGE_DIRECT_MAX:  (A A^T + mu I) a = r by blocked Cholesky, u = A^T a
 *                        PRIMAL  len > k and roundup(k, 16) <= PCR_RIDGE_DIRECT_MAX:  (A^T A + mu I) u = A^T r by blocked Cholesky,
 *                                the ratings streamed in chunks of 16 (any len)
 *                        CG      everything else: matrix-free conjugate gradient on the primal system from u = 0, until
 *                                |residual|^2 <= 1e-24 |A^T r|^2, at most 2 min(len, k) + 10 iterations
 *                      Users of at most PCR_RIDGE_WAVE_MAX ratings run on one wave (a 64-thread workgroup), longer ones on 256
 *                      threads.  pcr_tune("ridge_form", "cg") forces the CG form for every user ("auto" or removal: the rule).
 *   Statuses           PCR_RIDGE_OK; PCR_RIDGE_SINGULAR: a Cholesky pivot that is <= 0 or not finite, or a CG step with
 *                      p.Hp <= 0 or not finite -- the row is zeros and loss = obj = |r|^2; PCR_RIDGE_CG_CAP: the CG reached its
 *                      iteration cap and its last iterate is returned.
 *   Inputs             index[n + 1] / item / val as pcr_fold_in_model's: rows need not be item-ascending (a sorted copy is made:
 *                      every sum runs in ascending item order); the same item twice in a row is two ratings, as in training.  A
 *                      user without ratings gets a zero row, status OK, loss = obj = 0.
 *   Outputs            U_out [n][k]: the storage-type values widened.  per_user (optional) [n][PCR_RIDGE_FIELDS] = len, form,
 *                      iters (CG form; 0 otherwise), loss, obj, status, where loss = |r - A u^|^2 and obj = loss + mu |u^|^2 are
 *                      evaluated at the RETURNED (rounded) row u^.  stats (optional): the counts, and loss / obj added in user
 *                      order.
 *   Determinism        a user's row and table line depend on its ratings, F and the parameters alone: every sum has a fixed
 *                      order, no atomics, nothing is exchanged between workgroups, every loop has a static bound.  Two identical
 *                      calls are bitwise identical.
 *   Errors             PCR_ERR_ARG before any device is looked for, the message naming the entry: a null F or U_out, k < 1 or
 *                      rows < 1, an item id outside [0, rows), a rating that is not finite, index[0] != 0 or a non-monotone index,
 *                      a lambda that is negative or not finite, an unknown precision.  Without a device: PCR_ERR_DEVICE. */
#define PCR_RIDGE_FIELDS 6
#define PCR_RIDGE_DUAL   0
#define PCR_RIDGE_PRIMAL 1
#define PCR_RIDGE_CG     2
#define PCR_RIDGE_OK       0
#define PCR_RIDGE_SINGULAR 1
#define PCR_RIDGE_CG_CAP   2
#define PCR_RIDGE_WAVE_MAX   64
#define PCR_RIDGE_DIRECT_MAX 112   /* the lower-triangular tiles of a 112 x 112 matrix are 60 KB of LDS: two workgroups per CU */
typedef struct pcr_ridge_stats {
    int64_t users, dual, primal, cg, singular, cg_cap, iters;
    double  loss, obj;
} pcr_ridge_stats;
/* Standalone: F (rows x k) host fp64 in model-file layout. */
int pcr_fold_in_ridge_model(const double *F, int64_t rows, int64_t k, double lambda, int weighted, int precision, int device,
                            int64_t n, const int64_t *index, const int32_t *item, const double *val,
                            double *U_out, pcr_ridge_stats *stats, double *per_user);               /* [device] */
/* On ANY live solver, CCDR1 included: its device V, storage type, stream and lambda.  V is replicated on every rank, so the call
 * is local: nothing is exchanged and any rank may call it alone.  Nothing of the solver is written.  Profile slot: foldin/ridge. */
int pcr_fold_in_ridge(pcr_solver *s, int weighted, int64_t n, const int64_t *index, const int32_t *item, const double *val,
                      double *U_out, pcr_ridge_stats *stats, double *per_user);                     /* [device] */

/* ------------------------------------------------------------------------- */
/* confidence-weighted and implicit fold-in: the ridge fold-in of a model     */
/* trained with rating weights (pcr_solver_set_rating_weights) and / or with  */
/* implicit feedback (pcr_solver_set_implicit); no reference counterpart      */
/* ------------------------------------------------------------------------- */
/* The ridge fold-in's problem under the objective such a model was trained on.  For a user with ratings r_p on rows I of F (len of
 * them), a_p = F[I_p], weights c_p > 0 (all 1 when weight is NULL), alpha >= 0 the weight of every unrated cell (a rating 0), d the
 * rows of F and G = F^T F (k x k):
 *     minimise sum_p c_p (r_p - a_p.u)^2 + alpha (u^T G u - sum_p (a_p.u)^2) + mu |u|^2,
 *     mu = lambda W, W = sum_p c_p + alpha (d - len) (weighted != 0: the row's total weight, as in training) or mu = lambda,
 *     <=>  M u = b,  M = alpha G + sum_p (c_p - alpha) a_p a_p^T + mu I,  b = sum_p c_p r_p a_p
 * -- training's own column update written for a whole row: the sum over all d cells goes through G, computed once per call on
 * v_mfma_f64_16x16x4_f64, and the rated cells are taken back out next to the ratings (an item rated twice is two ratings and two
 * subtractions); the d x len unrated cells are never formed.  With weight NULL (or all 1) and alpha 0 this is the ridge fold-in,
 * bit for bit.  weight and alpha are used in fp64 as given; only F and the returned row have the storage type.  F = U with the
 * item-major ratings folds in new ITEMS.
 *   Forms              a function of (len, k, alpha > 0) alone, never of the batch, the position or the grid:
 *                        alpha == 0  the ridge entry's rule.  DUAL: (A A^T + mu C^-1) a = r, u = A^T a (C = diag c);
 *                                    PRIMAL: (A^T C A + mu I) u = A^T C r; CG: Hp = A^T (c o (A p)) + mu p.
 *                        alpha > 0   PRIMAL at every len >= 1 while roundup(k, 16) <= PCR_RIDGE_DIRECT_MAX (the alpha G term
 *                                    makes the system k x k whatever the length); CG beyond, Hp = A^T ((c - alpha) o (A p)) +
 *                                    alpha G p + mu p with G read from device memory, at most 2 k + 10 iterations.
 *                      One wave (64 threads) up to PCR_RIDGE_WAVE_MAX ratings, except that an implicit primal system of more
 *                      than 4 x 4 tiles (roundup(k, 16) > 64) always runs on 256 threads; 256 threads beyond and for the CG form.
 *                      pcr_tune("ridge_form", "cg") forces the CG form, as for the ridge entry.
 *   Statuses           the ridge entry's.  PCR_RIDGE_SINGULAR rows are zeros with loss = obj = sum_p c_p r_p^2.
 *   Inputs             index / item / val as pcr_fold_in_ridge_model's; weight [index[n]] in the caller's order (the sorted copy
 *                      of a row carries its weights through the same permutation), or NULL.  A user without ratings gets a zero
 *                      row, status OK, loss = obj = 0, at any alpha.
 *   Outputs            as the ridge entry's (pcr_ridge_stats, per_user [n][PCR_RIDGE_FIELDS]), with, at the returned (rounded) row,
 *                      loss = sum_p c_p (r_p - a_p.u^)^2 + alpha (u^^T G u^ - sum_p (a_p.u^)^2) and obj = loss + mu |u^|^2.
 *   Determinism        as the ridge entry's; G's row blocks are fixed by (rows, k) alone and added in block order, no atomics.
 *                      Two identical calls are bitwise identical.
 *   Errors             PCR_ERR_ARG before any device is looked for, the message naming the entry: everything the ridge entry
 *                      refuses, a weight that is not finite or <= 0, an alpha that is negative or not finite.  Without a device:
 *                      PCR_ERR_DEVICE.  Profile slots: foldin/conf, and foldin/conf.gram for G. */
/* Standalone: F (rows x k) host fp64 in model-file layout. */
int pcr_fold_in_conf_model(const double *F, int64_t rows, int64_t k, double lambda, int weighted, double alpha,
                           int precision, int device, int64_t n, const int64_t *index, const int32_t *item,
                           const double *val, const double *weight /* [index[n]] in the caller's order, or NULL = ones */,
                           double *U_out, pcr_ridge_stats *stats, double *per_user);                /* [device] */
/* On ANY live solver, as pcr_fold_in_ridge: its device V, storage type, stream and lambda; nothing of the solver is written.
 * alpha is the caller's: the entry does not read the solver's pcr_solver_set_implicit setting. */
int pcr_fold_in_conf(pcr_solver *s, int weighted, double alpha, int64_t n, const int64_t *index, const int32_t *item,
                     const double *val, const double *weight, double *U_out, pcr_ridge_stats *stats,
                     double *per_user);                                                             /* [device] */

/* ------------------------------------------------------------------------- */
/* non-negative fold-in: rows >= 0 for CCDR1 models trained with -N 1         */
/* (do_nmf, ccd-r1.cpp:19; no reference counterpart)                          */
/* ------------------------------------------------------------------------- */
/* The ridge fold-in's problem under the constraint the model was trained with.  For a user with ratings r on rows I of F (len of
 * them), A = F[I], mu = lambda len (weighted != 0) or lambda (weighted == 0) as above:
 *     minimise |r - A u|^2 + mu |u|^2   subject to u >= 0.
 * With G = A^T A + mu I and b = A^T r the minimiser (unique for mu > 0) has a passive set P with u_P = G_PP^-1 b_P >= 0, u_Z = 0
 * on the complement Z and y = G u - b >= 0 on Z.  It is found by block principal pivoting with exact solves (the Kim-Park rule):
 *     P = all k coordinates;  alpha = 3;  beta = k + 1
 *     for pivot = 1 .. PCR_NNLS_PIVOT_CAP:
 *         u_P = G_PP^-1 b_P,  u_Z = 0;   y_Z = (G u - b)_Z,  y_P = 0
 *         V = { j in P : u_j < 0 }  union  { j in Z : y_j < 0 }
 *         if V is empty: PCR_NNLS_OK, stop
 *         if |V| < beta:   beta = |V|; alpha = 3; X = V
 *         elif alpha > 0:  alpha -= 1;          X = V
 *         else:                                 X = { max V }
 *         P = P xor X
 * Pivot 1 is the unconstrained ridge solve: a user whose ridge row is already >= 0 stops there.  One workgroup solves one user in
 * fp64 and rounds the row to the storage type on store (which keeps >= 0).  F = U and the item-major CSR fold in new items.
 *   Forms              a function of the rank k alone (pcr_nnls_form):
 *                        DIRECT  roundup(k, 16) <= PCR_RIDGE_DIRECT_MAX: G is built once on v_mfma_f64_16x16x4_f64 (the ridge
 *                                entry's primal build) and kept in LDS; every pivot factors a copy with Z masked to a unit
 *                                diagonal by blocked Cholesky and solves for b masked to P; 64 threads per user when the padded
 *                                rank is <= 64, 256 beyond
 *                        CG      wider ranks: the solve on P is the ridge entry's matrix-free CG from u = 0 with the search
 *                                direction masked to P, Hp = mask_P(A^T (A p) + mu p), until |residual|^2 <= 1e-24 |b_P|^2, at
 *                                most 2 min(len, |P|) + 10 iterations; one more pass gives y
 *                      pcr_tune("nnls_form", "cg") forces the CG form ("auto" or removal: the rule).
 *   Statuses           PCR_NNLS_OK; PCR_NNLS_SINGULAR: a masked Cholesky pivot that is <= 0 or not finite, or a CG step with
 *                      p.Hp <= 0 or not finite -- the row is zeros and loss = obj = |r|^2; PCR_NNLS_CAP: PCR_NNLS_PIVOT_CAP pivots
 *                      without an empty V, or a solve that stopped at its CG cap -- the row is the last iterate with its negative
 *                      entries set to 0.  The pivot cap is a safety bound (the rule is finite in exact arithmetic).
 *   Inputs             as pcr_fold_in_ridge_model's.  A user without ratings gets a zero row, status OK, 0 pivots.
 *   Outputs            U_out [n][k]: the storage-type values widened, every one >= 0.  per_user (optional) [n][PCR_NNLS_FIELDS] =
 *                      len, form, pivots, zeros (the coordinates of the returned row that are 0), loss, obj, status; loss and obj
 *                      at the RETURNED (rounded) row.  stats (optional): the counts, and loss / obj added in user order.
 *   Determinism        as the ridge entry's: a user's bits depend on its ratings, F and the parameters alone.
 *   Errors             the ridge entry's, the message naming the nnls entry; PCR_ERR_ARG before any device is looked for.
 *                      Without a device: PCR_ERR_DEVICE. */
#define PCR_NNLS_FIELDS 7
#define PCR_NNLS_DIRECT 0
#define PCR_NNLS_CG     1
#define PCR_NNLS_OK       0
#define PCR_NNLS_SINGULAR 1
#define PCR_NNLS_CAP      2
#define PCR_NNLS_PIVOT_CAP 64
typedef struct pcr_nnls_stats {
    int64_t users, direct, cg, singular, cap, pivots, zeros;
    double  loss, obj;
} pcr_nnls_stats;
/* Standalone: F (rows x k) host fp64 in model-file layout. */
int pcr_fold_in_nnls_model(const double *F, int64_t rows, int64_t k, double lambda, int weighted, int precision, int device,
                           int64_t n, const int64_t *index, const int32_t *item, const double *val,
                           double *U_out, pcr_nnls_stats *stats, double *per_user);                 /* [device] */
/* On ANY live solver: its device V, storage type, stream and lambda (pcr_fold_in_ridge's conventions).  Nothing of the solver is
 * written.  Profile slot: foldin/nnls. */
int pcr_fold_in_nnls(pcr_solver *s, int weighted, int64_t n, const int64_t *index, const int32_t *item, const double *val,
                     double *U_out, pcr_nnls_stats *stats, double *per_user);                       /* [device] */

/* ------------------------------------------------------------------------- */
/* item fold-in: rows of V for items a PrimalCR / PrimalCR++ model was not    */
/* trained on (no reference counterpart: the reference can only retrain)      */
/* ------------------------------------------------------------------------- */
/* U and the trained rows of V are fixed.  New item j has raters R_j, user i gave it r_ij; its row v minimises
 *     F_j(v) = lambda/2 |v|^2 + sum_{i in R_j} phi_ij(u_i . v)
 *     phi_ij(s) = sum_{k in Omega_i, lev(r_ik) < lev(r_ij)} max(0, 1 - s + m_ik)^2
 *               + sum_{k in Omega_i, lev(r_ik) > lev(r_ij)} max(0, 1 + s - m_ik)^2
 * where Omega_i is user i's TRAINING row, m_ik = u_i . v_k rounded to the storage type as training stores it, and lev is the
 * solver's level key (lround for PrimalCR++, the raw double for PrimalCR).  F_j is exactly the change of the training objective
 * when item j and its ratings are appended to the data; it is strictly convex for lambda > 0.  Its gradient is lambda v + U_R^T c
 * with c_i = phi_ij'(s_i), its generalised Hessian lambda I + U_R^T diag(h) U_R with h_i = 2 * (active pairs of rater i at s_i):
 * row j of obtain_g_new / compute_Ha_new on the appended data.  A pair at the boundary (its hinge argument exactly 0) counts as
 * active for PrimalCR++ and not for PrimalCR, as the training windows have it.
 * NEW ITEMS ARE FOLDED IN INDEPENDENTLY OF EACH OTHER: a pair of two new items rated by the same user is not modelled.
 * The user-side kernel cannot serve with the roles swapped: the loss compares items within a user, so a new row couples to the
 * whole training row of every rater.  Two kernels (pcr_itemfold.h): k_rater_scores builds the rater table -- the scores m of the
 * training row of every UNIQUE rater of the batch, once, with the dense level of every rating -- and k_itemfold runs an item's
 * whole optimisation in one workgroup and one launch.  Starting from v = V0[j] rounded to the storage type, a step does:
 *   1 State at v       s = U_R v in the storage type; one scan of each rater's table segment gives phi, c and h.
 *   2 End test         g and gn2 = |g|^2.  The item ends CONVERGED, v unchanged, when it has no rater, when gn2 < 1e-4, or when
 *                      the solver is PrimalCR and no rater's row holds a level different from the new rating's.
 *   3 Newton step      CG from delta = 0 on the generalised Hessian with h frozen at v, at most cg_max_iter iterations, tolerance
 *                      cg_tol |g|; the line search from stepsize, halving, at most 20 evaluations under strict <, each with
 *                      fresh scores and a fresh scan.
 *   4 Accepted try     v becomes that point ROUNDED TO THE STORAGE TYPE; one more step taken.  The try's state is carried: it is
 *                      bit for bit what a fresh evaluation at that v gives, so steps = S equals S chained calls of steps = 1.
 *   5 No try accepted  the item ends STALLED and v IS LEFT AS IT WAS BEFORE THIS STEP.
 *   6 Step cap         after `steps` accepted steps the item ends STEP_CAP.
 *   Inputs             U (d1 x k), V (d2 x k) host fp64 in model-file layout; tr_index[d1 + 1] / tr_item / tr_val: the training
 *                      CSR of the d1 users (only the raters' rows are read; their sums run in the rows' own order; the same item
 *                      twice in a row is two ratings).  index[n + 1] / user / val: the new items' ratings, item-major (a CSR over
 *                      the users).  An item's raters are taken in ascending user order (a sorted copy is made).  The same user
 *                      twice in an item's row counts as two ratings: each is compared with the training row, they are not
 *                      compared with each other.  A rater with an empty training row adds nothing.  V0 [n][k] (NULL: zeros).
 *   Outputs            V_out [n][k]: the storage-type values widened.  per_item (optional) [n][PCR_ITEMFOLD_FIELDS] = raters,
 *                      steps taken, CG iterations, line-search evaluations, obj0 = F_j at the start point, obj = F_j at the
 *                      returned row, gnorm2 = |g|^2 at the last point where the gradient was evaluated (the returned v for
 *                      CONVERGED, else the start of the last step), status (the PCR_FOLDIN_* values).  An item without raters
 *                      ends CONVERGED with its V0 row, gnorm2 = 0.  stats (optional): the counts and sums; obj in item order.
 *   Forms              by the item's rater count alone: one wave up to PCR_ITEMFOLD_WAVE_MAX raters; 256 threads with the
 *                      per-rater arrays in LDS up to PCR_ITEMFOLD_LDS_MAX; 512 threads with them in a per-workgroup slice of
 *                      global scratch beyond (the grid bounded so that the slices stay within 1 GiB).  The rater table takes a
 *                      rater on one wave up to PCR_ITEMFOLD_SCORES_WAVE_MAX training ratings, on 256 threads beyond.
 *   Determinism        an item's row and table line depend on its ratings, its raters' training rows, U, V and the parameters
 *                      alone -- not on the other items, its position, batches or the launch grid: every sum has a fixed order,
 *                      no atomics touch results, nothing is handed between workgroups, there is no spin-wait and every loop has
 *                      a static bound.  The host orders items by descending rater count.  Two identical calls are bitwise equal.
 *   Memory             the rater table (sizeof(T) + 2 bytes per training rating of a unique rater, plus 4 for the item id) is
 *                      capped at 1 GiB of scores and levels (pcr_tune("itemfold_table_bytes")): when a call's unique raters
 *                      exceed it the items are processed in batches (a batch holds at least one item); a row's result does not
 *                      depend on the batching.
 *   Errors             PCR_ERR_ARG before any device is looked for, the message naming the entry: a user id outside [0, d1), a
 *                      rating that is not finite, index[0] != 0 or a non-monotone index (either CSR), a training item of a rater
 *                      outside [0, d2), steps < 1, a null U, V, V_out or training array.  PCR_ERR_UNSUPPORTED: solver type 0 (a
 *                      CCDR1 item is a ridge solve: pcr_fold_in_ridge with F = U), and a rater with more than 65535 levels.
 *                      Two limits of the device forms are PCR_ERR_UNSUPPORTED too, reported when the call reaches the form: a rank
 *                      whose vectors and the per-rater arrays of the form's LARGEST item (PCR_ITEMFOLD_WAVE_MAX resp.
 *                      PCR_ITEMFOLD_LDS_MAX raters) do not fit a workgroup's 160 KiB of LDS -- a function of the rank, the storage
 *                      type and the item's form alone, never of the other items of the call (ranks up to several hundred fit every
 *                      form) -- and an item whose per-rater arrays alone exceed the 1 GiB scratch cap (tens of millions of raters).
 *                      Without a device: PCR_ERR_DEVICE. */
#define PCR_ITEMFOLD_FIELDS 8   /* raters, steps, cg, ls, obj0, obj, gnorm2, status */
#define PCR_ITEMFOLD_WAVE_MAX 64
#define PCR_ITEMFOLD_LDS_MAX  2048
#define PCR_ITEMFOLD_SCORES_WAVE_MAX 64
typedef struct pcr_itemfold_stats {
    int64_t items, converged, step_cap, stalled;
    int64_t steps, cg, ls, raters, unique_raters;
    double  obj;
} pcr_itemfold_stats;
/* Standalone: k, lambda, solver_type, stepsize, cg_max_iter, cg_tol, precision and device are read from p. */
int pcr_fold_in_items_model(const pcr_params *p, const double *U, int64_t d1, const double *V, int64_t d2,
                            const int64_t *tr_index, const int32_t *tr_item, const double *tr_val,
                            int64_t n, const int64_t *index, const int32_t *user, const double *val,
                            const double *V0, int steps, double *V_out,
                            pcr_itemfold_stats *stats, double *per_item);                           /* [device] */
/* On a live PCR or PCR++ solver: its device U and V, storage type, stream and parameters; nothing of the solver is written.  The
 * solver keeps only dense ranks of its ratings, not comparable keys, so `train` supplies the rating values: it must be the data
 * set the solver was created from (its dimensions and nnz are checked against the solver).  Every user must be on the rank: a
 * shard or multi-rank solver returns PCR_ERR_STATE, as does a CCDR1 solver.  Profile slots: itemfold/scores (the rater table) and
 * itemfold/newton. */
int pcr_fold_in_items(pcr_solver *s, const pcr_dataset *train, int64_t n, const int64_t *index, const int32_t *user,
                      const double *val, const double *V0, int steps, double *V_out,
                      pcr_itemfold_stats *stats, double *per_item);                                 /* [device] */

/* ------------------------------------------------------------------------- */
/* explaining recommendations: a score decomposed over the user's own rated   */
/* items (no reference counterpart)                                           */
/* ------------------------------------------------------------------------- */
/* A user's row u is trained to a stationary point of f(u) = lambda_u/2 |u|^2 + sum over the user's comparable pairs of hinge^2.
 * With I the user's training row, the gradient is g = lambda_u u + sum_{p in I} c_p v_{i_p}, c_p the sweep coefficients of
 * obtain_g_u_new (pcrpp.cpp:493-539) that the training and fold-in kernels build.  So for ANY item j
 *     s(u, j) = v_j . u = sum_{p in I} e_p(j) + rho(j),    e_p(j) = -(c_p / lambda_u) (v_{i_p} . v_j),    rho(j) = (v_j . g) / lambda_u
 * one signed contribution per rated item ("because you rated X") and a residual that is zero at a converged row and reports
 * honestly how far from stationarity the row is.  Nothing is approximated.  One workgroup explains one user (k_explain,
 * pcr_explain.h): the state at u, then the listed items in tiles of 16 against the user's rows of V in chunks of 256 ratings.
 *   Inputs             index[n + 1] / item / val: the n users' training rows, as pcr_fold_in_model's.  Rows need not be
 *                      item-ascending (a sorted copy is made, equal items keeping their order; "position" below is the position
 *                      in that sorted row); the same item twice in a row is two ratings.  Levels as in training: lround buckets
 *                      for PrimalCR++, the raw double for PrimalCR, with inclusive resp. strict windows.  U [n][k]: row i is
 *                      rounded to the storage type (p->precision), as training stores it.  lists [n][L]: 0-based item ids, the
 *                      non-padding entries first, then -1 padding; an id may sit in the user's training row (a known item can
 *                      be explained) and may occur twice (the two positions are independent).  1 <= L <= PCR_EXPLAIN_MAX_L,
 *                      1 <= E <= PCR_EXPLAIN_MAX_E.  weights (NULL: 1) [n]: c_u > 0 and finite; the user is explained at
 *                      lambda_u = lambda / c_u, divided once in fp64 on the host -- the rule of pcr_solver_set_user_weights.
 *                      lambda must be finite and > 0 (the decomposition divides by it).
 *   Arithmetic         m = V_I u is formed in the storage type by the kernel primitive pcr_fold_in_model uses: the bits its state
 *                      has for the same row.  Everything after that is fp64: c_p from the sorted m, NOT rounded to the storage
 *                      type; g = lambda_u u + sum c_p v_p; the dots v_{i_p} . v_j, v_j . u and v_j . g over the factors as the
 *                      storage type holds them, widened.  The order of the k-term and n-term sums is fixed but not part of the
 *                      contract; each e_p is good to about (k + 2) 2^-52 sum_t |v_pt v_jt| |c_p| / lambda_u, and the identity
 *                      below to that bound summed over p plus the same for rho and score.  Against another implementation
 *                      c_p also inherits the rounding of m: |dc_p| <= 2 n dm, dm the error of a k-term dot in the storage type.
 *   per_pair           (optional) [n][L][PCR_EXPLAIN_PAIR_FIELDS] = score, support, opposition, residual.  score = v_j . u in
 *                      fp64: the decomposed quantity, NOT the f32 chain of pcr_recommend's scores (they agree to f32 rounding).
 *                      support = sum of the e_p > 0, opposition = sum of the e_p < 0, both added in ascending position;
 *                      residual = rho(j).  score = support + opposition + residual to the bound above.  A padding position
 *                      holds NaN in all four fields.
 *   Contributors       expl_item / expl_contrib [n][L][E]: the user's ratings by DESCENDING e_p, equal e_p by ascending position;
 *                      each entry is the rated item's id and its e_p.  Entries with e_p <= 0 are listed like any other: the
 *                      caller cuts at the sign.  The SIGN OF A ZERO contribution is unspecified: a coefficient that is exactly 0
 *                      gives +0 or -0 by the sign of the dot beside it (the two compare equal in the order).  A user with fewer than E ratings ends the row with (-1, 0.0); a padding list
 *                      position holds (-1, 0.0) throughout.
 *   per_user           (optional) [n][PCR_EXPLAIN_USER_FIELDS] = the rating count, loss (the hinge part of the objective at u,
 *                      unweighted) and gnorm2 = |g|^2 of this entry's fp64 g.  A user without ratings has g = lambda_u u:
 *                      support = opposition = 0, residual = score to rounding, every contributor padding.
 *   stats              (optional) users = n, pairs = the non-padding list positions, contributors = the non-padding contributor
 *                      entries, residual_abs_max = the largest |residual| of a non-padding position (0 without one).
 *   Determinism        a user's output depends on its row, u, V, its list and the parameters alone -- not on the other users,
 *                      its position, batches or the launch grid; its workgroup form on the length of its row alone.  No atomics
 *                      touch results, nothing is handed between workgroups, there is no spin-wait, every loop has a static
 *                      bound and every sum a fixed order: two identical calls are bitwise identical.
 *   Forms              by the user's length, as pcr_fold_in's: one wave up to PCR_FOLDIN_WAVE_MAX ratings; 256 threads with the
 *                      per-rating arrays in LDS up to PCR_FOLDIN_LDS_MAX; 512 threads with them in a per-workgroup slice of
 *                      global scratch beyond.
 *   Errors             PCR_ERR_ARG before any device is looked for, the message naming the entry, in this order: null
 *                      parameters, a null V, k < 1, an unknown precision, a lambda that is not finite or <= 0; then everything
 *                      pcr_fold_in_model refuses of the rows (a solver type other than 0, 1, 2, n < 0, d2 < 1, a null index,
 *                      index[0] != 0, a non-monotone index, null item / val, an item id outside [0, d2), a rating that is not
 *                      finite); a null U, lists, expl_item or expl_contrib; L or E out of range; a list id outside [0, d2) that
 *                      is not -1; a non-padding id after a -1; a weight that is not finite or <= 0.  Solver type 0 is
 *                      PCR_ERR_UNSUPPORTED (a squared-loss row decomposes through its residuals: pcr_explain_ridge below), as is whatever
 *                      the level builder refuses.  A rank whose vectors, tile and the per-rating arrays of the form's LARGEST
 *                      user do not fit a workgroup's 160 KiB of LDS is PCR_ERR_UNSUPPORTED, reported when the call reaches the
 *                      form -- a function of the rank, the storage type and the form alone.  Without a device: PCR_ERR_DEVICE. */
#define PCR_EXPLAIN_MAX_L 128      /* listed items per user */
#define PCR_EXPLAIN_MAX_E 16       /* contributors reported per listed item */
#define PCR_EXPLAIN_PAIR_FIELDS 4  /* score, support, opposition, residual */
#define PCR_EXPLAIN_USER_FIELDS 3  /* ratings, loss, gnorm2 */
typedef struct pcr_explain_stats {
    int64_t users, pairs, contributors;
    double  residual_abs_max;
} pcr_explain_stats;
/* Standalone: V (d2 x k) and the users' rows U (n x k) host fp64 in model-file layout; k, lambda, solver_type, precision and
 * device are read from p. */
int pcr_explain_model(const pcr_params *p, const double *V, int64_t d2, int64_t n,
                      const int64_t *index, const int32_t *item, const double *val,
                      const double *U, const double *weights, int L, const int32_t *lists, int E,
                      int32_t *expl_item, double *expl_contrib, double *per_pair, double *per_user,
                      pcr_explain_stats *stats);                                                   /* [device] */
/* On a live PCR or PCR++ solver: its device U and V, storage type, lambda, solver type and stream.  users[n] are GLOBAL ids of the
 * shard (NULL: all of them in order; n is then ignored and taken as the shard's n_users.  Ids outside it: PCR_ERR_ARG).  train must be the data set the solver was
 * created from (its dimensions and nnz are checked, as pcr_fold_in_items does): it supplies the rows and their rating values.
 * A CCDR1 solver, a multi-rank solver or one from pcr_solver_create_shard is PCR_ERR_STATE.  weights [n] is the caller's: the
 * entry does not read the solver's own.  Nothing of the solver is written: training that continues afterwards gives bitwise the
 * same factors.  Profile slot: explain/contrib. */
int pcr_explain(pcr_solver *s, const pcr_dataset *train, int64_t n, const int32_t *users,
                const double *weights, int L, const int32_t *lists, int E,
                int32_t *expl_item, double *expl_contrib, double *per_pair, double *per_user,
                pcr_explain_stats *stats);                                                         /* [device] */

/* ------------------------------------------------------------------------- */
/* explaining squared-loss recommendations: a CCDR1 / ridge row's score over   */
/* the user's own rated items (no reference counterpart)                      */
/* ------------------------------------------------------------------------- */
/* For squared-loss factorisation the explanation is Hu, Koren and Volinsky's ("Collaborative filtering for implicit feedback
 * datasets", ICDM 2008, section 5): the score is a sum over the user's rated items of rating x a user-specific similarity taken
 * through the inverse of the user's regularised Gram matrix.  It is exact.
 *   Definition         Take user i with its training row sorted by item id, equal items keeping their order; "position" p = 0 ..
 *                      len - 1 is the position in that sorted row.  The row has items i_p and ratings r_p; A = F[I] is len x k,
 *                      the storage-type values widened to fp64 as they are read; mu = lambda len when weighted != 0, else
 *                      mu = lambda (pcr_fold_in_ridge's rule); u^ = U[i] rounded to the storage type.  The free set P is every
 *                      coordinate when nonneg == 0 and { t : u^_t > 0 } when nonneg != 0 (a row trained with -N 1, or one that
 *                      pcr_fold_in_nnls returned); Z is its complement.  With G = A_P^T A_P + mu I and b = A_P^T r:
 *                          u*_P = G^-1 b, u*_Z = 0;    for a listed item j with row v_j of F: (z_j)_P = G^-1 (v_j)_P, (z_j)_Z = 0
 *                          e_p(j)      = r_p (v_{i_p} . z_j)          contribution of rated item i_p
 *                          sum_p e_p(j) = v_j . u*                    (exactly, in exact arithmetic)
 *                          score(j)    = v_j . u^                     (fp64 -- not pcr_recommend's f32 chain)
 *                          residual(j) = v_j . (u^ - u*)              how far the given row is from the exact minimiser on P
 *                          score       = support + opposition + residual
 *                      support / opposition are the sums of the positive / negative e_p, added in ascending position.
 *                      U == NULL explains the exact minimiser itself: u^ := u* unrounded and residual = +0.0; U == NULL with
 *                      nonneg != 0 is PCR_ERR_ARG (the free set comes from the row).  A user without ratings has u* = 0 and no
 *                      system is formed (mu may be 0 there): support = opposition = 0, residual = score, every contributor is
 *                      padding; the same holds with |P| = 0.  F = U with an item-major CSR explains an item's row by its raters:
 *                      the entry only sees F.
 *   Arithmetic         everything after an element of F or U is read is fp64, in both storage types, as in pcr_explain and the
 *                      ridge kernels: G on v_mfma_f64_16x16x4_f64, a blocked Cholesky, the two triangular solves for u* and for
 *                      every listed item, the dots.  The order of every sum is fixed but not part of the contract.  lambda must be
 *                      finite and > 0, so G is positive definite; a Cholesky pivot that is <= 0 or not finite still gives status
 *                      PCR_RIDGE_SINGULAR for that user: contributors are padding, support = opposition = 0, residual = score.
 *   Outputs            as pcr_explain's.  expl_item / expl_contrib [n][L][E]: the user's ratings by DESCENDING e_p, equal e_p by
 *                      ascending position; entries <= 0 are listed like any other; the sign of a zero is unspecified; the padding
 *                      is (-1, 0.0).  per_pair (optional) [n][L][PCR_EXPLAIN_PAIR_FIELDS] = score, support, opposition,
 *                      residual; padding positions hold NaN.  per_user (optional) [n][PCR_EXPLAIN_RIDGE_USER_FIELDS] = len, |P|,
 *                      loss = |r - A u^|^2, dist2 = |u^ - u*|^2, status (PCR_RIDGE_OK or PCR_RIDGE_SINGULAR).  stats (optional):
 *                      users = n, pairs = the non-padding list positions, contributors = the non-padding contributor entries,
 *                      singular = the users with status SINGULAR, residual_abs_max = the largest |residual| of a non-padding
 *                      position (0 without one).  lists [n][L] as pcr_explain's: non-padding ids first, then -1; an id may sit
 *                      in the row and may occur twice; 1 <= L <= PCR_EXPLAIN_MAX_L, 1 <= E <= PCR_EXPLAIN_MAX_E.
 *   Determinism        a user's output depends on its row, u^, F, its list and the parameters alone -- not on the other users, its
 *                      position or the launch grid.  No atomics touch results, nothing is handed between workgroups, there is no
 *                      spin-wait, every loop has a static bound and every sum a fixed order: two identical calls are bitwise
 *                      identical.  One workgroup form (256 threads) for every row length and rank (k_explain_ridge,
 *                      pcr_explain_ridge.h).
 *   Errors             PCR_ERR_ARG before any device is looked for, the message naming the entry, in this order: a null F, k < 1,
 *                      rows < 1 or beyond 2^31, an unknown precision, a lambda that is not finite or < 0, n < 0, a null index,
 *                      index[0] != 0, a non-monotone index, null item / val, an item id outside [0, rows), a rating that is not
 *                      finite; a lambda that is 0; U == NULL with nonneg != 0; null lists, expl_item or expl_contrib; L or E out
 *                      of range; a list id outside [0, rows) that is not -1; a non-padding id after a -1.  Then a rank with
 *                      roundup(k, 16) > PCR_RIDGE_DIRECT_MAX is PCR_ERR_UNSUPPORTED -- a function of k alone, reported before
 *                      any device work (a matrix-free form for wide ranks stays out).  Without a device: PCR_ERR_DEVICE. */
#define PCR_EXPLAIN_RIDGE_USER_FIELDS 5  /* ratings, free, loss, dist2, status */
typedef struct pcr_explain_ridge_stats {
    int64_t users, pairs, contributors, singular;
    double  residual_abs_max;
} pcr_explain_ridge_stats;
/* Standalone: F (rows x k) and the users' rows U (n x k, or NULL) host fp64 in model-file layout. */
int pcr_explain_ridge_model(const double *F, int64_t rows, int64_t k, double lambda, int weighted, int nonneg,
                            int precision, int device, int64_t n,
                            const int64_t *index, const int32_t *item, const double *val,
                            const double *U /* [n][k] or NULL */, int L, const int32_t *lists, int E,
                            int32_t *expl_item, double *expl_contrib, double *per_pair, double *per_user,
                            pcr_explain_ridge_stats *stats);                                   /* [device] */
/* On a live single-rank solver from pcr_solver_create (CCDR1 is the intended one; any solver type runs): its device U and V
 * (F = V), storage type, stream and the lambda pcr_fold_in_ridge runs with.  users[n] are GLOBAL ids (NULL: all of them in order;
 * n is then ignored.  Ids outside the solver's users: PCR_ERR_ARG).  train must be the data set the solver was created from (its
 * dimensions and nnz are checked, as pcr_explain checks it): it supplies the rows and their rating values.  nonneg is the
 * caller's: the entry does not read -N from the solver.  A multi-rank solver or one from pcr_solver_create_shard is
 * PCR_ERR_STATE.  Nothing of the solver is written: training that continues afterwards gives bitwise the same factors.
 * Profile slot: explain/ridge. */
int pcr_explain_ridge(pcr_solver *s, const pcr_dataset *train, int64_t n, const int32_t *users,
                      int weighted, int nonneg, int L, const int32_t *lists, int E,
                      int32_t *expl_item, double *expl_contrib, double *per_pair, double *per_user,
                      pcr_explain_ridge_stats *stats);                                         /* [device] */

/* per-kernel device timing (HIP events on the solver's stream, one pair per launch).
 * slot names: "<class>/<workgroup size>[.<length bound>][g][c][l][r][#n]" for the per-user kernels (classes
 * prepare, vgrad, vhv, ustep; g = global-scratch variant, c = workgroup clusters, l = k_ustep's latency form (8 rows
 * in flight), r = one-wave k_ustep class with LDS-resident rows, #n = the n-th kernel symbol
 * of a workgroup form that two length classes of the U step share -- every class is its own symbol in a
 * profiler's per-kernel tables; "vgrad/all", "vhv/all" = both LDS classes in one launch), "wall:<class>" for
 * the fork..join wall time of a class whose length classes run concurrently, and "sddmm", "spmm",
 * "spmm_fin", "cg", "eval", "allreduce".
 * pcr_profile_list writes the comma-separated names of the slots seen so far.
 * pcr_profile_enable(s, n): n = 0 off, 1 time every launch, n > 1 time every n-th launch of each
 * slot (an event pair costs ~3 us of queue time, so sampling keeps the timed region honest);
 * pcr_profile_get returns the summed time and the number of TIMED launches, pcr_profile_launches the number of
 * launches of the slot since the last reset, timed or not (total time of a sampled slot = average x launches);
 * pcr_profile_scope what ONE launch of the slot covers on this rank: the ratings and users of its length
 * class (the whole shard for the rating-/item-parallel kernels), so that a caller can price a launch
 * without mirroring the class layout. */
int pcr_profile_enable(pcr_solver *s, int on);
int pcr_profile_list(pcr_solver *s, char *buf, int64_t cap);
int pcr_profile_get(pcr_solver *s, const char *name, double *total_ms, int64_t *launches);
int pcr_profile_launches(pcr_solver *s, const char *name, int64_t *launches);
int pcr_profile_scope(pcr_solver *s, const char *name, int64_t *ratings, int64_t *users);
int pcr_profile_reset(pcr_solver *s);
/* blocks until the solver's stream is idle */
int pcr_solver_sync(pcr_solver *s);

#ifdef __cplusplus
}
#endif
#endif /* PRIMALCR_H */
