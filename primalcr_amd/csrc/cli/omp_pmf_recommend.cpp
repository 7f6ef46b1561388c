// omp-pmf-recommend -- top-K unrated items per user from a model file (pcr_recommend_model, include/primalcr.h), or, with
// --eval, the full-catalogue top-N evaluation of those lists against a data directory's test ratings (pcr_evaluate_topn_model).
// The reference has no counterpart: pmf-predict.cpp scores the pairs of a test file only.
//   omp-pmf-recommend [-K topk] [-x data_dir] [-u users_file] [--f32] [--scores] model_file output_file
//   omp-pmf-recommend --eval data_dir [-c c1,c2,...] [--threshold v] [--ranks] [-K topk] [-x data_dir] [--f32] model_file [output_file]
//     -K topk        items per user (default 10, at most PCR_RECOMMEND_MAX_K)
//     -x data_dir    leave out the training ratings of a data directory (its meta file; d1 / d2 must match the model)
//     -u users_file  one 1-based user id per line (default: every user of the model)
//     --f32          score with f32 factors (default: fp64, as the model file holds them)
//     --scores       write every item as item:score (score in "%lf", as omp-pmf-predict prints it)
//     --eval dir     evaluate against the test file of a data directory (its meta file; d1 / d2 must match the model)
//     -c cutoffs     comma-separated ascending cutoffs, at most PCR_TOPN_MAX_CUTOFFS (default: -K)
//     --threshold v  a test rating is relevant when >= v (default: every test rating)
//     --ranks        also the exact full-catalogue rank metrics (pcr_evaluate_ranks_model)
//   omp-pmf-recommend --diversity [-x data_dir] [-c c1,c2,...] [-u users_file] [-K topk] [--f32] model_file [output_file]
//     --diversity    beyond-accuracy metrics of the lists (pcr_evaluate_diversity_model): coverage, Gini index of item exposure,
//                    novelty (popularity from -x's training ratings) and intra-list diversity; not together with --eval
//   omp-pmf-recommend --mmr theta [--pool P] [-K topk] [-x data_dir] [-u users_file] [--f32] [--scores] model_file output_file
//     --mmr theta    re-rank every list by Maximal Marginal Relevance (pcr_recommend_diverse_model): the -K items are taken
//                    greedily from the user's P best, theta in [0, 1] weighing likeness (cosine of rows of V) against score;
//                    the output format is that of the plain list; not together with --eval or --diversity
//     --pool P       the pool of --mmr (default min(1024, 10 K)); refused without --mmr, --tradeoff or --max-per-group
//   omp-pmf-recommend --tradeoff t1,t2,... [--pool P] [-K topk] [-c c1,...] [--eval data_dir [--threshold v]] [-x data_dir] [-u users_file] [--f32] model_file
//     --tradeoff ts  the accuracy / diversity trade-off of --mmr (pcr_evaluate_rerank_model): at most PCR_RERANK_MAX_THETAS thetas
//                    in [0, 1]; the catalogue is scored once, every theta's lists are re-ranked and evaluated on the device.  The
//                    lists hold the largest cutoff's items (default -K) out of the user's P best.  For each theta and cutoff
//                    stdout gets the --eval line (with --eval) and the --diversity line, each prefixed with "theta <t> " (%g).
//                    Not together with --mmr, --diversity, --ranks, --scores or an output file
//   omp-pmf-recommend --fold-in data_dir -l lambda [-s 1|2] [--steps S] [-K topk] [--f32] [--scores] model_file output_file
//   omp-pmf-recommend --fold-in data_dir -l lambda [-s 1|2] [--steps S] --eval data_dir [-c ...] [--threshold v] [--f32] model_file [output_file]
//     --fold-in dir  lists for users the model was not trained on (pcr_fold_in_model): the users are the rows of the data
//                    directory's training file (its d2 must equal the model's, its d1 is free); their factors are found on the
//                    device against the model's V and their ratings are left out of the lists.  stdout gets one line "foldin users n
//                    converged n step_cap n stalled n steps n cg n ls n obj x" (%g), then the lists go to output_file in the plain
//                    format (pcr_recommend_model on the new factors).  With --eval the folded-in users are scored against that
//                    directory's test ratings instead (strong generalisation: held-out users, folded in on their training part,
//                    evaluated on their test part) and the --eval lines follow.  Not together with -x, -u, --diversity, --mmr,
//                    --tradeoff or --ranks
//     -l lambda      the regulariser the model was trained with (required with --fold-in)
//     -s 1|2         1 = PrimalCR, 2 = PrimalCR++ (default) levels and windows;  --steps S: at most S Newton steps per user (default 10)
//   omp-pmf-recommend --fold-in-ridge data_dir -l lambda [--plain-reg] [-K topk] [--f32] [--scores] model_file output_file
//   omp-pmf-recommend --fold-in-ridge data_dir -l lambda [--plain-reg] --eval data_dir [-c ...] [--threshold v] [--f32] model_file [output_file]
//     --fold-in-ridge dir  --fold-in for squared-loss models (CCDR1, -s 0; pcr_fold_in_ridge_model): each new user's row is the exact
//                    minimiser of |r - V_I u|^2 + mu |u|^2, mu = lambda x the user's rating count (CCDR1's regulariser) or, with
//                    --plain-reg, mu = lambda.  stdout gets one line "foldin_ridge users n dual n primal n cg n singular n cg_cap n
//                    iters n loss x obj x" (%g); everything else as --fold-in, with the same exclusions of other modes; takes no -s
//                    and no --steps
//   omp-pmf-recommend --fold-in-ridge data_dir -l lambda [--rating-weights file] [--implicit alpha] ...
//     --rating-weights file, --implicit alpha  --fold-in-ridge for a model trained with omp-pmf-train's options of the same names
//                    (pcr_fold_in_conf_model): file holds 'user item weight' lines, one per rating of data_dir, matched with
//                    pcr_dataset_match_weights; alpha is the weight of every unrated cell (finite, >= 0).  Malformed values are
//                    refused before any device work.  The summary line starts with "foldin_conf".  Refused with --fold-in,
//                    --fold-in-nnls and --fold-in-items.
//   omp-pmf-recommend --fold-in-nnls data_dir -l lambda [--plain-reg] [-K topk] [--f32] [--scores] model_file output_file
//   omp-pmf-recommend --fold-in-nnls data_dir -l lambda [--plain-reg] --eval data_dir [-c ...] [--threshold v] [--f32] model_file [output_file]
//     --fold-in-nnls dir  --fold-in-ridge under u >= 0, for CCDR1 models trained with -N 1 (pcr_fold_in_nnls_model): each new user's
//                    row is the exact minimiser of the same objective over the non-negative rows.  stdout gets one line
//                    "foldin_nnls users n direct n cg n singular n cap n pivots n zeros n loss x obj x" (%g); combinations and
//                    refusals as --fold-in-ridge, which it does not go with
//   omp-pmf-recommend --fold-in-items ratings_file -x data_dir -l lambda [-s 1|2] [--steps S] [--f32] model_file output_model
//     --fold-in-items f  rows of V for items the model was not trained on (pcr_fold_in_items_model): the file holds lines "user item
//                    rating", 1-based; the items are 1 .. n and number the NEW items (n, the largest id, may not exceed the number
//                    of lines: an id without a line is an item without raters, a stray huge id is refused), the users are the model's.  -x is required and
//                    supplies the training ratings of the model's users (d1 / d2 must match the model).  output_model is the model
//                    file with V extended by the n rows: new item t becomes item d2 + t.  stdout gets one line "foldin_items items n
//                    converged n step_cap n stalled n steps n cg n ls n raters n unique_raters n obj x" (obj in %g).  Refused
//                    together with every other mode (--eval, --diversity, --mmr, --tradeoff, --ranks, --fold-in, --fold-in-ridge,
//                    --fold-in-nnls, --allow, --candidates) and with -K, -u, -c, --threshold, --pool, --scores and --plain-reg
//   omp-pmf-recommend [--allow items_file] [--candidates file] [-K topk] [-x data_dir] [-u users_file] [--f32] [--scores] model_file output_file
//     --allow file   recommend among these items only (pcr_recommend_filtered_model): one 1-based item id per line, like -u
//     --candidates f a candidate list per requested user: line i holds the space-separated 1-based item ids of the i-th requested
//                    user (any order, no id twice; an empty line is an empty row), as many lines as users; the list is the -K best
//                    of them.  Both go with the plain list and --scores and intersect with each other and with -x; not together
//                    with --eval, --diversity, --mmr, --tradeoff, --ranks or --fold-in
//   omp-pmf-recommend --eval data_dir [--among items_file] [--eval-candidates file | --negatives N [--seed S]] [--ranks] [-c ...] [--threshold v] [-x data_dir] [--f32] model_file [output_file]
//     --among file   evaluate within these items only (pcr_evaluate_topn_filtered_model, pcr_evaluate_ranks_filtered_model): the
//                    format of --allow; a test item outside them is not relevant
//     --eval-candidates f  evaluate within a candidate row per user: the format of --candidates, one line per user of the model
//     --negatives N  sampled-candidate evaluation: every user with test ratings is ranked among its test items and N items drawn
//                    (pcr_sample_negatives, --seed S, default 0) from those in neither its test row nor -x's training row
//                    All three go with --eval only (with or without --ranks), intersect, keep the formats of --eval / --ranks and
//                    are refused with --fold-in*, --diversity, --mmr and --tradeoff; --negatives does not go with --eval-candidates
//   omp-pmf-recommend --groups file --max-per-group q [--pool P] [--allow items_file] [-K topk] [-x data_dir] [-u users_file] [--f32] [--scores] model_file output_file
//     --groups file  exactly d2 lines: line j holds the integer group id of item j, a negative id means "in no group"
//     --max-per-group q  at most q items of one group in a list (pcr_recommend_capped_model): the -K items are the first of the
//                    user's P best (--pool, default min(1024, 10 K)) that the rule keeps; the output format is that of the plain
//                    list; stdout gets one line "capped users n exact n pool_exhausted n short n kept n".  The two flags go
//                    together and with --allow; not together with --candidates, --eval, --diversity, --mmr, --tradeoff, --ranks
//                    or any --fold-in*
//   omp-pmf-recommend --explain file [--top E] -x data_dir -l lambda [-s 1|2] [--allow items_file] [-K topk] [-u users_file] [--f32] [--scores] model_file output_file
//     --explain file why every listed item scores as it does (pcr_explain_model): after the lists are written, `file` gets one line
//                    per requested user and list position, "user item score support opposition residual  it1:c1 it2:c2 ...": the
//                    1-based ids, score = v . u split exactly into the contributions c of the user's own rated items it (the
//                    --top E largest, default 5, at most PCR_EXPLAIN_MAX_E; support / opposition: the sums of all positive /
//                    negative ones) and a residual that is 0 at a converged row; numbers in %g, padding left out.  Needs -x (the
//                    training ratings the model was trained on), -l (its regulariser) and -K <= PCR_EXPLAIN_MAX_L; -s as
//                    --fold-in's.  Goes with the plain list (and --allow) only: refused with --eval, --diversity, --mmr,
//                    --tradeoff, --ranks, any --fold-in*, --groups and --candidates
//   omp-pmf-recommend --explain-ridge file [--top E] -x data_dir -l lambda [--plain-reg] [--nonneg] [--allow items_file] [-K topk] [-u users_file] [--f32] [--scores] model_file output_file
//     --explain-ridge file  the same for a squared-loss (CCDR1, -s 0) model (pcr_explain_ridge_model): the contributions are
//                    rating x the similarity of the rated and the listed item through the inverse of the user's regularised
//                    Gram matrix, the residual is the distance of the model's row from the exact minimiser.  Output format,
//                    --top, -x, -l and -K as --explain's; the regulariser is weighted by each user's rating count as in CCDR1
//                    training, --plain-reg: the plain lambda |u|^2; --nonneg: a model trained with -N 1 (the system is
//                    restricted to the coordinates where the row is > 0).  No -s, no --steps; not together with --explain;
//                    refused with what --explain is refused with
// Output: one line per user, in input order: the 1-based user id, then the 1-based item ids (padding is left out).  Users go
// to the device in batches, so host memory for the lists stays bounded on any catalogue.
// With --eval: stdout gets one line per cutoff, "cutoff c users n users_graded n hits n precision x recall x hit_rate x map x
// ndcg x ndcg_graded x" (values in %g); the output file, if given, one line per counted user at the largest cutoff: the 1-based
// user id, then hits precision recall ap ndcg ndcg_graded (%g; nan where ndcg_graded is undefined).
// With --diversity: stdout gets one line per cutoff, "diversity@c users n users_ild n recs n items_covered n coverage x gini x
// novelty x ild x" (values in %g); the output file, if given, one line per requested user at the largest cutoff: the 1-based
// user id, then len novelty ild (%g).
// With --eval --ranks: after the cutoff lines one line "ranks users n users_auc n relevant n mrr x mean_rank x auc x mpr x"; the
// output file then holds, per counted user, the 1-based user id, then first_rank rr mean_rank auc mpr (%g) instead.
#include <algorithm>
#include <cerrno>
#include <charconv>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <unistd.h>

#include "primalcr.h"

static const char* USAGE =
    "Usage: omp-pmf-recommend [-K topk] [-x data_dir] [-u users_file] [--f32] [--scores] model_file output_file\n"
    "       omp-pmf-recommend --eval data_dir [-c c1,c2,...] [--threshold v] [--ranks] [-K topk] [-x data_dir] [--f32] model_file [output_file]\n"
    "    -K topk        items per user (default 10, 1 .. 1024)\n"
    "    -x data_dir    leave out the training ratings of this data directory (meta file)\n"
    "    -u users_file  one 1-based user id per line (default: every user)\n"
    "    --f32          score in f32 (default fp64)\n"
    "    --scores       write item:score instead of item\n"
    "    --eval dir     top-N metrics against the test ratings of this data directory (meta file)\n"
    "    -c cutoffs     comma-separated ascending cutoffs, at most 8, each 1 .. 1024 (default: -K)\n"
    "    --threshold v  a test rating is relevant when >= v (default: every test rating)\n"
    "    --ranks        with --eval: also a line of exact full-catalogue rank metrics (mrr, mean_rank, auc, mpr)\n"
    "       omp-pmf-recommend --diversity [-x data_dir] [-c c1,c2,...] [-u users_file] [-K topk] [--f32] model_file [output_file]\n"
    "    --diversity    coverage, Gini index of item exposure, novelty (popularity from -x) and intra-list diversity of the lists;\n"
    "                   output_file optional: per requested user at the largest cutoff, len novelty ild\n"
    "       omp-pmf-recommend --mmr theta [--pool P] [-K topk] [-x data_dir] [-u users_file] [--f32] [--scores] model_file output_file\n"
    "    --mmr theta    re-rank the lists by Maximal Marginal Relevance: -K items taken greedily from the user's P best,\n"
    "                   theta in 0 .. 1 (0: the plain list); output as the plain list; not with --eval or --diversity\n"
    "    --pool P       the pool of --mmr, topk .. 1024 (default min(1024, 10 topk)); only with --mmr\n"
    "    output_file    with --eval optional: per counted user at the largest cutoff, hits precision recall ap ndcg ndcg_graded;\n"
    "                   with --ranks: per counted user first_rank rr mean_rank auc mpr\n"
    "       omp-pmf-recommend --tradeoff t1,t2,... [--pool P] [-K topk] [-c c1,...] [--eval data_dir [--threshold v]] [-x data_dir] [-u users_file] [--f32] model_file\n"
    "    --tradeoff ts  metrics of the --mmr lists for up to 8 comma-separated thetas in 0 .. 1, one scoring pass: per theta and\n"
    "                   cutoff the --eval line (with --eval) and the --diversity line, each prefixed with \"theta <t> \";\n"
    "                   not with --mmr, --diversity, --ranks, --scores or an output file\n"
    "       omp-pmf-recommend --fold-in data_dir -l lambda [-s 1|2] [--steps S] [-K topk] [--f32] [--scores] model_file output_file\n"
    "       omp-pmf-recommend --fold-in data_dir -l lambda [-s 1|2] [--steps S] --eval data_dir [-c ...] [--threshold v] [--f32] model_file [output_file]\n"
    "    --fold-in dir  lists for new users: the rows of this data directory's training file (same items as the model, any number\n"
    "                   of users) are folded into the model on the device, their ratings are left out of the lists; stdout gets a\n"
    "                   \"foldin users n converged n step_cap n stalled n steps n cg n ls n obj x\" line; with --eval the new users\n"
    "                   are scored against that directory's test ratings; not with -x, -u, --diversity, --mmr, --tradeoff or --ranks\n"
    "    -l lambda      the regulariser of the model (required with --fold-in)\n"
    "    -s 1|2         1 = PrimalCR, 2 = PrimalCR++ (default);  --steps S  at most S Newton steps per user (default 10)\n"
    "       omp-pmf-recommend --fold-in-ridge data_dir -l lambda [--plain-reg] [-K topk] [--f32] [--scores] model_file output_file\n"
    "       omp-pmf-recommend --fold-in-ridge data_dir -l lambda [--plain-reg] --eval data_dir [-c ...] [--threshold v] [--f32] model_file [output_file]\n"
    "    --fold-in-ridge dir  --fold-in for squared-loss (CCDR1, -s 0) models: the exact ridge solution per new user; stdout gets a\n"
    "                   \"foldin_ridge users n dual n primal n cg n singular n cg_cap n iters n loss x obj x\" line; -l lambda is\n"
    "                   weighted by each user's rating count as in CCDR1 training; --plain-reg: the plain lambda |u|^2; no -s, --steps\n"
    "       omp-pmf-recommend --fold-in-ridge data_dir -l lambda [--rating-weights file] [--implicit alpha] ...\n"
    "    --rating-weights file, --implicit alpha  with --fold-in-ridge: the fold-in of a model trained with omp-pmf-train's options of\n"
    "                   the same names: per-rating confidence weights ('user item weight' lines, one per rating of data_dir) and the\n"
    "                   weight of every unrated cell (finite, >= 0); the summary line starts with foldin_conf; not with --fold-in,\n"
    "                   --fold-in-nnls or --fold-in-items\n"
    "       omp-pmf-recommend --fold-in-nnls data_dir -l lambda [--plain-reg] [-K topk] [--f32] [--scores] model_file output_file\n"
    "       omp-pmf-recommend --fold-in-nnls data_dir -l lambda [--plain-reg] --eval data_dir [-c ...] [--threshold v] [--f32] model_file [output_file]\n"
    "    --fold-in-nnls dir  --fold-in-ridge under u >= 0, for CCDR1 models trained with -N 1: the exact non-negative minimiser per new\n"
    "                   user; stdout gets a \"foldin_nnls users n direct n cg n singular n cap n pivots n zeros n loss x obj x\" line;\n"
    "                   -l, --plain-reg and the refusals as --fold-in-ridge, which it does not go with\n"
    "       omp-pmf-recommend --fold-in-items ratings_file -x data_dir -l lambda [-s 1|2] [--steps S] [--f32] model_file output_model\n"
    "    --fold-in-items f  rows of V for new items: lines \"user item rating\" (1-based; items 1 .. n number the new items) are folded\n"
    "                   into the model on the device against the training ratings of -x (required); output_model is the model with V\n"
    "                   extended by the n rows (new item t becomes item d2 + t); stdout gets a \"foldin_items items n converged n\n"
    "                   step_cap n stalled n steps n cg n ls n raters n unique_raters n obj x\" line; not with any other mode\n"
    "       omp-pmf-recommend [--allow items_file] [--candidates file] [-K topk] [-x data_dir] [-u users_file] [--f32] [--scores] model_file output_file\n"
    "    --allow file   recommend among these items only: one 1-based item id per line\n"
    "    --candidates f line i: the space-separated 1-based candidate items of the i-th requested user (an empty line: none);\n"
    "                   the list is the -K best of them; both go with the plain list and --scores only\n"
    "       omp-pmf-recommend --eval data_dir [--among items_file] [--eval-candidates file | --negatives N [--seed S]] [--ranks] [-c ...] [--threshold v] [-x data_dir] [--f32] model_file [output_file]\n"
    "    --among file   with --eval: evaluate within these items only (one 1-based item id per line); a test item outside is not relevant\n"
    "    --eval-candidates f  with --eval: evaluate within a candidate row per user; line i: the 1-based items of user i of the model\n"
    "    --negatives N  with --eval: every user's test items against N sampled items outside its test row and -x's training row;\n"
    "                   --seed S (default 0) picks the sample; not with --eval-candidates; the output keeps --eval's / --ranks' formats\n"
    "       omp-pmf-recommend --groups file --max-per-group q [--pool P] [--allow items_file] [-K topk] [-x data_dir] [-u users_file] [--f32] [--scores] model_file output_file\n"
    "    --groups file  one line per item of the model: line j holds the integer group id of item j (negative: in no group)\n"
    "    --max-per-group q  at most q items of one group in a list: the -K items are the first of the user's P best (--pool, default\n"
    "                   min(1024, 10 topk)) that the rule keeps; output as the plain list; stdout gets a \"capped users n exact n\n"
    "                   pool_exhausted n short n kept n\" line; both flags go together and with --allow, not with --candidates,\n"
    "                   --eval, --diversity, --mmr, --tradeoff, --ranks or --fold-in*\n"
    "       omp-pmf-recommend --explain file [--top E] -x data_dir -l lambda [-s 1|2] [--allow items_file] [-K topk] [-u users_file] [--f32] [--scores] model_file output_file\n"
    "    --explain file after the lists: one line per user and list position to `file`, \"user item score support opposition residual\n"
    "                   it1:c1 it2:c2 ...\": the score split into the contributions of the user's own rated items (the --top E largest,\n"
    "                   default 5, 1 .. 16) and a residual that is 0 at a converged row; needs -x (the training ratings), -l (the\n"
    "                   model's lambda) and -K <= 128; -s 1|2 as --fold-in; with the plain list and --allow only: not with --eval,\n"
    "                   --diversity, --mmr, --tradeoff, --ranks, --fold-in*, --groups or --candidates\n"
    "       omp-pmf-recommend --explain-ridge file [--top E] -x data_dir -l lambda [--plain-reg] [--nonneg] [--allow items_file] [-K topk] [-u users_file] [--f32] [--scores] model_file output_file\n"
    "    --explain-ridge file  the same for a squared-loss (CCDR1) model: rating x similarity through the inverse of the user's\n"
    "                   regularised Gram matrix, and the residual to the exact minimiser; output, --top, -x, -l and -K as --explain;\n"
    "                   the regulariser is weighted by the user's rating count, --plain-reg: the plain lambda |u|^2; --nonneg: a\n"
    "                   model trained with -N 1; no -s, no --steps; not with --explain, nor with what --explain is refused with\n";

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

// --allow: one 1-based item id per line (blank lines skipped); allow[j] = 1 for the listed items
static bool read_allow(const char* path, int64_t d2, std::vector<uint8_t>& allow) {
    FILE* fp = fopen(path, "r");
    if (!fp) { fprintf(stderr, "can't open allow file %s\n", path); return false; }
    allow.assign((size_t)d2, 0);
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
        if (end == p || errno || !end || *end != 0) { fprintf(stderr, "allow file %s, line %lld: not an item id\n", path, (long long)ln); ok = false; break; }
        if (v < 1 || v > d2) { fprintf(stderr, "allow file %s, line %lld: item %lld outside 1 .. %lld\n", path, (long long)ln, v, (long long)d2); ok = false; break; }
        allow[(size_t)(v - 1)] = 1;
    }
    fclose(fp);
    return ok;
}

// --candidates: line i = the space-separated 1-based item ids of the i-th requested user (an empty line: an empty row), exactly
// n lines; the rows as a CSR of 0-based ids.  A line may have any length.
static bool read_candidates(const char* path, int64_t n, int64_t d2, std::vector<int64_t>& ptr, std::vector<int32_t>& item) {
    FILE* fp = fopen(path, "r");
    if (!fp) { fprintf(stderr, "can't open candidates file %s\n", path); return false; }
    ptr.assign(1, 0);
    item.reserve(64);                                              // (a file of empty rows still hands the library a pointer)
    char* line = nullptr;
    size_t cap = 0;
    bool ok = true;
    while (ok && getline(&line, &cap, fp) >= 0) {
        const long long ln = (long long)ptr.size();
        const char* p = line;
        while (true) {
            while (*p == ' ' || *p == '\t' || *p == '\r' || *p == '\n') ++p;
            if (*p == 0) break;
            errno = 0;
            char* end = nullptr;
            const long long v = strtoll(p, &end, 10);
            if (end == p || errno || (*end != ' ' && *end != '\t' && *end != '\r' && *end != '\n' && *end != 0)) {
                fprintf(stderr, "candidates file %s, line %lld: not an item id\n", path, ln); ok = false; break;
            }
            if (v < 1 || v > d2) { fprintf(stderr, "candidates file %s, line %lld: item %lld outside 1 .. %lld\n", path, ln, v, (long long)d2); ok = false; break; }
            item.push_back((int32_t)(v - 1));
            p = end;
        }
        ptr.push_back((int64_t)item.size());
    }
    free(line);
    fclose(fp);
    if (ok && (int64_t)ptr.size() - 1 != n) {
        fprintf(stderr, "candidates file %s: %lld lines for %lld requested users\n", path, (long long)ptr.size() - 1, (long long)n);
        ok = false;
    }
    return ok;
}

// "5,10,20": 1 .. PCR_TOPN_MAX_CUTOFFS integers in [1, PCR_RECOMMEND_MAX_K], strictly ascending
static bool parse_cutoffs(const char* v, std::vector<int>& out) {
    const char* p = v;
    while (true) {
        char* end = nullptr;
        errno = 0;
        const long x = strtol(p, &end, 10);
        if (end == p || errno || x < 1 || x > PCR_RECOMMEND_MAX_K || (*end != ',' && *end != 0)) return false;
        if (!out.empty() && x <= out.back()) return false;
        out.push_back((int)x);
        if ((int)out.size() > PCR_TOPN_MAX_CUTOFFS) return false;
        if (*end == 0) return true;
        p = end + 1;
    }
}

// a data directory whose dims must match the model: its CSR `which` (0 training, 1 test); val may be NULL
static bool load_csr(const char* dir, int which, int64_t d1, int64_t d2, std::vector<int64_t>& index, std::vector<int32_t>& item,
                     std::vector<double>* val) {
    pcr_dataset* ds = nullptr;
    if (pcr_dataset_load_mt(dir, 0, &ds) != PCR_OK) { fprintf(stderr, "%s\n", pcr_last_error()); return false; }
    int64_t xd1, xd2, nnz, tnnz;
    pcr_dataset_dims(ds, &xd1, &xd2, &nnz, &tnnz);
    if (xd1 != d1 || xd2 != d2) {
        fprintf(stderr, "data set %s is %lld x %lld, the model %lld x %lld\n", dir, (long long)xd1, (long long)xd2, (long long)d1, (long long)d2);
        pcr_dataset_free(ds);
        return false;
    }
    const int64_t z = which == 0 ? nnz : tnnz;
    index.resize((size_t)d1 + 1);
    std::vector<int64_t> it64((size_t)z);
    if (val) val->resize((size_t)z);
    pcr_dataset_csr(ds, which, index.data(), it64.data(), val ? val->data() : nullptr);
    pcr_dataset_free(ds);
    item.assign(it64.begin(), it64.end());
    return true;
}

// --eval: the metrics per cutoff to stdout, the per-user rows at the largest cutoff to out_path (if given)
static int run_eval(const char* edir, const std::vector<double>& U, const std::vector<double>& V, int64_t d1, int64_t d2, int64_t k,
                    const std::vector<int64_t>* xindex, const std::vector<int32_t>* xitem, const std::vector<int>& cuts, double threshold,
                    bool f32, bool with_ranks, const char* out_path, const char* among, const char* ecfile, long long negatives,
                    unsigned long long seed) {
    std::vector<int64_t> tindex;
    std::vector<int32_t> titem;
    std::vector<double> tval;
    if (!load_csr(edir, 1, d1, d2, tindex, titem, &tval)) return 1;
    std::vector<uint8_t> allow;                                    // --among / --eval-candidates / --negatives: the filter of both calls
    std::vector<int64_t> cptr;
    std::vector<int32_t> citem;
    if (among && !read_allow(among, d2, allow)) return 1;
    if (ecfile && !read_candidates(ecfile, d1, d2, cptr, citem)) return 1;
    citem.reserve(citem.size() + 1);                               // (a file of empty rows still hands the library a pointer)
    if (negatives >= 0) {
        cptr.resize((size_t)d1 + 1);
        const int64_t* xi = xindex ? xindex->data() : nullptr;
        const int32_t* xt = xitem ? xitem->data() : nullptr;
        int rc = pcr_sample_negatives(d1, d2, xi, xt, tindex.data(), titem.data(), 0, negatives, seed, 1, cptr.data(), nullptr);
        if (rc == PCR_OK) {
            citem.resize((size_t)cptr[(size_t)d1] + 1);
            rc = pcr_sample_negatives(d1, d2, xi, xt, tindex.data(), titem.data(), 0, negatives, seed, 1, cptr.data(), citem.data());
        }
        if (rc != PCR_OK) { fprintf(stderr, "evaluate: %s\n", pcr_last_error()); return 1; }
    }
    const bool filtered = among || ecfile || negatives >= 0;
    const pcr_item_filter flt = {among ? allow.data() : nullptr, cptr.empty() ? nullptr : cptr.data(), cptr.empty() ? nullptr : citem.data()};
    const int nc = (int)cuts.size();
    std::vector<pcr_topn_stats> st((size_t)nc);
    std::vector<double> per;
    const bool topn_rows = out_path && !with_ranks;
    if (topn_rows) per.resize((size_t)d1 * nc * 6);
    const int trc = filtered
        ? pcr_evaluate_topn_filtered_model(U.data(), d1, V.data(), d2, k, xindex ? xindex->data() : nullptr, xitem ? xitem->data() : nullptr,
                                           tindex.data(), titem.data(), tval.data(), nc, cuts.data(), threshold, f32 ? PCR_F32 : PCR_F64, &flt,
                                           st.data(), topn_rows ? per.data() : nullptr, 0)
        : pcr_evaluate_topn_model(U.data(), d1, V.data(), d2, k, xindex ? xindex->data() : nullptr, xitem ? xitem->data() : nullptr, tindex.data(),
                                  titem.data(), tval.data(), nc, cuts.data(), threshold, f32 ? PCR_F32 : PCR_F64, st.data(),
                                  topn_rows ? per.data() : nullptr, 0);
    if (trc != PCR_OK) {
        fprintf(stderr, "evaluate: %s\n", pcr_last_error());
        return 1;
    }
    for (const pcr_topn_stats& s : st)
        printf("cutoff %d users %lld users_graded %lld hits %lld precision %g recall %g hit_rate %g map %g ndcg %g ndcg_graded %g\n", s.cutoff,
               (long long)s.users, (long long)s.users_graded, (long long)s.hits, s.precision, s.recall, s.hit_rate, s.map, s.ndcg, s.ndcg_graded);
    if (with_ranks) {
        pcr_rank_stats rs;
        if (out_path) per.resize((size_t)d1 * PCR_RANK_FIELDS);
        const int rrc = filtered
            ? pcr_evaluate_ranks_filtered_model(U.data(), d1, V.data(), d2, k, xindex ? xindex->data() : nullptr, xitem ? xitem->data() : nullptr,
                                                tindex.data(), titem.data(), tval.data(), threshold, f32 ? PCR_F32 : PCR_F64, &flt, &rs,
                                                out_path ? per.data() : nullptr, nullptr, 0)
            : pcr_evaluate_ranks_model(U.data(), d1, V.data(), d2, k, xindex ? xindex->data() : nullptr, xitem ? xitem->data() : nullptr,
                                       tindex.data(), titem.data(), tval.data(), threshold, f32 ? PCR_F32 : PCR_F64, &rs,
                                       out_path ? per.data() : nullptr, nullptr, 0);
        if (rrc != PCR_OK) {
            fprintf(stderr, "evaluate: %s\n", pcr_last_error());
            return 1;
        }
        printf("ranks users %lld users_auc %lld relevant %lld mrr %g mean_rank %g auc %g mpr %g\n", (long long)rs.users, (long long)rs.users_auc,
               (long long)rs.relevant, rs.mrr, rs.mean_rank, rs.auc, rs.mpr);
    }
    if (!out_path) return 0;
    FILE* fp = fopen(out_path, "wb");
    if (!fp) { fprintf(stderr, "can't open output file %s\n", out_path); return 1; }
    bool ok = true;
    for (int64_t u = 0; u < d1 && ok && with_ranks; ++u) {
        const double* r = per.data() + (size_t)u * PCR_RANK_FIELDS;
        if (r[0] != r[0]) continue;                                   // not counted
        ok = fprintf(fp, "%lld %g %g %g %g %g\n", (long long)u + 1, r[0], r[1], r[2], r[3], r[4]) > 0;
    }
    for (int64_t u = 0; u < d1 && ok && !with_ranks; ++u) {
        const double* r = per.data() + ((size_t)u * nc + (nc - 1)) * 6;
        if (r[0] != r[0]) continue;                                   // not counted
        ok = fprintf(fp, "%lld %g %g %g %g %g %g\n", (long long)u + 1, r[0], r[1], r[2], r[3], r[4], r[5]) > 0;
    }
    ok = (fclose(fp) == 0) && ok;
    if (!ok) { fprintf(stderr, "short write to %s\n", out_path); return 1; }
    return 0;
}

// --diversity: one line per cutoff to stdout, the per-user rows at the largest cutoff to out_path (if given)
static int run_diversity(const std::vector<double>& U, const std::vector<double>& V, int64_t d1, int64_t d2, int64_t k,
                         const std::vector<int64_t>* xindex, const std::vector<int32_t>* xitem, const std::vector<int32_t>& users,
                         const std::vector<int>& cuts, bool f32, const char* out_path) {
    const int nc = (int)cuts.size();
    const int64_t n = (int64_t)users.size();
    std::vector<pcr_diversity_stats> st((size_t)nc);
    std::vector<double> per;
    if (out_path) per.resize((size_t)n * nc * PCR_DIVERSITY_FIELDS);
    if (pcr_evaluate_diversity_model(U.data(), d1, V.data(), d2, k, xindex ? xindex->data() : nullptr, xitem ? xitem->data() : nullptr, n,
                                     users.data(), nc, cuts.data(), f32 ? PCR_F32 : PCR_F64, st.data(), out_path ? per.data() : nullptr, nullptr,
                                     0) != PCR_OK) {
        fprintf(stderr, "diversity: %s\n", pcr_last_error());
        return 1;
    }
    for (const pcr_diversity_stats& s : st)
        printf("diversity@%d users %lld users_ild %lld recs %lld items_covered %lld coverage %g gini %g novelty %g ild %g\n", s.cutoff,
               (long long)s.users, (long long)s.users_ild, (long long)s.recs, (long long)s.items_covered, s.coverage, s.gini, s.novelty, s.ild);
    if (!out_path) return 0;
    FILE* fp = fopen(out_path, "wb");
    if (!fp) { fprintf(stderr, "can't open output file %s\n", out_path); return 1; }
    bool ok = true;
    for (int64_t i = 0; i < n && ok; ++i) {
        const double* r = per.data() + ((size_t)i * nc + (nc - 1)) * PCR_DIVERSITY_FIELDS;
        ok = fprintf(fp, "%lld %g %g %g\n", (long long)users[(size_t)i] + 1, r[0], r[1], r[2]) > 0;
    }
    ok = (fclose(fp) == 0) && ok;
    if (!ok) { fprintf(stderr, "short write to %s\n", out_path); return 1; }
    return 0;
}

// "0,0.25,1": 1 .. PCR_RERANK_MAX_THETAS numbers in [0, 1]
static bool parse_thetas(const char* v, std::vector<double>& out) {
    const char* p = v;
    while (true) {
        char* end = nullptr;
        const double x = strtod(p, &end);
        if (end == p || !(x >= 0.0 && x <= 1.0) || (*end != ',' && *end != 0)) return false;
        out.push_back(x);
        if ((int)out.size() > PCR_RERANK_MAX_THETAS) return false;
        if (*end == 0) return true;
        p = end + 1;
    }
}

// --tradeoff: per theta and cutoff the --eval line (edir given) and the --diversity line, each prefixed with "theta <t> "
static int run_tradeoff(const char* edir, const std::vector<double>& U, const std::vector<double>& V, int64_t d1, int64_t d2, int64_t k,
                        const std::vector<int64_t>* xindex, const std::vector<int32_t>* xitem, const std::vector<int32_t>& users,
                        const std::vector<double>& thetas, int pool, const std::vector<int>& cuts, double threshold, bool f32) {
    std::vector<int64_t> tindex;
    std::vector<int32_t> titem;
    std::vector<double> tval;
    if (edir && !load_csr(edir, 1, d1, d2, tindex, titem, &tval)) return 1;
    const int nc = (int)cuts.size(), nt = (int)thetas.size();
    std::vector<pcr_topn_stats> ts((size_t)nt * nc);
    std::vector<pcr_diversity_stats> ds((size_t)nt * nc);
    if (pcr_evaluate_rerank_model(U.data(), d1, V.data(), d2, k, xindex ? xindex->data() : nullptr, xitem ? xitem->data() : nullptr,
                                  edir ? tindex.data() : nullptr, edir ? titem.data() : nullptr, edir ? tval.data() : nullptr,
                                  (int64_t)users.size(), users.data(), nt, thetas.data(), pool, nc, cuts.data(), threshold,
                                  f32 ? PCR_F32 : PCR_F64, edir ? ts.data() : nullptr, ds.data(), nullptr, nullptr, nullptr, 0) != PCR_OK) {
        fprintf(stderr, "tradeoff: %s\n", pcr_last_error());
        return 1;
    }
    for (int t = 0; t < nt; ++t)
        for (int c = 0; c < nc; ++c) {
            const pcr_topn_stats& s = ts[(size_t)t * nc + c];
            const pcr_diversity_stats& d = ds[(size_t)t * nc + c];
            if (edir)
                printf("theta %g cutoff %d users %lld users_graded %lld hits %lld precision %g recall %g hit_rate %g map %g ndcg %g ndcg_graded %g\n",
                       thetas[(size_t)t], s.cutoff, (long long)s.users, (long long)s.users_graded, (long long)s.hits, s.precision, s.recall, s.hit_rate,
                       s.map, s.ndcg, s.ndcg_graded);
            printf("theta %g diversity@%d users %lld users_ild %lld recs %lld items_covered %lld coverage %g gini %g novelty %g ild %g\n",
                   thetas[(size_t)t], d.cutoff, (long long)d.users, (long long)d.users_ild, (long long)d.recs, (long long)d.items_covered, d.coverage,
                   d.gini, d.novelty, d.ild);
        }
    return 0;
}

// --fold-in: the training CSR of a data directory over the model's items (any number of users) and, from it, the new users'
// factors (pcr_fold_in_model); the summary line goes to stdout
// (ridge: pcr_fold_in_ridge_model instead, mu = lambda x count unless plain_reg; its own summary line; nnls: pcr_fold_in_nnls_model,
// likewise)
static bool run_fold_in(const char* dir, const std::vector<double>& V, int64_t d2, int64_t k, double lambda, int solver, int steps, bool f32,
                        bool ridge, bool nnls, bool plain_reg, int64_t* n_out, std::vector<int64_t>& index, std::vector<int32_t>& item, std::vector<double>& U_new,
                        const char* wfile = nullptr, bool conf = false, double alpha = 0.0) {
    pcr_dataset* ds = nullptr;
    if (pcr_dataset_load_mt(dir, 0, &ds) != PCR_OK) { fprintf(stderr, "%s\n", pcr_last_error()); return false; }
    int64_t n, xd2, nnz, tnnz;
    pcr_dataset_dims(ds, &n, &xd2, &nnz, &tnnz);
    if (xd2 != d2) {
        fprintf(stderr, "data set %s has %lld items, the model %lld\n", dir, (long long)xd2, (long long)d2);
        pcr_dataset_free(ds);
        return false;
    }
    index.resize((size_t)n + 1);
    std::vector<int64_t> it64((size_t)nnz);
    std::vector<double> val((size_t)nnz);
    pcr_dataset_csr(ds, 0, index.data(), it64.data(), val.data());
    std::vector<double> rw;                                        // --rating-weights: the weights in the CSR's order
    if (wfile) {
        auto fail = [&](const std::string& why) { fprintf(stderr, "--rating-weights: %s\n", why.c_str()); pcr_dataset_free(ds); return false; };
        int64_t wn = 0, got = 0;
        if (pcr_rating_file_count(wfile, &wn) != PCR_OK) return fail(pcr_last_error());
        std::vector<int32_t> wu((size_t)wn), wi((size_t)wn);
        std::vector<double> wv((size_t)wn);
        if (pcr_rating_file_read(wfile, 0, wn, wu.data(), wi.data(), wv.data(), &got) != PCR_OK) return fail(pcr_last_error());
        if (got != wn) return fail(std::string(wfile) + ": entry " + std::to_string(got + 1) + " is malformed");
        rw.resize((size_t)nnz);
        if (pcr_dataset_match_weights(ds, wn, wu.data(), wi.data(), wv.data(), rw.data()) != PCR_OK) return fail(pcr_last_error());
    }
    pcr_dataset_free(ds);
    item.assign(it64.begin(), it64.end());
    pcr_params p;
    pcr_params_default(&p);
    p.solver_type = solver; p.k = (int)k; p.lambda = lambda; p.precision = f32 ? PCR_F32 : PCR_F64;
    U_new.resize((size_t)n * k);
    if (nnls) {
        pcr_nnls_stats ns;
        if (pcr_fold_in_nnls_model(V.data(), d2, k, lambda, plain_reg ? 0 : 1, p.precision, 0, n, index.data(), item.data(), val.data(), U_new.data(),
                                   &ns, nullptr) != PCR_OK) {
            fprintf(stderr, "fold-in-nnls: %s\n", pcr_last_error());
            return false;
        }
        printf("foldin_nnls users %lld direct %lld cg %lld singular %lld cap %lld pivots %lld zeros %lld loss %g obj %g\n", (long long)ns.users,
               (long long)ns.direct, (long long)ns.cg, (long long)ns.singular, (long long)ns.cap, (long long)ns.pivots, (long long)ns.zeros, ns.loss, ns.obj);
        *n_out = n;
        return true;
    }
    if (conf) {                                                    // --fold-in-ridge with --rating-weights and / or --implicit
        pcr_ridge_stats rs;
        if (pcr_fold_in_conf_model(V.data(), d2, k, lambda, plain_reg ? 0 : 1, alpha, p.precision, 0, n, index.data(), item.data(), val.data(),
                                   wfile ? rw.data() : nullptr, U_new.data(), &rs, nullptr) != PCR_OK) {
            fprintf(stderr, "fold-in-ridge: %s\n", pcr_last_error());
            return false;
        }
        printf("foldin_conf users %lld dual %lld primal %lld cg %lld singular %lld cg_cap %lld iters %lld loss %g obj %g\n", (long long)rs.users,
               (long long)rs.dual, (long long)rs.primal, (long long)rs.cg, (long long)rs.singular, (long long)rs.cg_cap, (long long)rs.iters, rs.loss, rs.obj);
        *n_out = n;
        return true;
    }
    if (ridge) {
        pcr_ridge_stats rs;
        if (pcr_fold_in_ridge_model(V.data(), d2, k, lambda, plain_reg ? 0 : 1, p.precision, 0, n, index.data(), item.data(), val.data(), U_new.data(),
                                    &rs, nullptr) != PCR_OK) {
            fprintf(stderr, "fold-in-ridge: %s\n", pcr_last_error());
            return false;
        }
        printf("foldin_ridge users %lld dual %lld primal %lld cg %lld singular %lld cg_cap %lld iters %lld loss %g obj %g\n", (long long)rs.users,
               (long long)rs.dual, (long long)rs.primal, (long long)rs.cg, (long long)rs.singular, (long long)rs.cg_cap, (long long)rs.iters, rs.loss, rs.obj);
        *n_out = n;
        return true;
    }
    pcr_foldin_stats st;
    if (pcr_fold_in_model(&p, V.data(), d2, n, index.data(), item.data(), val.data(), nullptr, steps, U_new.data(), &st, nullptr) != PCR_OK) {
        fprintf(stderr, "fold-in: %s\n", pcr_last_error());
        return false;
    }
    printf("foldin users %lld converged %lld step_cap %lld stalled %lld steps %lld cg %lld ls %lld obj %g\n", (long long)st.users, (long long)st.converged,
           (long long)st.step_cap, (long long)st.stalled, (long long)st.steps, (long long)st.cg, (long long)st.ls, st.obj);
    *n_out = n;
    return true;
}

// --fold-in-items: the new items' ratings ("user item rating", 1-based) as an item-major CSR over the model's users (file order
// inside an item), the training CSR of xdir, the new rows (pcr_fold_in_items_model) and the extended model file; the summary line
// goes to stdout
static int run_fold_in_items(const char* path, const char* xdir, const char* model, const char* out_model, double lambda, int solver, int steps,
                             bool f32) {
    int64_t d1, d2, k;
    if (pcr_model_load(model, &d1, &d2, &k, nullptr, nullptr) != PCR_OK) { fprintf(stderr, "can't open model file %s\n", model); return 1; }
    std::vector<double> U((size_t)d1 * k), V((size_t)d2 * k);
    if (pcr_model_load(model, &d1, &d2, &k, U.data(), V.data()) != PCR_OK) { fprintf(stderr, "%s\n", pcr_last_error()); return 1; }
    FILE* fp = fopen(path, "r");
    if (!fp) { fprintf(stderr, "can't open ratings file %s\n", path); return 1; }
    std::vector<int32_t> fu, fi;
    std::vector<double> fv;
    int64_t n = 0;
    char line[512];
    for (int64_t ln = 1; fgets(line, sizeof line, fp); ++ln) {
        char* q = line;
        while (*q == ' ' || *q == '\t') ++q;
        if (*q == '\n' || *q == '\r' || !*q) continue;
        char *e1 = nullptr, *e2 = nullptr, *e3 = nullptr;
        const long long u = strtoll(q, &e1, 10);
        const long long it = e1 != q ? strtoll(e1, &e2, 10) : 0;
        const double r = (e2 && e2 != e1) ? strtod(e2, &e3) : 0.0;
        if (e1 == q || !e2 || e2 == e1 || !e3 || e3 == e2) { fprintf(stderr, "%s:%lld: expected \"user item rating\"\n", path, (long long)ln); fclose(fp); return 1; }
        if (u < 1 || u > d1) { fprintf(stderr, "%s:%lld: user %lld is outside 1 .. %lld\n", path, (long long)ln, u, (long long)d1); fclose(fp); return 1; }
        if (it < 1 || it > 2147483000LL) { fprintf(stderr, "%s:%lld: item %lld must be at least 1\n", path, (long long)ln, it); fclose(fp); return 1; }
        if (!std::isfinite(r)) { fprintf(stderr, "%s:%lld: the rating is not finite\n", path, (long long)ln); fclose(fp); return 1; }
        fu.push_back((int32_t)(u - 1)); fi.push_back((int32_t)(it - 1)); fv.push_back(r);
        n = std::max<int64_t>(n, it);
    }
    fclose(fp);
    // the ids number the new items 1 .. n: an id beyond the number of rating lines is a stray line, not n - 1 unrated items
    if (n > (int64_t)fi.size()) {
        fprintf(stderr, "%s: item id %lld exceeds the %lld ratings of the file (the new items are numbered 1 .. n)\n", path, (long long)n, (long long)fi.size());
        return 1;
    }
    std::vector<int64_t> index((size_t)n + 1, 0);
    for (int32_t it : fi) index[(size_t)it + 1] += 1;
    for (int64_t j = 0; j < n; ++j) index[(size_t)j + 1] += index[(size_t)j];
    std::vector<int64_t> at(index.begin(), index.end() - 1);
    std::vector<int32_t> user(fu.size());
    std::vector<double> val(fv.size());
    for (size_t z = 0; z < fu.size(); ++z) { const int64_t o = at[(size_t)fi[z]]++; user[(size_t)o] = fu[z]; val[(size_t)o] = fv[z]; }
    std::vector<int64_t> tindex;
    std::vector<int32_t> titem;
    std::vector<double> tval;
    if (!load_csr(xdir, 0, d1, d2, tindex, titem, &tval)) return 1;
    pcr_params p;
    pcr_params_default(&p);
    p.solver_type = solver; p.k = (int)k; p.lambda = lambda; p.precision = f32 ? PCR_F32 : PCR_F64;
    std::vector<double> Vx((size_t)(d2 + n) * k);
    std::copy(V.begin(), V.end(), Vx.begin());
    pcr_itemfold_stats st;
    if (pcr_fold_in_items_model(&p, U.data(), d1, V.data(), d2, tindex.data(), titem.data(), tval.data(), n, index.data(), user.data(), val.data(), nullptr,
                                steps, Vx.data() + (size_t)d2 * k, &st, nullptr) != PCR_OK) {
        fprintf(stderr, "fold-in-items: %s\n", pcr_last_error());
        return 1;
    }
    if (pcr_model_save(out_model, U.data(), d1, Vx.data(), d2 + n, k) != PCR_OK) { fprintf(stderr, "%s\n", pcr_last_error()); return 1; }
    printf("foldin_items items %lld converged %lld step_cap %lld stalled %lld steps %lld cg %lld ls %lld raters %lld unique_raters %lld obj %g\n",
           (long long)st.items, (long long)st.converged, (long long)st.step_cap, (long long)st.stalled, (long long)st.steps, (long long)st.cg,
           (long long)st.ls, (long long)st.raters, (long long)st.unique_raters, st.obj);
    return 0;
}

// --groups: exactly d2 lines, line j the integer group id of item j (negative: in no group)
static bool read_groups(const char* path, int64_t d2, std::vector<int32_t>& group) {
    FILE* fp = fopen(path, "r");
    if (!fp) { fprintf(stderr, "can't open groups file %s\n", path); return false; }
    group.clear();
    char line[256];
    int64_t ln = 0;
    bool ok = true;
    while (fgets(line, sizeof line, fp)) {
        ++ln;
        char* p = line;
        while (*p == ' ' || *p == '\t') ++p;
        errno = 0;
        char* end = nullptr;
        const long long v = strtoll(p, &end, 10);
        const bool none = end == p;                                // (a blank line is no id)
        while (end && (*end == ' ' || *end == '\t' || *end == '\r' || *end == '\n')) ++end;
        if (none || errno || !end || *end != 0 || v < INT32_MIN || v > INT32_MAX) {
            fprintf(stderr, "groups file %s, line %lld: not a group id\n", path, (long long)ln); ok = false; break;
        }
        if (ln > d2) break;                                        // (reported below)
        group.push_back((int32_t)v);
    }
    fclose(fp);
    if (ok && ln != d2) { fprintf(stderr, "groups file %s: %s than the model's %lld items\n", path, ln > d2 ? "more lines" : "fewer lines", (long long)d2); ok = false; }
    return ok;
}

// --explain: the batch's lists (items [m][K], -1 padding at the end) explained by the users' training rows; one line per user
// and list position to fp
static bool explain_batch(FILE* fp, const std::vector<double>& U, const std::vector<double>& V, int64_t d2, int64_t k,
                          const std::vector<int64_t>& xindex, const std::vector<int32_t>& xitem, const std::vector<double>& xval,
                          const int32_t* users, int64_t m, int K, const std::vector<int32_t>& items, int top, double lambda, int solver, bool f32,
                          bool ridge, bool weighted, bool nonneg) {
    std::vector<int64_t> index((size_t)m + 1, 0);
    for (int64_t i = 0; i < m; ++i) index[(size_t)i + 1] = index[(size_t)i] + (xindex[(size_t)users[i] + 1] - xindex[(size_t)users[i]]);
    std::vector<int32_t> item((size_t)index[(size_t)m]);
    std::vector<double> val((size_t)index[(size_t)m]), Ub((size_t)(m * k));
    for (int64_t i = 0; i < m; ++i) {
        const int64_t a = xindex[(size_t)users[i]], len = index[(size_t)i + 1] - index[(size_t)i];
        std::copy(xitem.begin() + a, xitem.begin() + a + len, item.begin() + index[(size_t)i]);
        std::copy(xval.begin() + a, xval.begin() + a + len, val.begin() + index[(size_t)i]);
        std::copy(U.begin() + (int64_t)users[i] * k, U.begin() + ((int64_t)users[i] + 1) * k, Ub.begin() + i * k);
    }
    pcr_params prm;
    pcr_params_default(&prm);
    prm.k = (int)k; prm.lambda = lambda; prm.solver_type = solver; prm.precision = f32 ? PCR_F32 : PCR_F64;
    std::vector<int32_t> ei((size_t)(m * K * top));
    std::vector<double> ec((size_t)(m * K * top)), pp((size_t)(m * K * PCR_EXPLAIN_PAIR_FIELDS));
    const int rc = ridge ? pcr_explain_ridge_model(V.data(), d2, k, lambda, weighted ? 1 : 0, nonneg ? 1 : 0, prm.precision, 0, m, index.data(), item.data(),
                                                   val.data(), Ub.data(), K, items.data(), top, ei.data(), ec.data(), pp.data(), nullptr, nullptr)
                         : pcr_explain_model(&prm, V.data(), d2, m, index.data(), item.data(), val.data(), Ub.data(), nullptr, K, items.data(), top,
                                             ei.data(), ec.data(), pp.data(), nullptr, nullptr);
    if (rc != PCR_OK) {
        fprintf(stderr, "%s: %s\n", ridge ? "explain-ridge" : "explain", pcr_last_error());
        return false;
    }
    for (int64_t i = 0; i < m; ++i)
        for (int l = 0; l < K; ++l) {
            const int32_t j = items[(size_t)(i * K + l)];
            if (j < 0) break;
            const double* q = pp.data() + (size_t)(i * K + l) * PCR_EXPLAIN_PAIR_FIELDS;
            if (fprintf(fp, "%lld %lld %g %g %g %g ", (long long)users[i] + 1, (long long)j + 1, q[0], q[1], q[2], q[3]) < 0) return false;
            for (int e = 0; e < top; ++e) {
                const size_t z = (size_t)(i * K + l) * top + e;
                if (ei[z] < 0) break;
                if (fprintf(fp, " %lld:%g", (long long)ei[z] + 1, ec[z]) < 0) return false;
            }
            if (fputc('\n', fp) == EOF) return false;
        }
    return true;
}

int main(int argc, char** argv) {
    int K = 10;
    bool f32 = false, with_scores = false, with_ranks = false, diversity = false;
    const char *xdir = nullptr, *ufile = nullptr, *edir = nullptr, *afile = nullptr, *cfile = nullptr, *among = nullptr, *ecfile = nullptr;
    long long negatives = -1;                                      // --negatives (-1: not given)
    unsigned long long seed = 0;
    bool have_seed = false;
    std::vector<int> cuts;
    double threshold = -INFINITY, theta = 0.0;
    bool mmr = false;
    int pool = 0;
    std::vector<double> thetas;                                    // --tradeoff
    std::vector<const char*> pos;
    const char* fdir = nullptr;                                    // --fold-in
    const char* rdir = nullptr;                                    // --fold-in-ridge
    const char* ndir = nullptr;                                    // --fold-in-nnls
    const char* ifile = nullptr;                                   // --fold-in-items
    const char* gfile = nullptr;                                   // --groups
    int max_per_group = 0;                                         // --max-per-group (0: not given)
    bool have_K = false;
    bool plain_reg = false;
    const char* rwfile = nullptr;                                  // --rating-weights (with --fold-in-ridge)
    bool have_implicit = false;                                    // --implicit alpha (with --fold-in-ridge)
    double implicit_alpha = 0.0;
    double lambda = 0.0;
    bool have_lambda = false, have_s = false, have_steps = false;
    int solver = PCR_SOLVER_PCRPP, steps = 10;
    const char* efile = nullptr;                                   // --explain, --explain-ridge
    bool eridge = false, eboth = false, nonneg = false;            // --explain-ridge (eboth: given with --explain), --nonneg
    int top = 0;                                                   // --top (0: not given)
    for (int i = 1; i < argc; ++i) {
        const char* a = argv[i];
        if (!strcmp(a, "--explain") || !strcmp(a, "--explain-ridge")) {
            if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", a); return usage(); }
            const bool r = a[9] != 0;
            if (efile && r != eridge) eboth = true;
            efile = argv[++i];
            eridge = r;
            continue;
        }
        if (!strcmp(a, "--nonneg")) { nonneg = true; continue; }
        if (!strcmp(a, "--top")) {
            if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", a); return usage(); }
            const char* v = argv[++i];
            char* end = nullptr;
            const long x = strtol(v, &end, 10);
            if (!*v || *end || x < 1 || x > PCR_EXPLAIN_MAX_E) { fprintf(stderr, "--top %s: must be an integer in 1 .. %d\n", v, PCR_EXPLAIN_MAX_E); return 1; }
            top = (int)x;
            continue;
        }
        if (!strcmp(a, "--fold-in-ridge")) {
            if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", a); return usage(); }
            rdir = argv[++i];
            continue;
        }
        if (!strcmp(a, "--fold-in-nnls")) {
            if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", a); return usage(); }
            ndir = argv[++i];
            continue;
        }
        if (!strcmp(a, "--fold-in-items")) {
            if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", a); return usage(); }
            ifile = argv[++i];
            continue;
        }
        if (!strcmp(a, "--plain-reg")) { plain_reg = true; continue; }
        if (!strcmp(a, "--rating-weights")) {
            if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", a); return usage(); }
            rwfile = argv[++i];
            continue;
        }
        if (!strcmp(a, "--implicit")) {
            if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", a); return usage(); }
            const char* v = argv[++i];
            char* end = nullptr;
            implicit_alpha = strtod(v, &end);
            if (end == v || *end != '\0' || !(implicit_alpha - implicit_alpha == 0.0) || implicit_alpha < 0.0) {
                fprintf(stderr, "--implicit '%s' is not a finite number >= 0\n", v);
                return 1;
            }
            have_implicit = true;
            continue;
        }
        if (!strcmp(a, "--fold-in") || !strcmp(a, "-l") || !strcmp(a, "-s") || !strcmp(a, "--steps")) {
            if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", a); return usage(); }
            const char* v = argv[++i];
            char* end = nullptr;
            if (!strcmp(a, "--fold-in")) fdir = v;
            else if (a[1] == 'l') {
                lambda = strtod(v, &end);
                if (!*v || *end || !(lambda == lambda) || std::isinf(lambda)) { fprintf(stderr, "-l %s: must be a number\n", v); return 1; }
                have_lambda = true;
            } else if (a[1] == 's') {
                const long x = strtol(v, &end, 10);
                if (!*v || *end || (x != 1 && x != 2)) { fprintf(stderr, "-s %s: must be 1 (PrimalCR) or 2 (PrimalCR++)\n", v); return 1; }
                solver = (int)x; have_s = true;
            } else {
                const long x = strtol(v, &end, 10);
                if (!*v || *end || x < 1 || x > 1000000) { fprintf(stderr, "--steps %s: must be an integer >= 1\n", v); return 1; }
                steps = (int)x; have_steps = true;
            }
            continue;
        }
        if (!strcmp(a, "--eval") || !strcmp(a, "-c") || !strcmp(a, "--threshold")) {
            if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", a); return usage(); }
            const char* v = argv[++i];
            if (a[1] == 'c') {
                cuts.clear();
                if (!parse_cutoffs(v, cuts)) {
                    fprintf(stderr, "-c %s: must be 1 .. %d strictly ascending integers in 1 .. %d, separated by commas\n", v, PCR_TOPN_MAX_CUTOFFS, PCR_RECOMMEND_MAX_K);
                    return 1;
                }
            } else if (a[2] == 'e') edir = v;
            else {
                char* end = nullptr;
                threshold = strtod(v, &end);
                if (!*v || *end || threshold != threshold) { fprintf(stderr, "--threshold %s: must be a number\n", v); return 1; }
            }
        } else if (!strcmp(a, "--mmr")) {
            if (i + 1 >= argc) { fprintf(stderr, "--mmr needs a value\n"); return usage(); }
            const char* v = argv[++i];
            char* end = nullptr;
            theta = strtod(v, &end);
            if (!*v || *end || !(theta >= 0.0 && theta <= 1.0)) { fprintf(stderr, "--mmr %s: must be a number in 0 .. 1\n", v); return 1; }
            mmr = true;
        } else if (!strcmp(a, "--tradeoff")) {
            if (i + 1 >= argc) { fprintf(stderr, "--tradeoff needs a value\n"); return usage(); }
            const char* v = argv[++i];
            thetas.clear();
            if (!parse_thetas(v, thetas)) {
                fprintf(stderr, "--tradeoff %s: must be 1 .. %d numbers in 0 .. 1, separated by commas\n", v, PCR_RERANK_MAX_THETAS);
                return 1;
            }
        } else if (!strcmp(a, "--pool")) {
            if (i + 1 >= argc) { fprintf(stderr, "--pool needs a value\n"); return usage(); }
            const char* v = argv[++i];
            char* end = nullptr;
            const long x = strtol(v, &end, 10);
            if (!*v || *end || x < 1 || x > PCR_RECOMMEND_MAX_K) { fprintf(stderr, "--pool %s: must be an integer in 1 .. %d\n", v, PCR_RECOMMEND_MAX_K); return 1; }
            pool = (int)x;
        } else if (!strcmp(a, "-K") || !strcmp(a, "-x") || !strcmp(a, "-u")) {
            if (i + 1 >= argc) return usage();
            const char* v = argv[++i];
            if (a[1] == 'K') {
                char* end = nullptr;
                const long x = strtol(v, &end, 10);
                if (!*v || *end || x < 1 || x > PCR_RECOMMEND_MAX_K) { fprintf(stderr, "-K %s: must be an integer in 1 .. %d\n", v, PCR_RECOMMEND_MAX_K); return 1; }
                K = (int)x; have_K = true;
            } else if (a[1] == 'x') xdir = v;
            else ufile = v;
        } else if (!strcmp(a, "--allow") || !strcmp(a, "--candidates")) {
            if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", a); return usage(); }
            (a[2] == 'a' ? afile : cfile) = argv[++i];
        } else if (!strcmp(a, "--groups")) {
            if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", a); return usage(); }
            gfile = argv[++i];
        } else if (!strcmp(a, "--max-per-group")) {
            if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", a); return usage(); }
            const char* v = argv[++i];
            char* end = nullptr;
            errno = 0;
            const long x = strtol(v, &end, 10);
            if (!*v || *end || errno || x < 1 || x > INT_MAX) { fprintf(stderr, "--max-per-group %s: must be an integer >= 1\n", v); return 1; }
            max_per_group = (int)x;
        } else if (!strcmp(a, "--among") || !strcmp(a, "--eval-candidates")) {
            if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", a); return usage(); }
            (a[2] == 'a' ? among : ecfile) = argv[++i];
        } else if (!strcmp(a, "--negatives") || !strcmp(a, "--seed")) {
            if (i + 1 >= argc) { fprintf(stderr, "%s needs a value\n", a); return usage(); }
            const char* v = argv[++i];
            char* end = nullptr;
            errno = 0;
            if (a[2] == 'n') {
                negatives = strtoll(v, &end, 10);
                if (!*v || *end || errno || negatives < 0) { fprintf(stderr, "--negatives %s: must be an integer >= 0\n", v); return 1; }
            } else {
                seed = strtoull(v, &end, 10);
                if (!*v || *end || errno || *v == '-') { fprintf(stderr, "--seed %s: must be an integer >= 0\n", v); return 1; }
                have_seed = true;
            }
        } else if (!strcmp(a, "--f32")) f32 = true;
        else if (!strcmp(a, "--scores")) with_scores = true;
        else if (!strcmp(a, "--ranks")) with_ranks = true;
        else if (!strcmp(a, "--diversity")) diversity = true;
        else if (a[0] == '-' && a[1]) { fprintf(stderr, "unknown option %s\n", a); return usage(); }
        else pos.push_back(a);
    }
    const bool tradeoff = !thetas.empty();
    const bool capped = gfile || max_per_group;                    // (the plain list's flow with pcr_recommend_capped_model)
    if (top && !efile) { fprintf(stderr, "--top goes with --explain\n"); return 1; }
    if (eboth) { fprintf(stderr, "--explain-ridge does not go with --explain\n"); return 1; }
    if (nonneg && !eridge) { fprintf(stderr, "--nonneg goes with --explain-ridge\n"); return 1; }
    if (eridge) {                                                  // (--explain's flow with pcr_explain_ridge_model)
        if (edir || diversity || mmr || tradeoff || with_ranks || ifile || fdir || rdir || ndir || capped || cfile) {
            fprintf(stderr, "--explain-ridge does not go with --eval, --diversity, --mmr, --tradeoff, --ranks, --fold-in*, --groups or --candidates\n");
            return 1;
        }
        if (!xdir) { fprintf(stderr, "--explain-ridge needs -x data_dir (the training ratings)\n"); return 1; }
        if (!have_lambda) { fprintf(stderr, "--explain-ridge needs -l lambda\n"); return 1; }
        if (!(lambda > 0.0)) { fprintf(stderr, "-l %g: must be > 0 with --explain-ridge\n", lambda); return 1; }
        if (have_s || have_steps) { fprintf(stderr, "--explain-ridge takes no -s and no --steps\n"); return 1; }
        if (K > PCR_EXPLAIN_MAX_L) { fprintf(stderr, "-K %d: --explain-ridge takes lists of at most %d items\n", K, PCR_EXPLAIN_MAX_L); return 1; }
        if (!top) top = 5;
    } else if (efile) {                                            // (the plain list's flow, then pcr_explain_model on its lists)
        if (edir || diversity || mmr || tradeoff || with_ranks || ifile || fdir || rdir || ndir || capped || cfile) {
            fprintf(stderr, "--explain does not go with --eval, --diversity, --mmr, --tradeoff, --ranks, --fold-in*, --groups or --candidates\n");
            return 1;
        }
        if (!xdir) { fprintf(stderr, "--explain needs -x data_dir (the training ratings)\n"); return 1; }
        if (!have_lambda) { fprintf(stderr, "--explain needs -l lambda\n"); return 1; }
        if (!(lambda > 0.0)) { fprintf(stderr, "-l %g: must be > 0 with --explain\n", lambda); return 1; }
        if (have_steps || plain_reg) { fprintf(stderr, "--explain takes no --steps and no --plain-reg\n"); return 1; }
        if (K > PCR_EXPLAIN_MAX_L) { fprintf(stderr, "-K %d: --explain takes lists of at most %d items\n", K, PCR_EXPLAIN_MAX_L); return 1; }
        if (!top) top = 5;
    }
    if (capped) {
        if (!gfile || !max_per_group) { fprintf(stderr, "--groups and --max-per-group go together\n"); return 1; }
        if (edir || diversity || mmr || tradeoff || with_ranks || ifile || fdir || rdir || ndir || cfile) {
            fprintf(stderr, "--groups and --max-per-group do not go with --eval, --diversity, --mmr, --tradeoff, --ranks, --fold-in* or --candidates\n");
            return 1;
        }
    }
    if (among || ecfile || negatives >= 0 || have_seed) {          // (the filtered evaluation: --eval's flow with a filter)
        if (!edir) { fprintf(stderr, "--among, --eval-candidates, --negatives and --seed go with --eval\n"); return 1; }
        if (ifile || fdir || rdir || ndir || diversity || mmr || tradeoff) {
            fprintf(stderr, "--among, --eval-candidates and --negatives do not go with --fold-in*, --diversity, --mmr or --tradeoff\n");
            return 1;
        }
        if (negatives >= 0 && ecfile) { fprintf(stderr, "--negatives does not go with --eval-candidates\n"); return 1; }
        if (have_seed && negatives < 0) { fprintf(stderr, "--seed goes with --negatives\n"); return 1; }
    }
    if (rwfile || have_implicit) {                                 // (pcr_fold_in_conf_model: the ridge fold-in of a weighted / implicit model)
        const char* mine = rwfile ? "--rating-weights" : "--implicit";
        if (fdir || ndir || ifile) { fprintf(stderr, "%s does not go with --fold-in, --fold-in-nnls or --fold-in-items\n", mine); return 1; }
        if (!rdir) { fprintf(stderr, "%s goes with --fold-in-ridge\n", mine); return 1; }
    }
    if (ifile) {                                                   // (a mode of its own: it writes a model, no lists)
        if (fdir || rdir || ndir) { fprintf(stderr, "--fold-in-items does not go with --fold-in, --fold-in-ridge or --fold-in-nnls\n"); return 1; }
        if (edir || diversity || mmr || tradeoff || with_ranks || afile || cfile) {
            fprintf(stderr, "--fold-in-items does not go with --eval, --diversity, --mmr, --tradeoff, --ranks, --allow or --candidates\n");
            return 1;
        }
        if (have_K || ufile || with_scores || plain_reg || pool || !cuts.empty() || threshold != -INFINITY) {
            fprintf(stderr, "--fold-in-items does not go with -K, -u, -c, --threshold, --pool, --scores or --plain-reg\n");
            return 1;
        }
        if (!xdir) { fprintf(stderr, "--fold-in-items needs -x data_dir (the training ratings)\n"); return 1; }
        if (!have_lambda) { fprintf(stderr, "--fold-in-items needs -l lambda\n"); return 1; }
        if (pos.size() != 2) return usage();
        const int rc = run_fold_in_items(ifile, xdir, pos[0], pos[1], lambda, solver, steps, f32);
        if (rc) return rc;
        fflush(stdout); fflush(stderr);
        _exit(0);
    }
    if (ndir) {                                                    // (--fold-in-ridge's rules under its own name)
        if (rdir) { fprintf(stderr, "--fold-in-nnls does not go with --fold-in-ridge\n"); return 1; }
        if (fdir) { fprintf(stderr, "--fold-in-nnls does not go with --fold-in\n"); return 1; }
        if (afile || cfile) { fprintf(stderr, "--allow and --candidates do not go with --fold-in-nnls\n"); return 1; }
        if (xdir || ufile || diversity || mmr || tradeoff || with_ranks) { fprintf(stderr, "--fold-in-nnls does not go with -x, -u, --diversity, --mmr, --tradeoff or --ranks\n"); return 1; }
        if (have_s || have_steps) { fprintf(stderr, "--fold-in-nnls takes no -s and no --steps\n"); return 1; }
        if (!have_lambda) { fprintf(stderr, "--fold-in-nnls needs -l lambda\n"); return 1; }
        if (lambda < 0.0) { fprintf(stderr, "-l %g: must not be negative with --fold-in-nnls\n", lambda); return 1; }
    } else if (rdir) {                                             // (its own rules; then it follows --fold-in's flow)
        if (fdir) { fprintf(stderr, "--fold-in-ridge does not go with --fold-in\n"); return 1; }
        if (afile || cfile) { fprintf(stderr, "--allow and --candidates do not go with --fold-in-ridge\n"); return 1; }
        if (xdir || ufile || diversity || mmr || tradeoff || with_ranks) { fprintf(stderr, "--fold-in-ridge does not go with -x, -u, --diversity, --mmr, --tradeoff or --ranks\n"); return 1; }
        if (have_s || have_steps) { fprintf(stderr, "--fold-in-ridge takes no -s and no --steps\n"); return 1; }
        if (!have_lambda) { fprintf(stderr, "--fold-in-ridge needs -l lambda\n"); return 1; }
        if (lambda < 0.0) { fprintf(stderr, "-l %g: must not be negative with --fold-in-ridge\n", lambda); return 1; }
    } else if (plain_reg && !efile) { fprintf(stderr, "--plain-reg goes with --fold-in-ridge\n"); return 1; }
    const bool nnls = ndir != nullptr, ridge = rdir != nullptr || nnls;          // (ridge: both take --fold-in-ridge's flow)
    if (ridge) fdir = nnls ? ndir : rdir;
    if ((afile || cfile) && (edir || diversity || mmr || tradeoff || with_ranks || fdir)) {
        fprintf(stderr, "--allow and --candidates do not go with --eval, --diversity, --mmr, --tradeoff, --ranks or --fold-in\n");
        return 1;
    }
    if (fdir) {
        if (!ridge && (xdir || ufile || diversity || mmr || tradeoff || with_ranks)) { fprintf(stderr, "--fold-in does not go with -x, -u, --diversity, --mmr, --tradeoff or --ranks\n"); return 1; }
        if (!have_lambda && !ridge) { fprintf(stderr, "--fold-in needs -l lambda\n"); return 1; }
    } else if (!efile && (have_lambda || have_s || have_steps)) { fprintf(stderr, "-l, -s and --steps go with --fold-in\n"); return 1; }
    if (tradeoff) {                                                // (its own rules; the checks below are the other modes')
        if (mmr || diversity || with_ranks || with_scores) { fprintf(stderr, "--tradeoff does not go with --mmr, --diversity, --ranks or --scores\n"); return 1; }
        if (pos.size() > 1) { fprintf(stderr, "--tradeoff writes no output file\n"); return 1; }
        if (pos.empty()) return usage();
        if (!edir && threshold != -INFINITY) { fprintf(stderr, "--threshold goes with --eval\n"); return 1; }
        if (cuts.empty()) cuts.push_back(K);
        if (!pool) pool = std::min(PCR_RECOMMEND_MAX_K, 10 * cuts.back());
        if (pool < cuts.back()) { fprintf(stderr, "--pool %d: below the largest cutoff %d\n", pool, cuts.back()); return 1; }
    }
    if (diversity && edir) { fprintf(stderr, "--diversity does not go with --eval\n"); return 1; }
    if (mmr && (edir || diversity)) { fprintf(stderr, "--mmr does not go with --eval or --diversity\n"); return 1; }
    if (pool && !mmr && !tradeoff && !capped) { fprintf(stderr, "--pool goes with --mmr\n"); return 1; }
    if (!tradeoff && ((edir || diversity) ? (pos.empty() || pos.size() > 2) : pos.size() != 2)) return usage();
    if (diversity && (with_scores || with_ranks || threshold != -INFINITY)) { fprintf(stderr, "--scores, --ranks and --threshold do not go with --diversity\n"); return 1; }
    if (!edir && !diversity && !tradeoff && (!cuts.empty() || threshold != -INFINITY)) { fprintf(stderr, "-c and --threshold go with --eval\n"); return 1; }
    if (!edir && with_ranks) { fprintf(stderr, "--ranks goes with --eval\n"); return 1; }
    if (mmr || capped) {
        if (!pool) pool = std::min(PCR_RECOMMEND_MAX_K, 10 * K);
        if (pool < K) { fprintf(stderr, "--pool %d: below -K %d\n", pool, K); return 1; }
    }
    if (edir && !tradeoff && (ufile || with_scores)) { fprintf(stderr, "-u and --scores do not go with --eval\n"); return 1; }
    int64_t d1, d2, k;
    if (pcr_model_load(pos[0], &d1, &d2, &k, nullptr, nullptr) != PCR_OK) { fprintf(stderr, "can't open model file %s\n", pos[0]); return 1; }
    std::vector<double> U((size_t)d1 * k), V((size_t)d2 * k);
    if (pcr_model_load(pos[0], &d1, &d2, &k, U.data(), V.data()) != PCR_OK) { fprintf(stderr, "%s\n", pcr_last_error()); return 1; }
    std::vector<int32_t> users;
    if (ufile) { if (!read_users(ufile, d1, users)) return 1; }
    else { users.resize((size_t)d1); for (int64_t u = 0; u < d1; ++u) users[(size_t)u] = (int32_t)u; }
    std::vector<int64_t> xindex;
    std::vector<int32_t> xitem;
    std::vector<double> xval;                                      // --explain: the training ratings' values
    if (xdir && !load_csr(xdir, 0, d1, d2, xindex, xitem, efile ? &xval : nullptr)) return 1;
    std::vector<uint8_t> allow;                                    // --allow / --candidates: the filter of every batch
    std::vector<int64_t> cptr, bptr;
    std::vector<int32_t> citem;
    if (afile && !read_allow(afile, d2, allow)) return 1;
    if (cfile && !read_candidates(cfile, (int64_t)users.size(), d2, cptr, citem)) return 1;
    std::vector<int32_t> group;                                    // --groups
    if (gfile && !read_groups(gfile, d2, group)) return 1;
    if (fdir) {                                                    // the new users take the model's users' place: their factors, their ratings excluded
        std::vector<double> U_new;
        if (!run_fold_in(fdir, V, d2, k, lambda, solver, steps, f32, ridge, nnls, plain_reg, &d1, xindex, xitem, U_new, rwfile, rwfile || have_implicit,
                         implicit_alpha)) return 1;
        U.swap(U_new);
        users.resize((size_t)d1);
        for (int64_t u = 0; u < d1; ++u) users[(size_t)u] = (int32_t)u;
        xdir = fdir;
    }
    if (tradeoff) {
        const int rc = run_tradeoff(edir, U, V, d1, d2, k, xdir ? &xindex : nullptr, xdir ? &xitem : nullptr, users, thetas, pool, cuts, threshold, f32);
        if (rc) return rc;
        fflush(stdout); fflush(stderr);
        _exit(0);
    }
    if (diversity) {
        if (cuts.empty()) cuts.push_back(K);
        const int rc = run_diversity(U, V, d1, d2, k, xdir ? &xindex : nullptr, xdir ? &xitem : nullptr, users, cuts, f32,
                                     pos.size() == 2 ? pos[1] : nullptr);
        if (rc) return rc;
        fflush(stdout); fflush(stderr);
        _exit(0);
    }
    if (edir) {
        if (cuts.empty()) cuts.push_back(K);
        const int rc = run_eval(edir, U, V, d1, d2, k, xdir ? &xindex : nullptr, xdir ? &xitem : nullptr, cuts, threshold, f32,
                                with_ranks, pos.size() == 2 ? pos[1] : nullptr, among, ecfile, negatives, seed);
        if (rc) return rc;
        fflush(stdout); fflush(stderr);
        _exit(0);
    }
    FILE* out_fp = fopen(pos[1], "wb");
    if (!out_fp) { fprintf(stderr, "can't open output file %s\n", pos[1]); return 1; }
    FILE* ex_fp = efile ? fopen(efile, "wb") : nullptr;
    if (efile && !ex_fp) { fprintf(stderr, "can't open explanation file %s\n", efile); fclose(out_fp); return 1; }
    const int64_t n = (int64_t)users.size();
    const int64_t batch = std::max<int64_t>(1, ((int64_t)1 << 22) / K);   // 4 M list entries per call
    std::vector<int32_t> items;
    std::vector<double> scores;
    std::string o;
    bool ok = true;
    pcr_cap_stats cap_all = {0, 0, 0, 0, 0};                       // --groups: the batches' summaries added up
    for (int64_t b0 = 0; b0 < n && ok; b0 += batch) {
        const int64_t m = std::min(batch, n - b0);
        items.resize((size_t)(m * K)); scores.resize((size_t)(m * K));
        const int64_t* xi = xdir ? xindex.data() : nullptr;
        const int32_t* xt = xdir ? xitem.data() : nullptr;
        pcr_item_filter flt = {afile ? allow.data() : nullptr, nullptr, nullptr};
        if (cfile) {                                               // the batch's rows, cand_ptr rebased to its first
            bptr.resize((size_t)m + 1);
            for (int64_t i = 0; i <= m; ++i) bptr[(size_t)i] = cptr[(size_t)(b0 + i)] - cptr[(size_t)b0];
            flt.cand_ptr = bptr.data(); flt.cand_item = citem.data() + cptr[(size_t)b0];
        }
        pcr_cap_stats cst = {0, 0, 0, 0, 0};
        const int rc = capped ? pcr_recommend_capped_model(U.data(), d1, V.data(), d2, k, xi, xt, m, users.data() + b0, K, pool, group.data(),
                                                           max_per_group, f32 ? PCR_F32 : PCR_F64, afile ? &flt : nullptr, items.data(),
                                                           scores.data(), nullptr, &cst, 0)
                     : (afile || cfile) ? pcr_recommend_filtered_model(U.data(), d1, V.data(), d2, k, xi, xt, m, users.data() + b0, K,
                                                                       f32 ? PCR_F32 : PCR_F64, &flt, items.data(), scores.data(), 0)
                     : mmr ? pcr_recommend_diverse_model(U.data(), d1, V.data(), d2, k, xi, xt, m, users.data() + b0, K, pool, theta,
                                                         f32 ? PCR_F32 : PCR_F64, items.data(), scores.data(), 0)
                           : pcr_recommend_model(U.data(), d1, V.data(), d2, k, xi, xt, m, users.data() + b0, K, f32 ? PCR_F32 : PCR_F64,
                                                 items.data(), scores.data(), 0);
        if (rc != PCR_OK) {
            fprintf(stderr, "recommend: %s\n", pcr_last_error());
            fclose(out_fp);
            return 1;
        }
        cap_all.users += cst.users; cap_all.exact += cst.exact; cap_all.exhausted += cst.exhausted;
        cap_all.short_rows += cst.short_rows; cap_all.kept += cst.kept;
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
        if (ex_fp && ok && !explain_batch(ex_fp, U, V, d2, k, xindex, xitem, xval, users.data() + b0, m, K, items, top, lambda, solver, f32, eridge, !plain_reg, nonneg)) {
            fclose(out_fp); fclose(ex_fp);
            return 1;
        }
    }
    ok = (fclose(out_fp) == 0) && ok;
    if (!ok) { fprintf(stderr, "short write to %s\n", pos[1]); return 1; }
    if (ex_fp && fclose(ex_fp) != 0) { fprintf(stderr, "short write to %s\n", efile); return 1; }
    if (capped)
        printf("capped users %lld exact %lld pool_exhausted %lld short %lld kept %lld\n", (long long)cap_all.users, (long long)cap_all.exact,
               (long long)cap_all.exhausted, (long long)cap_all.short_rows, (long long)cap_all.kept);
    fflush(stdout); fflush(stderr);
    _exit(0);
}
