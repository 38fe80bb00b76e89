/* Content model on the GPU: the reference's per-user tag-count recommender
 * ("tag_count").
 *
 *   model        python/app_local/models.py:24-336 (TagCount_UserProfile),
 *                identical in python/full_data/tag_count_predictor.py:6-239
 *   evaluation   python/full_data/worker_process.py:231-258 (_test_model),
 *                :344-372 (_median_eval), :376-418 (_tag_count_eval)
 * The Python mirror is movie_recommender_amd/tagcount.py; this header is the
 * C ABI it binds (exported by cpp_ls_lib.so).
 *
 * A user's model is a sparse tag profile (one value per tag of every rated
 * movie), a genre profile, and up to two small linear models:
 *   profiles   offset = rating - 3; for every tag t of the movie, in the
 *              movie's stored order, tag_profile[t] += offset * value (separate
 *              multiply and add, from 0); genre_profile[g] += offset; at the
 *              end each entry is divided by its tag / genre count.  A rating
 *              with offset 0 contributes nothing.
 *   rows       per rating: b = rating - median, tag_dot = sum profile[t] *
 *              value over the movie's tags in stored order, genre_dot = sum
 *              genre_profile[g] over the movie's genres in stored order.
 *              A1 gets [genre_dot, 1] from every rating, A0 gets [tag_dot,
 *              genre_dot, 1] from the ratings with tag_dot > 0.1.
 *   fit        x0 = minimum-norm least-squares solution of A0 x = b0 when A0
 *              has >= 3 rows, x1 of A1 x = b1 with >= 2 rows: Householder QR
 *              of [A | b], then the SVD of R; singular values <= eps *
 *              max(rows, cols) * s_max count as zero.
 *   score      tag_product / genre_product as tag_dot / genre_dot.  Model 0
 *              unless tag_product < 1e-6 or there is no x0:
 *                s = 0; s += tag_product * x0[0]; s += genre_product * x0[1];
 *                s += x0[2]; s += median
 *              else model 1 if there is an x1:
 *                s = 0; s += genre_product * x1[0]; s += x1[1]; s += median
 *              else s = median.
 * Every product and sum of the profiles, the dot products and the scores is
 * a separately rounded fp64 operation in exactly this order (no FMA); the
 * divisions are correctly rounded.  So profiles, dot products, the rows of
 * A0 and the choice of model are bit-equal to the reference's Python.
 *
 * All functions return 0 on success and -1 on failure (message via
 * mr_last_error(), declared in mr_als.h).  Buffers are caller-owned host
 * memory; nothing is retained after a call returns.
 */
#ifndef MR_TAGCOUNT_H
#define MR_TAGCOUNT_H

#ifdef __cplusplus
extern "C" {
#endif

#define MR_TAGCOUNT_MAX_GENRES 1024   /* distinct genres of a table (profile in LDS) */

typedef struct mr_tagcount mr_tagcount;

/* Table on device `device`.  Candidates are the movies with a median, in
 * movie_medians iteration order: cand_mid[c] = movie id (unique, >= 0),
 * cand_med[c] = median.  Candidate c's genres are entries genre_off[c] ..
 * genre_off[c+1]-1 of genre_idx (index into the table's n_genres distinct
 * genres, in the reference's list(set) order), its tags entries tag_off[c] ..
 * tag_off[c+1]-1 of (tag_idx, tag_val): index into the n_tags distinct tags
 * and the RAW movie_tags[m][t], in movie_tags[m] iteration order.  Indices are
 * distinct inside a candidate.  genre_count[n_genres] / tag_count[n_tags] are
 * the counts as fp64, positive and below 2^53. */
mr_tagcount* mr_tagcount_create(int device, int n_cand, const int* cand_mid,
                                const double* cand_med, const long long* genre_off,
                                const int* genre_idx, const long long* tag_off,
                                const int* tag_idx, const double* tag_val, int n_genres,
                                const double* genre_count, int n_tags, const double* tag_count);
void mr_tagcount_destroy(mr_tagcount* ctx);
int mr_tagcount_num_candidates(const mr_tagcount* ctx);

/* Fit of n_users rating lists: user u's ratings are off[u] .. off[u+1]-1 (any
 * number, 0 included), each a candidate index and the RAW rating.
 *   genre_profile  f64[n_users * n_genres]
 *   tp_off         i64[n_users + 1]   CSR of the tag profiles: user u's entries
 *   tp_idx, tp_val [tp_cap]           tp_off[u] .. tp_off[u+1]-1, tag index
 *                                     ascending, the values that are not 0
 *   x0  f64[n_users * 3], x1  f64[n_users * 2]   zeros without a model
 *   has0, has1     int[n_users]       1 when x0 / x1 exists
 *   n0             int[n_users]       rows of A0
 *   rank0, rank1   int[n_users]       effective rank (0 without a model)
 * tp_cap: entries tp_idx / tp_val hold; the sum of the tag counts of the rated
 * movies always suffices.  The same list gives the same bits alone or in any
 * batch. */
int mr_tagcount_fit(mr_tagcount* ctx, int n_users, const long long* off, const int* cand,
                    const double* ratings, double* genre_profile, long long* tp_off,
                    int* tp_idx, double* tp_val, long long tp_cap, double* x0, double* x1,
                    int* has0, int* has1, int* n0, int* rank0, int* rank1);

/* Scores of every candidate for n_users models (the arrays mr_tagcount_fit
 * writes; tag indices strictly ascending inside a user): out[u * n_cand + c]. */
int mr_tagcount_scores(mr_tagcount* ctx, int n_users, const double* genre_profile,
                       const long long* tp_off, const int* tp_idx, const double* tp_val,
                       const double* x0, const double* x1, const int* has0, const int* has1,
                       double* out);

/* Top-N as mr_rec_top_n (include/mr_serving.h), on these scores. */
int mr_tagcount_top_n(mr_tagcount* ctx, int n_users, const double* genre_profile,
                      const long long* tp_off, const int* tp_idx, const double* tp_val,
                      const double* x0, const double* x1, const int* has0, const int* has1,
                      const long long* excl_off, const int* excl_cand, int num_results,
                      int* out_mid, double* out_score, int* out_count);

/* Evaluation as mr_rec_evaluate: test user t is scored with model t on its
 * test ratings off[t] .. off[t+1]-1 (cand[i] = candidate index, -1 when the
 * movie has no median: no prediction; actual[i] = held-out rating).  pred,
 * sse, n_pred are optional. */
int mr_tagcount_evaluate(mr_tagcount* ctx, int n_test, const double* genre_profile,
                         const long long* tp_off, const int* tp_idx, const double* tp_val,
                         const double* x0, const double* x1, const int* has0, const int* has1,
                         const long long* off, const int* cand, const double* actual,
                         double* agreement, long long* n_agree, long long* n_disagree,
                         double* pred, double* sse, long long* n_pred);

/* Kernel time of the last call, milliseconds, per class: [0] profiles,
 * [1] rows and fit, [2] profile compaction, [3] profile scatter, [4] scores,
 * [5] exclusion, [6] top-N select, [7] evaluation. */
int mr_tagcount_last_kernel_ms(const mr_tagcount* ctx, double* ms8);

#ifdef __cplusplus
}
#endif
#endif
