/* Content model on the GPU: the reference's per-user tag least-squares
 * recommender ("tag_ls").
 *
 *   model        python/app_local/models.py:342-640 (TagLS_UserProfile),
 *                identical in python/full_data/tag_ls_predictor.py
 *   evaluation   python/full_data/worker_process.py:421-461 (_tag_ls_eval)
 * The Python mirror is movie_recommender_amd/content.py; this header is the
 * C ABI it binds (exported by cpp_ls_lib.so).
 *
 * A feature id is a genre id as is (below 1000) or a tag id + 1000.  A user's
 * model is a profile of at most 25 feature ids -- the most frequent ones in
 * its rating list by (count, id) descending, as many as the list length
 * allows -- and the coefficients x (one per profile id, then a bias) that
 * scipy.sparse.linalg.lsqr returns for A x = rating - median.  The model is
 * LSQR's iterate at ITS stopping test, not the least-squares solution, so
 * the fit runs the Paige & Saunders iteration in fp64 with SciPy's stopping
 * rules in SciPy's order of precedence.  Given x, a score is fp64 in a fixed
 * order: s = 0; s += attr_j * x_j for j = 0 .. p-1 in profile order (separate
 * multiply and add, no FMA); s += x_bias; s += median.
 *
 * All functions return 0 on success and -1 on failure (message via
 * mr_last_error(), declared in mr_als.h).  Buffers are caller-owned host
 * memory; nothing is retained after a call returns.
 */
#ifndef MR_CONTENT_H
#define MR_CONTENT_H

#ifdef __cplusplus
extern "C" {
#endif

#define MR_CONTENT_MAX_FACTORS 25                      /* profile ids per user */
#define MR_CONTENT_ROW (MR_CONTENT_MAX_FACTORS + 1)    /* x row: coefficients, bias */

typedef struct mr_content mr_content;

/* Feature table on device `device`.  Candidates are the movies with a median,
 * in movie_medians iteration order: cand_mid[c] = movie id (unique, >= 0),
 * cand_med[c] = median.  Candidate c's features are entries feat_off[c] ..
 * feat_off[c+1]-1 of (feat_id, feat_val), ids strictly increasing inside a
 * candidate and >= 0: a genre with value 1.0, a tag as tag id + 1000 with
 * value movie_tags[m][t] / tag_counts[t].  The device keeps this per-movie
 * layout only (plus each entry's number among the distinct ids, for the
 * profile counts): scoring looks a movie's features up in the user's
 * profile, so no transposed, per-feature layout is built. */
mr_content* mr_content_create(int device, int n_cand, const int* cand_mid,
                              const double* cand_med, const long long* feat_off,
                              const int* feat_id, const double* feat_val);
void mr_content_destroy(mr_content* ctx);
int mr_content_num_candidates(const mr_content* ctx);

/* Fit of n_users rating lists: user u's ratings are off[u] .. off[u+1]-1
 * (at least 2), each a candidate index and the RAW rating.  iter_lim_each
 * (optional, int[n_users]) overrides iter_lim per user.
 *   p_out        int[n_users]              profile length
 *   profile_out  int[n_users * 25]         feature ids (-1 past p)
 *   x_out        f64[n_users * 26]         x[0 .. p-1], bias at x[p], 0 past it
 *   itn_out, istop_out  int[n_users]       LSQR's iteration count and stop code
 * The same list gives the same bits alone or in any batch. */
int mr_content_fit(mr_content* ctx, int n_users, const long long* off, const int* cand,
                   const double* ratings, double atol, double btol, double conlim, int iter_lim,
                   const int* iter_lim_each, int* p_out, int* profile_out, double* x_out,
                   int* itn_out, int* istop_out);

/* Scores of every candidate for n_users models (p, profile, x as mr_content_fit
 * writes them; the p ids of a profile distinct and >= 0): out[u * n_cand + c]. */
int mr_content_scores(mr_content* ctx, int n_users, const int* p, const int* profile,
                      const double* x, double* out);

/* Top-N as mr_rec_top_n (include/mr_serving.h), on these scores. */
int mr_content_top_n(mr_content* ctx, int n_users, const int* p, const int* profile,
                     const double* x, const long long* excl_off, const int* excl_cand,
                     int num_results, int* out_mid, double* out_score, int* out_count);

/* Evaluation as mr_rec_evaluate: test user t is scored with model t on its
 * test ratings off[t] .. off[t+1]-1 (cand[i] = candidate index, -1 when the
 * movie has no median; actual[i] = held-out rating).  pred, sse, n_pred are
 * optional. */
int mr_content_evaluate(mr_content* ctx, int n_test, const int* p, const int* profile,
                        const double* x, const long long* off, const int* cand,
                        const double* actual, double* agreement, long long* n_agree,
                        long long* n_disagree, double* pred, double* sse, long long* n_pred);

/* Kernel time of the last call, milliseconds, per class: [0] profile,
 * [1] LSQR fit, [2] scores, [3] exclusion, [4] top-N select, [5] evaluation. */
int mr_content_last_kernel_ms(const mr_content* ctx, double* ms6);

#ifdef __cplusplus
}
#endif
#endif
