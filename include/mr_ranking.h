/* Ranking evaluation and new-user fold-in for implicit-feedback models
 * (DESIGN.md "Ranking evaluation and implicit fold-in").  Exported by
 * cpp_ls_lib.so; the Python face is movie_recommender_amd/ranking.py and
 * movie_recommender_amd/implicit.py.
 *
 * Both entry points are handle-free: buffers are caller-owned host memory and
 * nothing is retained after a call returns.  They return 0 on success and -1
 * on failure (message via mr_last_error(), declared in mr_als.h).  A refused
 * call touches no output and leaves the library usable.
 */
#ifndef MR_RANKING_H
#define MR_RANKING_H

#ifdef __cplusplus
extern "C" {
#endif

/* Rank counts of held-out (user, item) pairs among all items the user has
 * not seen, without ever storing the n_users x n_items scores.
 *
 * Score:  s(u, i) = ((sum_{j=0..k-1} x_uj * y_ij) + b_u) + m_i, the sum from
 * 0.0 in index order, every product and every addition rounded on its own (no
 * FMA) -- the arithmetic of mr_rec_scores, so the bits are the same.  NULL
 * user_bias / item_offset stand for 0.0 (which is still added).
 *
 * Test pairs and exclusions are CSR by user: user u owns entries
 * off[u] .. off[u+1]-1.  excl_off may be NULL (nothing excluded).  With
 * E_u = all items except excl(u), for test pair p = (u, i), i in E_u:
 *   above[p]        = #{ j in E_u, j != i : s(u, j) >  s(u, i) }
 *   tied[p]         = #{ j in E_u, j != i : s(u, j) == s(u, i) }  (-0.0 == +0.0)
 *   tied_before[p]  = #{ tied j : j > i }
 *   score[p]        = s(u, i)                        (optional, may be NULL)
 *   n_eligible[u]   = |E_u|
 * above + tied_before is the 0-based position of i in the (score, id)
 * descending list of mr_rec_top_n.  All counts are integers summed with
 * integer atomics: two calls return the same bits.
 *
 * Refused (-1): k outside 1 .. 512, offsets that do not start at 0 or
 * decrease, an item id outside 0 .. n_items-1, a duplicate inside one user's
 * exclusion list, a test item that its user also excludes.
 *
 * kernel_ms (optional): double[3], HIP-event milliseconds of this call per
 * kernel class: [0] pair scores (the thresholds and the excluded items'
 * scores), [1] the tile count kernel, [2] the exclusion subtraction. */
int mr_rank_counts(int device, int k, int n_users, int n_items,
                   const double* X, const double* user_bias,
                   const double* Y, const double* item_offset,
                   const long long* test_off, const int* test_item,
                   const long long* excl_off, const int* excl_item,
                   int* above, int* tied, int* tied_before,
                   double* score, int* n_eligible, double* kernel_ms);

/* Work division of mr_rank_counts, process-wide (tests and measurements; 0
 * restores a default): users per launch (rounded up to a multiple of 32),
 * item-tile groups per user tile (grid.y of the count kernel; each block
 * walks the item tiles of its group), and the pair slots per 32-user tile
 * that the sorted-threshold path keeps in LDS (0 .. 2048; users whose pairs
 * lie past them take the compare path, which has no limit; a negative value
 * means 0 slots).  The counts do not depend on any of them.  Returns -1 for
 * values out of range. */
int mr_rank_set_tuning(int user_chunk, int item_groups, int lds_pairs);

/* Implicit-feedback fold-in (Hu, Koren, Volinsky): the user half-step of
 * mr_als_set_implicit for users that were not in the training set.  User u's
 * list is item[off[u] .. off[u+1]-1] with strengths r >= 0.  In fp64, with
 * S = Y^T Y (fixed summation order) and w = alpha * r:
 *   G_u = S + sum w y y^T + lambda_u I,   c_u = sum (1 + w) y,
 *   lambda_u = reg (MR_REG_CONSTANT) or reg * (length of the list)
 *   (MR_REG_WEIGHTED);  x_u = Cholesky solve of G_u x = c_u.
 * x_out: f64[n_users * k].  status (optional): 1 solved, 0 a pivot was not
 * positive (possible only with reg = 0) and the row is all zero.  An empty
 * list gives exactly the zero row with status 1.  mr_fold_in (mr_foldin.h) is
 * the general form -- new items, explicit models, non-negative factors -- and
 * returns these bits with MR_FOLD_IMPLICIT and nonneg = 0.
 *
 * Refused (-1): k outside 1 .. 128, an id out of range, an r that is negative
 * or not finite, a negative or non-finite alpha or reg, an unknown reg_mode,
 * offsets that do not start at 0 or decrease. */
int mr_implicit_fold_in(int device, int k, int n_items, const double* Y,
                        double alpha, double reg, int reg_mode,
                        int n_users, const long long* off, const int* item, const double* r,
                        double* x_out, int* status);

#ifdef __cplusplus
}
#endif
#endif
