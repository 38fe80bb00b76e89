/* Fold-in for every trained model (DESIGN.md "Fold-in"): factors of entities
 * that were not in the training set -- new users or new items -- from the
 * opposite factor table, for explicit (ALS-WR, ridge) and implicit-feedback
 * models, unconstrained or non-negative.  Exported by cpp_ls_lib.so; the
 * Python face is movie_recommender_amd/foldin.py.
 *
 * The entry point is handle-free: buffers are caller-owned host memory and
 * nothing is retained after a call returns.  It returns 0 on success and -1
 * on failure (message via mr_last_error(), declared in mr_als.h).  A refused
 * call writes no output and leaves the library usable.
 */
#ifndef MR_FOLDIN_H
#define MR_FOLDIN_H

#ifdef __cplusplus
extern "C" {
#endif

enum { MR_FOLD_EXPLICIT = 0, MR_FOLD_IMPLICIT = 1 };

/* Everything is fp64.  Entity e's list is idx / r[off[e] .. off[e+1]-1] with
 * M entries; a_j = row idx_j of T (k numbers), K = k + intercept.
 *
 * MR_FOLD_EXPLICIT:  G = sum [a_j, 1][a_j, 1]^T,
 *                    c = sum (r_j - row_offset[idx_j]) [a_j, 1]
 *   (the 1 only with intercept; a NULL row_offset subtracts nothing).  With
 *   T = V, intercept = 1 and median-subtracted r this is the engine's user
 *   half-step; with T = U[:, :k], row_offset = U[:, k] and intercept = 0 its
 *   item half-step.
 * MR_FOLD_IMPLICIT:  G = T^T T + sum w a a^T,  c = sum (1 + w) a,  w = alpha r
 *   (intercept and row_offset are refused).
 * Ridge: lambda_e = reg (MR_REG_CONSTANT) or reg * M (MR_REG_WEIGHTED), added
 *   to the first k diagonal entries; the intercept is never penalised.
 *
 * nonneg = 0: Cholesky solve of G x = c.  With MR_FOLD_IMPLICIT the result is
 *   bit-identical to mr_implicit_fold_in.
 * nonneg = 1: minimise 1/2 x^T G x - c^T x with x_j >= 0 for j < k by block
 *   principal pivoting with the backup rule, from the empty free set (the rule
 *   of mr_als_set_nnls without a warm start).  The intercept is always free
 *   and never a pivot candidate.  Coordinates held at zero are stored as +0.
 *   At most max_rounds rounds, 4 (k + 1) when max_rounds is 0.
 *
 * x_out: f64[n_new * K].  status (optional): 1 solved / converged; 0 a
 * diagonal entry or a pivot was <= 0 and the whole row is zero; -1 the
 * non-negative solve stopped at the round cap and the last x is stored,
 * clamped at 0 on the constrained coordinates.  rounds (optional): rounds of
 * the non-negative solve; 1 for a Cholesky solve, 0 with status 0.  An empty
 * list gives the zero row with status 1 and rounds 0.
 *
 * Refused (-1): k outside 1 .. 128, intercept or row_offset with
 * MR_FOLD_IMPLICIT, an unknown mode or reg_mode, a negative or non-finite
 * alpha, reg or max_rounds, an id out of range, a non-finite r or a negative
 * r with MR_FOLD_IMPLICIT, a non-finite entry of T or row_offset, offsets
 * that do not start at 0 or decrease. */
int mr_fold_in(int device, int k, int n_rows, const double* T,
               const double* row_offset, int mode, int intercept,
               double alpha, double reg, int reg_mode, int nonneg, int max_rounds,
               int n_new, const long long* off, const int* idx, const double* r,
               double* x_out, int* status, int* rounds);

#ifdef __cplusplus
}
#endif
#endif
