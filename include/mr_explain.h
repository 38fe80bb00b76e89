/* Explanations (DESIGN.md "Explanations"): how the score of a target row
 * splits over the entries of an entity's own list, for every model whose
 * half-step is a linear solve.  Exported by cpp_ls_lib.so; the Python face is
 * movie_recommender_amd/foldin.py (explain, explain_users, explain_items).
 *
 * The entry point is handle-free like mr_fold_in: buffers are caller-owned
 * host memory and nothing is retained after a call returns.  It returns 0 on
 * success and -1 on failure (message via mr_last_error(), declared in
 * mr_als.h).  A refused call writes no output and leaves the library usable.
 */
#ifndef MR_EXPLAIN_H
#define MR_EXPLAIN_H

#include "mr_foldin.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The entity's system is mr_fold_in's (mr_foldin.h) with nonneg = 0: G x = c,
 * c = sum_j coef_j A_j, where A_j = [a_j, 1] with the intercept and a_j
 * otherwise, and coef_j = r_j - row_offset[idx_j] (MR_FOLD_EXPLICIT) or
 * 1 + alpha r_j (MR_FOLD_IMPLICIT).  So for a target row t of the same T
 *
 *     s_t = A_t . x = sum_j phi[t][j],   phi[t][j] = coef_j (A_t^T G^-1 A_j),
 *
 * exactly: phi[t][j] is what list entry j contributes to the score of t.
 *
 * Targets are a CSR by entity: entity e asks about rows tidx[toff[e] ..
 * toff[e+1]-1] (Q_e of them; 0 is legal, duplicates are legal and give the
 * same bits).  M_e is the length of its list.
 *
 * Outputs, each may be NULL, but phi or one of top_pos / top_val / top_cnt
 * must be given:
 *   x_out  f64[n_ent * K], status int[n_ent]: the bits and values mr_fold_in
 *          returns for the same inputs with nonneg = 0.
 *   score  f64[toff[n_ent]]: s_t = A_t . x summed in index order.
 *          row_offset[t] is NOT added: the caller adds medians or offsets, as
 *          it does to the scores of a folded-in row.
 *   phi    entity e owns Q_e * M_e doubles at phi + poff[e], row-major [q][j],
 *          j the position in the entity's list.  poff is int64[n_ent + 1] and
 *          must be the running sum of Q_e * M_e from 0; required with phi.
 *   top_pos int[toff[n_ent] * top], top_val f64[toff[n_ent] * top], top_cnt
 *          int[toff[n_ent]]: per target the top_cnt = min(top, M_e) largest
 *          contributions, descending by value, equal values (-0.0 == +0.0) by
 *          smaller position first; position = j in the entity's list.  Unused
 *          slots hold position -1 and value 0.  The values are the ones the
 *          same call writes to phi, bit for bit.
 *
 * Status 0 (a pivot was not positive): scores, phi and top values are zero
 * and top_cnt = 0.  An empty list: status 1, score 0, top_cnt = 0.
 *
 * Refused (-1): everything mr_fold_in refuses; top outside 0 .. 64; a target
 * id out of range; target offsets that do not start at 0 or that decrease; no
 * requested output; a poff that is not the running sum; one entity whose own
 * Q_e * M_e doubles exceed 256 MiB (entities go to the device in chunks whose
 * phi blocks stay below that; results do not depend on the chunking). */
int mr_explain(int device, int k, int n_rows, const double* T,
               const double* row_offset, int mode, int intercept,
               double alpha, double reg, int reg_mode,
               int n_ent, const long long* off, const int* idx, const double* r,
               const long long* toff, const int* tidx, int top,
               double* x_out, int* status, double* score,
               const long long* poff, double* phi,
               int* top_pos, double* top_val, int* top_cnt);

#ifdef __cplusplus
}
#endif
#endif
