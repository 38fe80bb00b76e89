/*
 * mr_lsqr.h -- device-resident general sparse LSQR (Paige & Saunders) for
 * MI355X (gfx950): min ||A x - b||^2 + damp^2 ||x - x0||^2 on A itself, with
 * SciPy's stopping rules and norm estimates.
 *
 * The reference's SciPy ALS (python/100k_data/ratings_als.py:347-529) runs
 * scipy.sparse.linalg.lsqr on a global design matrix per half-step.  A
 * context here uploads A's structure once (rows ordered by first column, the
 * explicit transpose and the CSR-stream row blocks built on the device, as
 * mr_cg does), takes new values without a re-sort, and solves with three
 * kernels per iteration and no host round trip.  The solver restates
 * scipy/sparse/linalg/_isolve/lsqr.py (1.15) operation for operation;
 * calc_var and show are not offered.
 *
 * Limit: every norm is the sqrt of a plain fp64 sum of squares (no scaling
 * against overflow), so entries beyond ~1e154 overflow where BLAS nrm2 would
 * not.
 */
#ifndef MR_LSQR_H
#define MR_LSQR_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mr_lsqr mr_lsqr;

/* Kernel classes timed with HIP events when timing is enabled. */
enum {
  MR_LSQR_K_A = 0,   /* uh = A v - alfa u, sum uh^2; beta, anorm                   */
  MR_LSQR_K_AT,      /* vh = A^T u - beta v, sum vh^2; alfa, rotations, norms      */
  MR_LSQR_K_X,       /* dk, x, w updates, sum dk^2; ddnorm, stop tests, publish    */
  MR_LSQR_K_SETUP,   /* u = b - A x0, v = A^T u, w = v (per solve)                 */
  MR_LSQR_K_COUNT
};

typedef struct mr_lsqr_result {
  int istop, itn;
  double r1norm, r2norm, anorm, acond, arnorm, xnorm;
} mr_lsqr_result;

typedef struct mr_lsqr_stats {
  int last_iterations;            /* itn of the last solve                        */
  long long iterations_total;     /* over all solves since the last reset         */
  double solve_ms;                /* device time of the solves (setup .. stop)    */
  double kernel_ms[MR_LSQR_K_COUNT];
  long long kernel_launches[MR_LSQR_K_COUNT];  /* launches that did work         */
  long long rows, cols, nnz;
  long long blocks_a, blocks_at;  /* CSR-stream row blocks of A and of A^T        */
  long long block_max_nnz, block_max_rows;
} mr_lsqr_stats;

/* A in CSR form as mr_cg_create takes it: row_indices[rows+1] (int32, from 0,
 * non-decreasing), col_indices / values [row_indices[rows]]; duplicate and
 * unsorted column ids within a row are legal.  NULL on error (mr_last_error). */
mr_lsqr* mr_lsqr_create(int device, int rows, int cols, const int* row_indices,
                        const int* col_indices, const double* values);
void mr_lsqr_destroy(mr_lsqr* ctx);

/* The same structure with new values, given in the caller's CSR order; the
 * device applies the stored row-sort and transpose maps. */
int mr_lsqr_set_values(mr_lsqr* ctx, const double* values);
/* index[nnz], stored once: -1 = the constant 1.0, any other entry (>= 0) an
 * index into the table of a later mr_lsqr_set_values_from_table. */
int mr_lsqr_set_value_map(mr_lsqr* ctx, const int* index);
/* values[j] = index[j] < 0 ? 1.0 : table[index[j]], gathered on the device. */
int mr_lsqr_set_values_from_table(mr_lsqr* ctx, const double* table, long long table_len);

/* scipy.sparse.linalg.lsqr(A, b, damp, atol, btol, conlim, iter_lim, x0=x0):
 * b[rows]; x0_or_null[cols] (NULL: x0 = 0); x_out[cols]; *out as SciPy's
 * istop, itn, r1norm, r2norm, anorm, acond, arnorm, xnorm.  0, or < 0 on
 * error. */
int mr_lsqr_solve(mr_lsqr* ctx, const double* b, const double* x0_or_null, double damp,
                  double atol, double btol, double conlim, int iter_lim, double* x_out,
                  mr_lsqr_result* out);
/* scipy.sparse.linalg.lsmr(A, b, damp, atol, btol, conlim, maxiter, x0=x0) on
 * the same context (values, value map, gather path, timing and stats as
 * mr_lsqr_solve; solves of both kinds may alternate): the solver restates
 * scipy/sparse/linalg/_isolve/lsmr.py (1.15) operation for operation, show
 * is not offered.  KA and KT are LSQR's kernels; KX updates h, hbar and x and
 * sums x^2.  Timings go into the four classes above.  *out as SciPy's istop,
 * itn, normr, normar, norma, conda, normx.  0, or < 0 on error. */
typedef struct mr_lsmr_result {
  int istop, itn;
  double normr, normar, norma, conda, normx;
} mr_lsmr_result;
int mr_lsqr_solve_lsmr(mr_lsqr* ctx, const double* b, const double* x0_or_null, double damp,
                       double atol, double btol, double conlim, int maxiter, double* x_out,
                       mr_lsmr_result* out);
/* *out = sum_i |b_i - (A x)_i|, one pass over A. */
int mr_lsqr_residual_l1(mr_lsqr* ctx, const double* b, const double* x, double* out);

int mr_lsqr_set_timing(mr_lsqr* ctx, int enable);
/* 0 (default): buffer loads while the gathered vector is below 4 GiB; 1:
 * pointer loads at any size (the same bits), as mr_cg_set_gather_path. */
int mr_lsqr_set_gather_path(mr_lsqr* ctx, int mode);
int mr_lsqr_get_stats(mr_lsqr* ctx, mr_lsqr_stats* out);
int mr_lsqr_reset_stats(mr_lsqr* ctx);

/* Truncated SVD of the resident matrix: the k largest singular triplets by a
 * thick-restart Golub-Kahan-Lanczos bidiagonalisation with full
 * re-orthogonalisation (CGS2), fp64, on the context's current values.
 *
 * ncv: size of the Lanczos basis, k < ncv <= min(rows, cols) or ncv == k ==
 * min(rows, cols); 0 = min(min(rows, cols), max(2k + 1, 20)).  tol >= 0: a
 * Ritz pair is converged when its residual estimate is <= tol * sigma_1 (0:
 * 8 ncv eps sigma_1).  maxiter: restarts at most, 0 = 10 min(rows, cols).
 * v0_or_null[cols]: the start vector, in the space of A's COLUMNS whatever
 * the shape (SciPy's ARPACK start vector belongs to the smaller dimension);
 * NULL: a splitmix64 stream from `seed` mapped to (-1, 1), which also
 * supplies the vectors that replace a breakdown.  The same inputs give the
 * same bits.
 *
 * s_out[k] descending; U_out[rows * k] and Vt_out[k * cols] row-major, both
 * NULL when want_vectors == 0.  A singular value the matrix does not have
 * (rank < k, nnz == 0) is returned as 0 with orthonormal vectors.
 * out->converged is 1 when k pairs converged; otherwise the first out->nconv
 * triplets are the converged ones.  out->spmv counts products with A and A^T,
 * out->anorm is the largest Ritz value seen, out->max_residual the largest
 * residual estimate of the k returned pairs; mr_lsqr_svds_residuals returns
 * the last call's k estimates.  The basis buffers, 2 (rows + cols)(ncv + 1)
 * doubles, are allocated by the first call and grown on demand.  A single
 * Lanczos vector finds one vector of a multiple singular value; further
 * copies appear only through rounding.  0, or -1 on error: k or ncv out of
 * range (min(rows, cols) == 0 admits no k), negative tol, non-finite or zero
 * v0. */
typedef struct mr_svds_result {
  int converged, restarts, nconv;
  long long spmv;
  double anorm, max_residual;
} mr_svds_result;
int mr_lsqr_svds(mr_lsqr* ctx, int k, int ncv, double tol, int maxiter,
                 const double* v0_or_null, unsigned long long seed, int want_vectors,
                 double* s_out, double* U_out, double* Vt_out, mr_svds_result* out);
int mr_lsqr_svds_residuals(mr_lsqr* ctx, int k, double* resid_out);

/* Kernel classes of the basis kernels; the SpMVs of an SVD are timed into
 * MR_LSQR_K_A / MR_LSQR_K_AT of mr_lsqr_stats. */
enum {
  MR_SVDS_K_ORTH = 0,   /* basis dot, partial sums, basis update, normalise */
  MR_SVDS_K_COMBINE,    /* basis times a small dense matrix                 */
  MR_SVDS_K_COUNT
};
typedef struct mr_svds_stats {
  double kernel_ms[MR_SVDS_K_COUNT];
  long long kernel_launches[MR_SVDS_K_COUNT];   /* timed intervals            */
  long long steps;          /* Lanczos steps (one A and one A^T product each)  */
  long long orth_bytes;     /* basis bytes the dot and update kernels read     */
  double solve_ms;          /* wall time of the calls                          */
} mr_svds_stats;
int mr_svds_get_stats(mr_lsqr* ctx, mr_svds_stats* out);

/* The basis kernels on host data.  mr_basis_orth: w_inout[n] orthogonalised
 * against the n x j column-major `basis` by classical Gram-Schmidt applied
 * twice; h_out[j] = the sum of both passes' coefficients, *norm_out = |w|
 * after it (w is not normalised; j == 0 leaves w as it is).  mr_basis_combine:
 * out (n x r, column-major) = basis (n x m, column-major) * Y (m x r,
 * row-major).  mr_basis_plan: the dot / update kernels' grid for n rows and
 * the rows one pass of that grid covers. */
int mr_basis_orth(int device, long long n, int j, const double* basis, double* w_inout,
                  double* h_out, double* norm_out);
int mr_basis_combine(int device, long long n, int m, int r, const double* basis,
                     const double* Y, double* out);
int mr_basis_plan(long long n, long long* blocks_out, long long* rows_per_pass_out);

#ifdef __cplusplus
}
#endif
#endif /* MR_LSQR_H */
