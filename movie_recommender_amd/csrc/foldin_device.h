// The per-entity normal equations and their Cholesky solve, shared by the
// fold-in (foldin.hip K-FI1 / K-FI2) and the explanations (explain.hip K-EX):
// one body, so the factors of both entry points are the same bits.  Plus the
// host-side validation both entry points start with.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../../include/mr_als.h"
#include "../../include/mr_foldin.h"
#include "mr_internal.h"

namespace mr {

__device__ __forceinline__ double fi_mul(double a, double b) {   // a product rounded on its own
#pragma clang fp contract(off)
  return a * b;
}

constexpr int FI_NE = 9;

// G = (S +) sum weight [a,1][a,1]^T + lambda I_k into G[K][K+1], c into its
// column K, for the list idx / r[b .. b + M - 1] (M > 0).  Rows [a | 1 | weight
// | rhs coefficient] are staged rows_per_stage at a time in As (the 1 only with
// an intercept; weight = 1 or w = alpha r; rhs coefficient = r - offset or
// 1 + w).  Each thread owns FI_NE entries of the upper triangle in registers
// (row order, several passes when K (K + 1) / 2 > 256 FI_NE), threads 0 .. K-1
// also one entry of c.  G is LDS or global memory; As is LDS.  The caller puts
// a barrier between this and the first read of G by another thread.
__device__ __forceinline__ void fi_build(int k, int icpt, int implicit, int rows_per_stage,
                                         double alpha, double lam, int64_t b, int M,
                                         const int* __restrict__ idx,
                                         const double* __restrict__ r,
                                         const double* __restrict__ T,
                                         const double* __restrict__ roff,
                                         const double* __restrict__ S, double* G, double* As) {
  const int K = k + icpt;
  const int W = K + 1;    // row width of G: K coordinates, then the rhs
  const int WS = K + 2;   // row width of the stage: K coordinates, weight, rhs coefficient
  const int tid = threadIdx.x;
  const int NT = K * (K + 1) / 2;
  for (int g0 = 0; g0 < NT; g0 += 256 * FI_NE) {
    const bool rhs_pass = g0 == 0;
    int ei[FI_NE], ej[FI_NE];
    double acc[FI_NE], cacc = 0.0;
#pragma unroll
    for (int t = 0; t < FI_NE; ++t) {
      int f = g0 + tid + 256 * t;
      acc[t] = 0.0;
      ei[t] = -1;
      ej[t] = -1;
      if (f < NT) {
        int i = 0, len = K;
        while (f >= len) {
          f -= len;
          ++i;
          --len;
        }
        ei[t] = i;
        ej[t] = i + f;
      }
    }
    for (int r0 = 0; r0 < M; r0 += rows_per_stage) {
      const int nr = min(rows_per_stage, M - r0);
      for (int q = tid; q < nr * WS; q += 256) {
        const int row = q / WS, j = q % WS;
        const int64_t p = b + r0 + row;
        const int id = idx[p];
        double v;
        if (j < k) {
          v = T[(int64_t)id * k + j];
        } else if (j < K) {
          v = 1.0;
        } else if (implicit) {
          const double w = fi_mul(alpha, r[p]);
          v = j == K ? w : 1.0 + w;
        } else {
          v = j == K ? 1.0 : (roff ? r[p] - roff[id] : r[p]);
        }
        As[row * WS + j] = v;
      }
      __syncthreads();
#pragma unroll
      for (int t = 0; t < FI_NE; ++t) {
        if (ei[t] < 0) continue;
        double s = acc[t];
        for (int row = 0; row < nr; ++row)
          s = fma(As[row * WS + K] * As[row * WS + ei[t]], As[row * WS + ej[t]], s);
        acc[t] = s;
      }
      if (rhs_pass && tid < K)
        for (int row = 0; row < nr; ++row)
          cacc = fma(As[row * WS + K + 1], As[row * WS + tid], cacc);
      __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < FI_NE; ++t) {
      if (ei[t] < 0) continue;
      double g = acc[t];
      if (implicit) g = S[ei[t] * k + ej[t]] + acc[t];
      if (ei[t] == ej[t] && ei[t] < k) g += lam;
      G[ei[t] * W + ej[t]] = g;
      G[ej[t] * W + ei[t]] = g;
    }
    if (rhs_pass && tid < K) G[tid * W + K] = cacc;
  }
}

// In-place Cholesky of G[K][K+1] in LDS (L in the lower triangle), then
// L y = c (right-looking) and L^T x = y on column K.  Returns true, to every
// thread of the block, when a pivot was not positive (G is then half-factored
// and column K is not a solution).  s_bad is one int of LDS.
__device__ __forceinline__ bool fi_cholesky_solve(int K, double* G, int* s_bad) {
  const int W = K + 1, tid = threadIdx.x;
  if (tid == 0) *s_bad = 0;
  __syncthreads();
  for (int j = 0; j < K; ++j) {
    if (tid == 0) {
      const double d = G[j * W + j];
      if (!(d > 0.0)) *s_bad = 1;
      else G[j * W + j] = sqrt(d);
    }
    __syncthreads();
    if (*s_bad) break;
    const double ljj = G[j * W + j];
    for (int i = j + 1 + tid; i < K; i += 256) G[i * W + j] /= ljj;
    __syncthreads();
    const int m = K - j - 1;
    for (int q = tid; q < m * m; q += 256) {
      const int ii = j + 1 + q / m, ll = j + 1 + q % m;
      if (ll <= ii) G[ii * W + ll] -= G[ii * W + j] * G[ll * W + j];
    }
    __syncthreads();
  }
  if (*s_bad) return true;   // block-uniform (read after the barrier that follows its last write)
  for (int p = 0; p < K; ++p) {
    if (tid == 0) G[p * W + K] /= G[p * W + p];
    __syncthreads();
    for (int i = p + 1 + tid; i < K; i += 256) G[i * W + K] -= G[i * W + p] * G[p * W + K];
    __syncthreads();
  }
  for (int p = K - 1; p >= 0; --p) {
    if (tid == 0) G[p * W + K] /= G[p * W + p];
    __syncthreads();
    for (int i = tid; i < p; i += 256) G[i * W + K] -= G[p * W + i] * G[p * W + K];
    __syncthreads();
  }
  return false;
}

// LDS of the solving build: G [K][K+1] plus a row stage of up to 32 rows (fewer
// at K >= 128) within 150 KiB.  rows = 0: K is too large.
inline void fi_solve_lds(int K, int* rows, size_t* gbytes, size_t* stage_bytes) {
  const size_t W = (size_t)K + 1, WS = (size_t)K + 2, budget = 150 * 1024;
  *gbytes = (size_t)K * W * sizeof(double);
  *rows = 0;
  *stage_bytes = 0;
  if (*gbytes + 8 * WS * sizeof(double) > budget) return;
  *rows = (int)std::min<size_t>(32, (budget - *gbytes) / (WS * sizeof(double)));
  *stage_bytes = (size_t)*rows * WS * sizeof(double);
}

inline bool fi_all_finite(const double* a, int64_t n) {
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite(a[i])) return false;
  return true;
}

// What mr_fold_in and mr_explain refuse about the table, the form and the
// lists; `who` opens the message.
inline int fi_validate(const char* who, int k, int n_rows, const double* T,
                       const double* row_offset, int mode, int intercept, double alpha,
                       double reg, int reg_mode, int n_ent, const long long* off, const int* idx,
                       const double* r) {
  const std::string w = std::string(who) + ": ";
  MR_CHECK(k >= 1 && k <= kMaxK, w + "k must be in 1..128");
  MR_CHECK(mode == MR_FOLD_EXPLICIT || mode == MR_FOLD_IMPLICIT, w + "unknown mode");
  MR_CHECK(intercept == 0 || intercept == 1, w + "intercept must be 0 or 1");
  const bool implicit = mode == MR_FOLD_IMPLICIT;
  MR_CHECK(!implicit || (!intercept && !row_offset),
           w + "the implicit mode takes no intercept and no row_offset");
  MR_CHECK(reg_mode == MR_REG_CONSTANT || reg_mode == MR_REG_WEIGHTED,
           w + "unknown regularization mode");
  MR_CHECK(std::isfinite(alpha) && alpha >= 0.0, w + "alpha must be finite and >= 0");
  MR_CHECK(std::isfinite(reg) && reg >= 0.0, w + "reg must be finite and >= 0");
  MR_CHECK(n_ent >= 0 && n_rows >= 0, w + "negative sizes");
  if (n_ent == 0) return 0;
  MR_CHECK(off, w + "off is required");
  MR_CHECK(rk_offsets_ok(off, n_ent), w + "offsets must start at 0 and not decrease");
  const int64_t nnz = off[n_ent];
  MR_CHECK(nnz == 0 || (idx && r), w + "idx and r are required");
  MR_CHECK(n_rows == 0 || T, w + "T is required");
  for (int e = 0; e < n_ent; ++e)
    MR_CHECK(off[e + 1] - off[e] < 0x7fffffff, w + "list too long");
  for (int64_t i = 0; i < nnz; ++i) {
    MR_CHECK(idx[i] >= 0 && idx[i] < n_rows, w + "id out of range");
    MR_CHECK(std::isfinite(r[i]), w + "r must be finite");
    MR_CHECK(!implicit || r[i] >= 0.0, w + "r must be >= 0 in the implicit mode");
  }
  MR_CHECK(fi_all_finite(T, (int64_t)n_rows * k), w + "T must be finite");
  MR_CHECK(!row_offset || fi_all_finite(row_offset, n_rows), w + "row_offset must be finite");
  return 0;
}

}  // namespace mr
