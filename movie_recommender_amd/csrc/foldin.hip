// Fold-in for every trained model on MI355X (gfx950): new users or new items
// from the opposite factor table, explicit (ridge, optional intercept and row
// offsets) or implicit (S = T^T T, confidence weights), unconstrained
// (Cholesky) or non-negative (block principal pivoting).
// C ABI: include/mr_foldin.h.  DESIGN.md "Fold-in".
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/mr_als.h"
#include "../../include/mr_foldin.h"
#include "mr_internal.h"

namespace mr {

__device__ __forceinline__ double fi_mul(double a, double b) {   // a product rounded on its own
#pragma clang fp contract(off)
  return a * b;
}

// ---------------------------------------------------------------------------
// K-FI1: the normal equations of one entity per 256-thread workgroup, the
// shape of implicit_fold_in_kernel (ranking.hip K-F2) for the four forms.
// Rows [a | 1 | weight | rhs coefficient] are staged rows_per_stage at a time
// (the 1 only with an intercept; weight = 1 or w = alpha r; rhs coefficient =
// r - offset or 1 + w).  Each thread owns FI_NE entries of the upper triangle
// of sum weight [a,1][a,1]^T in registers (row order, several passes when
// K (K + 1) / 2 > 256 FI_NE), threads 0 .. K-1 also one entry of c.  Then
// G = (S +) sum + lambda_e I_k goes to a [K][K+1] matrix, the rhs in column K:
//   SOLVE:  in LDS, factored and solved here (the Cholesky of K-F2: with the
//           implicit form every operation and its order are that kernel's, so
//           the bits are);
//   !SOLVE: in global memory, block b's slot of `scratch`, for K-FI2.
// Entity e = e0 + blockIdx.x.
// ---------------------------------------------------------------------------
constexpr int FI_NE = 9;

template <bool SOLVE>
__global__ __launch_bounds__(256) void fold_build_kernel(
    int e0, int k, int icpt, int implicit, int rows_per_stage, double alpha, double reg,
    int weighted, const int64_t* __restrict__ off, const int* __restrict__ idx,
    const double* __restrict__ r, const double* __restrict__ T, const double* __restrict__ roff,
    const double* __restrict__ S, double* __restrict__ scratch, double* __restrict__ X,
    int* __restrict__ status, int* __restrict__ rounds) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  __shared__ int s_bad;
  const int K = k + icpt;
  const int W = K + 1;    // row width of G: K coordinates, then the rhs
  const int WS = K + 2;   // row width of the stage: K coordinates, weight, rhs coefficient
  const int e = e0 + blockIdx.x, tid = threadIdx.x;
  const int64_t b = off[e];
  const int M = (int)(off[e + 1] - b);
  if (M == 0) {   // block-uniform: an entity without ratings is the zero row
    if (SOLVE) {
      for (int i = tid; i < K; i += 256) X[(int64_t)e * K + i] = 0.0;
      if (tid == 0) {
        status[e] = 1;
        rounds[e] = 0;
      }
    }
    return;
  }
  const int NT = K * (K + 1) / 2;
  double* G = SOLVE ? lds : scratch + (int64_t)blockIdx.x * K * W;   // [K][W]
  double* As = SOLVE ? lds + K * W : lds;                            // [rows_per_stage][WS]
  const double lam = weighted ? reg * (double)M : reg;
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
  if constexpr (SOLVE) {
    if (tid == 0) s_bad = 0;
    __syncthreads();
    for (int j = 0; j < K; ++j) {
      if (tid == 0) {
        const double d = G[j * W + j];
        if (!(d > 0.0)) s_bad = 1;
        else G[j * W + j] = sqrt(d);
      }
      __syncthreads();
      if (s_bad) break;
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
    if (s_bad) {   // block-uniform (read after the barrier that follows its last write)
      for (int i = tid; i < K; i += 256) X[(int64_t)e * K + i] = 0.0;
      if (tid == 0) {
        status[e] = 0;
        rounds[e] = 0;
      }
      return;
    }
    // L y = c (right-looking), then L^T x = y
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
    for (int i = tid; i < K; i += 256) X[(int64_t)e * K + i] = G[i * W + K];
    if (tid == 0) {
      status[e] = 1;
      rounds[e] = 1;
    }
  }
}

// ---------------------------------------------------------------------------
// K-FI2: the non-negative solve of one entity per 256-thread workgroup, the
// rounds of nnls_kernel (nnls.hip) in fp64 from a cold start: the free set F
// starts empty (the intercept, coordinate k, is always in it and never a pivot
// candidate).  G_e and c_e are K-FI1's [K][K+1] slot in global memory, re-read
// per round (it stays in L2: 133 KB at K = 129); LDS holds the round's
// (p + 1) x p factorisation workspace M, the solution xs, val (x on F, y = G x
// - c elsewhere), c and 1 / d.  infree / idx / the backup rule's (ninf, pb) are
// functions of block-uniform values only, so every branch that leads to a
// barrier is taken by the whole block.
// ---------------------------------------------------------------------------
constexpr int kFoldMaxK = kMaxK + 1;

__global__ __launch_bounds__(256) void fold_nnls_kernel(
    int e0, int k, int icpt, int max_rounds, const int64_t* __restrict__ off,
    const double* __restrict__ scratch, double* __restrict__ X, int* __restrict__ status,
    int* __restrict__ rounds) {
  extern __shared__ double sm[];
  const int K = k + icpt, W = K + 1;
  double* M = sm;                        // (K+1) x (K+1): rows 0 .. p, stride p | 1
  double* xs = M + (K + 1) * (K + 1);    // K+1: the round's solution over idx
  double* val = xs + (K + 1);            // K: x_j on F, y_j elsewhere
  double* cn = val + K;                  // K: c_e
  double* dinv = cn + K;                 // K: 1 / d_j of the round's factorisation
  __shared__ int idx[kFoldMaxK + 1];
  __shared__ int infree[kFoldMaxK + 1];
  __shared__ int cnt[2];
  __shared__ int nV, maxV;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int e = e0 + blockIdx.x;
  const double* Ge = scratch + (int64_t)blockIdx.x * K * W;
  double* xe = X + (int64_t)e * K;
  auto finish_zero = [&](int st) {   // the zero row
    for (int t = tid; t < K; t += 256) xe[t] = 0.0;
    if (tid == 0) {
      status[e] = st;
      rounds[e] = 0;
    }
  };
  if (off[e + 1] == off[e]) {   // block-uniform; K-FI1 wrote no slot
    finish_zero(1);
    return;
  }
  int bad_diag = 0;
  for (int t = tid; t < K; t += 256) {
    cn[t] = Ge[t * W + K];
    if (!(Ge[t * W + t] > 0.0)) bad_diag = 1;
    infree[t] = t < k ? 0 : 1;
  }
  if (__syncthreads_or(bad_diag)) {
    finish_zero(0);
    return;
  }

  int ninf = K + 1, pb = 3, round = 0;
  bool converged = false;
  while (true) {
    // 1. the ordered free list
    const bool f = tid < k && infree[tid];
    const unsigned long long bal = __ballot(f);
    if (w < 2 && lane == 0) cnt[w] = __popcll(bal);
    if (tid == 0) {
      nV = 0;
      maxV = -1;
    }
    __syncthreads();
    const int nF = cnt[0] + cnt[1];
    const int p = nF + icpt;
    if (f) idx[(w ? cnt[0] : 0) + __popcll(bal & ((1ull << lane) - 1ull))] = tid;
    if (icpt && tid == 0) idx[nF] = k;
    __syncthreads();
    // 2. lower triangle of G_FF, and c_F as row p
    const int ld = p | 1;
    for (int t = tid; t < (p + 1) * p; t += 256) {
      const int a = t / p, c = t - a * p;
      if (c > a) continue;
      M[a * ld + c] = a < p ? Ge[idx[a] * W + idx[c]] : cn[idx[c]];
    }
    __syncthreads();
    // 3. M = L D L^T unscaled, row p becomes z (L z = c_F): one barrier a column
    const int ti = tid >> 4, tl = tid & 15;
    bool npd = false;
    for (int j = 0; j < p; ++j) {
      const double d = M[j * ld + j];   // block-uniform: every thread leaves together
      if (!(d > 0.0)) {
        npd = true;
        break;
      }
      const double inv = 1.0 / d;
      if (tid == 0) dinv[j] = inv;
      const int i0 = j + 1 + ((ti - (j + 1)) & 15);   // first row > j with row % 16 == ti
      const int l0 = j + 1 + ((tl - (j + 1)) & 15);
      for (int i = i0; i <= p; i += 16) {
        const double lij = M[i * ld + j] * inv;
        const int lend = i < p ? i : p - 1;
        for (int l = l0; l <= lend; l += 16) M[i * ld + l] -= lij * M[l * ld + j];
      }
      __syncthreads();
    }
    if (npd) {
      finish_zero(0);
      return;
    }
    // 4. back substitution over the rows of M
    double* z = M + p * ld;
    for (int i = p - 1; i >= 0; --i) {
      const double xi = z[i] * dinv[i];
      for (int j = tid; j < i; j += 256) z[j] -= M[i * ld + j] * xi;
      if (tid == 0) xs[i] = xi;
      __syncthreads();
    }
    ++round;
    // 5. val = x on F (and the intercept), y = G x - c elsewhere
    if (tid < p) val[idx[tid]] = xs[tid];
    for (int row = tid >> 1; row < k; row += 128) {
      double acc = 0.0;
      if (!infree[row])
        for (int a = tid & 1; a < p; a += 2) acc += Ge[row * W + idx[a]] * xs[a];
      acc += __shfl_xor(acc, 1);
      if (!infree[row] && (tid & 1) == 0) val[row] = acc - cn[row];
    }
    __syncthreads();
    // 6. violations and the exchange
    const bool viol = tid < k && val[tid] < 0.0;
    if (viol) {
      atomicAdd(&nV, 1);
      atomicMax(&maxV, tid);
    }
    __syncthreads();
    const int nv = nV, mv = maxV;
    if (nv == 0) {
      converged = true;
      break;
    }
    if (round >= max_rounds) break;
    bool all;
    if (nv < ninf) {
      ninf = nv;
      pb = 3;
      all = true;
    } else if (pb >= 1) {
      --pb;
      all = true;
    } else {
      all = false;
    }
    if (viol && (all || tid == mv)) infree[tid] ^= 1;
    __syncthreads();
  }
  // coordinates outside F are +0; a negative x_j of an unconverged entity too
  for (int t = tid; t < k; t += 256) {
    const double v = infree[t] ? val[t] : 0.0;
    xe[t] = v > 0.0 ? v : 0.0;
  }
  if (icpt && tid == 0) xe[k] = val[k];
  if (tid == 0) {
    status[e] = converged ? 1 : -1;
    rounds[e] = round;
  }
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
static bool all_finite(const double* a, int64_t n) {
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite(a[i])) return false;
  return true;
}

static int fold_in(int device, int k, int n_rows, const double* T, const double* row_offset,
                   int mode, int intercept, double alpha, double reg, int reg_mode, int nonneg,
                   int max_rounds, int n_new, const long long* off, const int* idx,
                   const double* r, double* x_out, int* status, int* rounds) {
  MR_CHECK(k >= 1 && k <= kMaxK, "fold-in: k must be in 1..128");
  MR_CHECK(mode == MR_FOLD_EXPLICIT || mode == MR_FOLD_IMPLICIT, "fold-in: unknown mode");
  MR_CHECK(intercept == 0 || intercept == 1, "fold-in: intercept must be 0 or 1");
  MR_CHECK(nonneg == 0 || nonneg == 1, "fold-in: nonneg must be 0 or 1");
  const bool implicit = mode == MR_FOLD_IMPLICIT;
  MR_CHECK(!implicit || (!intercept && !row_offset),
           "fold-in: the implicit mode takes no intercept and no row_offset");
  MR_CHECK(reg_mode == MR_REG_CONSTANT || reg_mode == MR_REG_WEIGHTED,
           "fold-in: unknown regularization mode");
  MR_CHECK(std::isfinite(alpha) && alpha >= 0.0, "fold-in: alpha must be finite and >= 0");
  MR_CHECK(std::isfinite(reg) && reg >= 0.0, "fold-in: reg must be finite and >= 0");
  MR_CHECK(max_rounds >= 0, "fold-in: max_rounds must be >= 0");
  MR_CHECK(n_new >= 0 && n_rows >= 0, "fold-in: negative sizes");
  if (n_new == 0) return 0;
  MR_CHECK(off && x_out, "fold-in: off and x_out are required");
  MR_CHECK(rk_offsets_ok(off, n_new), "fold-in: offsets must start at 0 and not decrease");
  const int64_t nnz = off[n_new];
  MR_CHECK(nnz == 0 || (idx && r), "fold-in: idx and r are required");
  MR_CHECK(n_rows == 0 || T, "fold-in: T is required");
  for (int e = 0; e < n_new; ++e)
    MR_CHECK(off[e + 1] - off[e] < 0x7fffffff, "fold-in: list too long");
  for (int64_t i = 0; i < nnz; ++i) {
    MR_CHECK(idx[i] >= 0 && idx[i] < n_rows, "fold-in: id out of range");
    MR_CHECK(std::isfinite(r[i]), "fold-in: r must be finite");
    MR_CHECK(!implicit || r[i] >= 0.0, "fold-in: r must be >= 0 in the implicit mode");
  }
  MR_CHECK(all_finite(T, (int64_t)n_rows * k), "fold-in: T must be finite");
  MR_CHECK(!row_offset || all_finite(row_offset, n_rows), "fold-in: row_offset must be finite");

  const int K = k + intercept;
  const int cap = max_rounds > 0 ? max_rounds : 4 * (k + 1);
  RkScope sc;
  if (sc.init(device)) return -1;
  hipStream_t s = sc.s;
  const int kk = k * k;
  RkBuf<double> dT, dro, dpart, dS, dr, dX, dscr;
  RkBuf<int64_t> doff;
  RkBuf<int> didx, dstat, drnd;
  if (dT.upload(T, (int64_t)n_rows * k, s) ||
      doff.upload(reinterpret_cast<const int64_t*>(off), (int64_t)n_new + 1, s) ||
      didx.upload(idx, nnz, s) || dr.upload(r, nnz, s) || dX.alloc((int64_t)n_new * K) ||
      dstat.alloc(n_new) || drnd.alloc(n_new))
    return -1;
  if (row_offset && dro.upload(row_offset, n_rows, s)) return -1;
  if (implicit) {
    const int nblk = (int)std::max<int64_t>(1, std::min<int64_t>(((int64_t)n_rows + 63) / 64, 256));
    if (dpart.alloc((int64_t)nblk * kk) || dS.alloc(kk)) return -1;
    fold_yty_partial_kernel<<<dim3(nblk, (kk + 256 * FY_NQ - 1) / (256 * FY_NQ)), 256, 0, s>>>(
        dT.p, n_rows, k, dpart.p);
    fold_yty_combine_kernel<<<(kk + 255) / 256, 256, 0, s>>>(dpart.p, nblk, kk, dS.p);
    MR_HIP(hipGetLastError());
  }
  const int weighted = reg_mode == MR_REG_WEIGHTED ? 1 : 0;
  const size_t W = (size_t)K + 1, WS = (size_t)K + 2, gbytes = (size_t)K * W * sizeof(double);
  if (!nonneg) {
    // LDS: G [K][K+1] plus a row stage of up to 32 rows (fewer at K >= 128)
    const size_t budget = 150 * 1024;
    MR_CHECK(gbytes + 8 * WS * sizeof(double) <= budget, "fold-in: k too large");
    const int rows = (int)std::min<size_t>(32, (budget - gbytes) / (WS * sizeof(double)));
    const size_t lds = gbytes + (size_t)rows * WS * sizeof(double);
    if (lds > 64 * 1024)
      MR_HIP(hipFuncSetAttribute((const void*)fold_build_kernel<true>,
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    fold_build_kernel<true><<<n_new, 256, lds, s>>>(
        0, k, intercept, implicit ? 1 : 0, rows, alpha, reg, weighted, doff.p, didx.p, dr.p,
        dT.p, dro.p, dS.p, nullptr, dX.p, dstat.p, drnd.p);
    MR_HIP(hipGetLastError());
  } else {
    // entities per launch: the [K][K+1] fp64 slots stay below 256 MiB
    const int chunk = (int)std::max<int64_t>(
        1, std::min<int64_t>(n_new, (int64_t)(1LL << 28) / (int64_t)gbytes));
    if (dscr.alloc((int64_t)chunk * K * (int64_t)W)) return -1;
    const int rows = 32;
    const size_t lds_b = (size_t)rows * WS * sizeof(double);
    const size_t lds_n = (size_t)((K + 1) * (K + 1) + (K + 1) + 3 * K) * sizeof(double);
    if (lds_n > 64 * 1024)
      MR_HIP(hipFuncSetAttribute((const void*)fold_nnls_kernel,
                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_n));
    for (int e0 = 0; e0 < n_new; e0 += chunk) {
      const int nb = std::min(chunk, n_new - e0);
      fold_build_kernel<false><<<nb, 256, lds_b, s>>>(
          e0, k, intercept, implicit ? 1 : 0, rows, alpha, reg, weighted, doff.p, didx.p, dr.p,
          dT.p, dro.p, dS.p, dscr.p, dX.p, dstat.p, drnd.p);
      fold_nnls_kernel<<<nb, 256, lds_n, s>>>(e0, k, intercept, cap, doff.p, dscr.p, dX.p,
                                              dstat.p, drnd.p);
      MR_HIP(hipGetLastError());
    }
  }
  MR_D2H(x_out, dX.p, (size_t)n_new * K * 8, s);
  if (status) MR_D2H(status, dstat.p, (size_t)n_new * 4, s);
  if (rounds) MR_D2H(rounds, drnd.p, (size_t)n_new * 4, s);
  MR_HIP(hipStreamSynchronize(s));
  return 0;
}

}  // namespace mr

extern "C" {

int mr_fold_in(int device, int k, int n_rows, const double* T, const double* row_offset, int mode,
               int intercept, double alpha, double reg, int reg_mode, int nonneg, int max_rounds,
               int n_new, const long long* off, const int* idx, const double* r, double* x_out,
               int* status, int* rounds) {
  return mr::rk_guard([&]() {
    return mr::fold_in(device, k, n_rows, T, row_offset, mode, intercept, alpha, reg, reg_mode,
                       nonneg, max_rounds, n_new, off, idx, r, x_out, status, rounds);
  });
}

}  // extern "C"
