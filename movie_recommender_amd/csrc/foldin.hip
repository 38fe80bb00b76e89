// Fold-in for every trained model on MI355X (gfx950): new users or new items
// from the opposite factor table, explicit (ridge, optional intercept and row
// offsets) or implicit (S = T^T T, confidence weights), unconstrained
// (Cholesky) or non-negative (block principal pivoting).
// C ABI: include/mr_foldin.h.  DESIGN.md "Fold-in".
#include "foldin_device.h"

namespace mr {

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
// Entity e = e0 + blockIdx.x.  The build and the solve are fi_build and
// fi_cholesky_solve of foldin_device.h, which explain.hip runs as well.
// ---------------------------------------------------------------------------
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
  double* G = SOLVE ? lds : scratch + (int64_t)blockIdx.x * K * W;   // [K][W]
  double* As = SOLVE ? lds + K * W : lds;                            // [rows_per_stage][WS]
  const double lam = weighted ? reg * (double)M : reg;
  fi_build(k, icpt, implicit, rows_per_stage, alpha, lam, b, M, idx, r, T, roff, S, G, As);
  if constexpr (SOLVE) {
    if (fi_cholesky_solve(K, G, &s_bad)) {
      for (int i = tid; i < K; i += 256) X[(int64_t)e * K + i] = 0.0;
      if (tid == 0) {
        status[e] = 0;
        rounds[e] = 0;
      }
      return;
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
static int fold_in(int device, int k, int n_rows, const double* T, const double* row_offset,
                   int mode, int intercept, double alpha, double reg, int reg_mode, int nonneg,
                   int max_rounds, int n_new, const long long* off, const int* idx,
                   const double* r, double* x_out, int* status, int* rounds) {
  MR_CHECK(nonneg == 0 || nonneg == 1, "fold-in: nonneg must be 0 or 1");
  MR_CHECK(max_rounds >= 0, "fold-in: max_rounds must be >= 0");
  if (fi_validate("fold-in", k, n_rows, T, row_offset, mode, intercept, alpha, reg, reg_mode,
                  n_new, off, idx, r))
    return -1;
  if (n_new == 0) return 0;
  MR_CHECK(x_out, "fold-in: x_out is required");
  const bool implicit = mode == MR_FOLD_IMPLICIT;
  const int64_t nnz = off[n_new];

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
    int rows;
    size_t gb, stage;
    fi_solve_lds(K, &rows, &gb, &stage);
    MR_CHECK(rows > 0, "fold-in: k too large");
    const size_t lds = gb + stage;
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
