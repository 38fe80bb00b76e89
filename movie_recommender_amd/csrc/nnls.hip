// Non-negative ALS (DESIGN.md "Non-negative factors"): the per-entity solver
//   minimise 1/2 x^T (G_e + ridge I) x - c_e^T x   subject to x_j >= 0, j < k
// by block principal pivoting (Kim and Park, with their backup rule) on the
// side's normal equations as Engine::normal_equations left them.  The user
// bias (coordinate k) is free: always in the solve, never a pivot candidate.
// Nothing here touches the Gram, ridge or CG kernels; Engine::solve_nnls
// launches it where the Cholesky solver would run.
#include "mr_internal.h"

namespace mr {

// ---------------------------------------------------------------------------
// One 256-thread workgroup per entity, all of the entity's rounds in the one
// launch.  State: infree[j] (coordinate j is in the free set F), the ordered
// index list idx[0 .. p) of F (ascending, the bias last on the user side) and
// the backup rule's (ninf, pb), which every thread carries in registers (they
// are functions of block-uniform values).
//
// A round:
//   1. compact F into idx (two wave ballots: k <= 128);
//   2. gather the lower triangle of G_FF (+ ridge on the diagonal) from the
//      tri16 G_e (and Gs, Gn on the user side) into a p x p fp64 LDS matrix M
//      with row stride ld = p | 1, and c_F as row p of it;
//   3. factor M = L D L^T in place, unscaled (M[i][j] keeps L[i][j] d_j), so a
//      column needs ONE barrier: step j only reads column j and the pivot and
//      writes columns > j.  Row p rides along as one more row, which is the
//      forward substitution: it ends as z with L z = c_F.  The 256 threads
//      own the trailing elements 2-D cyclically (row mod 16, column mod 16);
//   4. back-substitute x_i = (z_i - sum_{a > i} M[a][i] x_a) / d_i, row-
//      oriented (z_j -= M[i][j] x_i for j < i), one barrier per row; step 3
//      left 1 / d_i in LDS, so no division stands in this chain;
//   5. y_j = (G x)_j - c_j for j outside F, G re-read from global memory (L2),
//      two lanes per row; val[j] = x_j on F and y_j elsewhere, so the
//      violation test is val[j] < 0 (strict) for both kinds;
//   6. none: converged.  Else exchange all of V (or only its largest index
//      once the backup rule has run out of retries) and go round again.
// A pivot <= 0, or a diagonal entry of G + ridge I <= 0 before the first
// round, makes the entity non-PD: it keeps max(previous x, 0) on the
// constrained coordinates and its previous bias.
// ---------------------------------------------------------------------------
constexpr int kNnlsMaxK = kMaxK + 1;   // coordinates of a user with the bias

template <bool USER>
__global__ __launch_bounds__(256) void nnls_kernel(
    int64_t E, int k, int ldk, double ridge, int max_rounds, int warm,
    const float* __restrict__ G, const float* __restrict__ Gs, const float* __restrict__ Gn,
    const float* __restrict__ C, const float* __restrict__ Cb, float* __restrict__ x,
    float* __restrict__ xb, int* __restrict__ rounds, int* __restrict__ nonpd) {
  extern __shared__ double sm[];
  const int K = USER ? k + 1 : k;
  double* M = sm;                        // (K+1) x (K+1): rows 0 .. p, stride p | 1
  double* xs = M + (K + 1) * (K + 1);    // K+1: the round's solution over idx
  double* val = xs + (K + 1);            // K: x_j on F, y_j elsewhere
  double* cn = val + K;                  // K: c_e
  double* dinv = val;                    // 1 / d_j of the round's factorisation (val is
                                         // dead from the exchange to the end of step 4)
  __shared__ int idx[kNnlsMaxK + 1];
  __shared__ int infree[kNnlsMaxK + 1];
  __shared__ int cnt[2];
  __shared__ int nV, maxV;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t e = blockIdx.x;
  const int nb = nb16_of(k);
  const float* Ge = G + e * gsize_of(k);
  const float* Gse = USER ? Gs + e * ldk : nullptr;
  float* xe = x + e * ldk;
  // natural element (i, j) of G_e, i, j < K, without the solver's ridge
  auto g = [&](int i, int j) -> double {
    if (i < k && j < k) return (double)Ge[packed_offset(i, j, nb)];
    if (!USER) return 0.0;
    if (i < k) return (double)Gse[i];
    if (j < k) return (double)Gse[j];
    return (double)Gn[e];
  };
  // previous x, clamped: what a non-PD entity keeps (the bias is not written)
  auto keep_previous = [&]() {
    for (int t = tid; t < k; t += blockDim.x) {
      const float v = xe[t];
      xe[t] = v > 0.f ? v : 0.f;
    }
    if (tid == 0) {
      rounds[e] = 0;
      atomicAdd(nonpd, 1);
    }
  };

  int bad_diag = 0;
  for (int t = tid; t < K; t += blockDim.x) {
    cn[t] = (t < k) ? (double)C[e * ldk + t] : (double)Cb[e];
    if (!(g(t, t) + ridge > 0.0)) bad_diag = 1;
    infree[t] = (t < k) ? (warm && xe[t] > 0.f) : 1;
  }
  if (__syncthreads_or(bad_diag)) {
    keep_previous();
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
    const int p = nF + (USER ? 1 : 0);
    if (f) idx[(w ? cnt[0] : 0) + __popcll(bal & ((1ull << lane) - 1ull))] = tid;
    if (USER && tid == 0) idx[nF] = k;
    __syncthreads();
    // 2. lower triangle of G_FF + ridge I, and c_F as row p
    const int ld = p | 1;
    for (int t = tid; t < (p + 1) * p; t += blockDim.x) {
      const int a = t / p, b = t - a * p;
      if (b > a) continue;
      double v;
      if (a < p) {
        v = g(idx[a], idx[b]);
        if (a == b) v += ridge;
      } else {
        v = cn[idx[b]];
      }
      M[a * ld + b] = v;
    }
    __syncthreads();
    // 3. M = L D L^T, row p becomes z (L z = c_F)
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
      keep_previous();
      return;
    }
    // 4. back substitution over the rows of M
    double* z = M + p * ld;
    for (int i = p - 1; i >= 0; --i) {
      const double xi = z[i] * dinv[i];
      for (int j = tid; j < i; j += blockDim.x) z[j] -= M[i * ld + j] * xi;
      if (tid == 0) xs[i] = xi;
      __syncthreads();
    }
    ++round;
    // 5. val = x on F (and the bias), y = G x - c elsewhere
    if (tid < p) val[idx[tid]] = xs[tid];
    for (int row = tid >> 1; row < k; row += 128) {
      double acc = 0.0;
      if (!infree[row])
        for (int a = tid & 1; a < p; a += 2) acc += g(row, idx[a]) * xs[a];
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
  for (int t = tid; t < k; t += blockDim.x) {
    const double v = infree[t] ? val[t] : 0.0;
    xe[t] = v > 0.0 ? (float)v : 0.f;
  }
  if (USER && tid == 0) xb[e] = (float)val[k];
  if (tid == 0) rounds[e] = converged ? round : -round;
}

int launch_nnls(hipStream_t s, bool user_side, int64_t E, int k, double ridge, int max_rounds,
                bool warm, const float* G, const float* Gs, const float* Gn, const float* C,
                const float* Cb, float* x, float* xb, int* rounds, int* nonpd) {
  if (E <= 0) return 0;
  MR_CHECK(k <= kMaxK, "the exact (NNLS) solver holds the free block in LDS: k <= 128");
  MR_CHECK(max_rounds >= 1, "nnls: max_rounds must be >= 1");
  const int K = user_side ? k + 1 : k;
  const size_t lds = (size_t)((K + 1) * (K + 1) + (K + 1) + 2 * K) * sizeof(double);
  if (user_side) {
    MR_HIP(hipFuncSetAttribute((const void*)nnls_kernel<true>,
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    MR_LAUNCH(nnls_kernel<true>, dim3((unsigned)E), dim3(256), lds, s,
        E, k, ldk_of(k), ridge, max_rounds, warm ? 1 : 0, G, Gs, Gn, C, Cb, x, xb, rounds, nonpd);
  } else {
    MR_HIP(hipFuncSetAttribute((const void*)nnls_kernel<false>,
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    MR_LAUNCH(nnls_kernel<false>, dim3((unsigned)E), dim3(256), lds, s,
        E, k, ldk_of(k), ridge, max_rounds, warm ? 1 : 0, G, Gs, Gn, C, Cb, x, xb, rounds, nonpd);
  }
  MR_HIP(hipGetLastError());
  return 0;
}

}  // namespace mr
