// Blocked exact solve (DESIGN.md "Blocked exact solve"): per-entity
// (G_e + ridge I) x_e = c_e by a tiled, left-looking Cholesky factorisation
// whose 16 x 16 x 16 products run on the fp64 matrix instruction
// (v_mfma_f64_16x16x4_f64).  Same operands and results as solve_kernel
// (kernels.hip), for every 1 <= k <= 512: the factor lives in a global
// scratch slot, tile by tile, not in LDS.  Selected by MR_OPT_SOLVE_BLOCKED;
// nothing here touches the Gram, ridge, CG or NNLS kernels.
//
// One 256-thread workgroup per slot, looping over entities slot, slot +
// slots, ...; no block waits for another (the only synchronisation is
// __syncthreads).
//
// Coordinates.  The factorisation runs over the "factor index" f < 16 T,
// T = ceil(K / 16): f < 16 NB is the virtual (tri16) index of mr_internal.h,
// so every G tile is one contiguous stored tile; on the user side the bias
// takes the virtual slot of natural index k when k < 16 NB, and slot 16 NB (a
// tile of its own) when k is a multiple of 16.  Every other slot is padding:
// unit diagonal, zero elsewhere, zero rhs.  x is permuted back on the way out.
//
// Tiles.  Slot tile (i, j), j <= i, at ((i (i + 1) / 2 + j) * 256 doubles, in
// "fragment order": element [reg * 64 + lane] = L_ij[lane & 15][(lane >> 4) +
// 4 reg].  That is at once the C/D layout in which the transposed tile leaves
// the matrix instruction and the A / B operand of k-step `reg` of a later
// product (the four k-slots of a step are lane groups; which four columns they
// hold is free as long as A and B agree), so tiles go from accumulator to
// memory to operand with no transpose, 512 contiguous bytes per access.
// The diagonal tile holds W_jj = L_jj^-1 in the same order.
//
// Per tile column j (two barriers):
//   (a) wave w: P_w = sum_{m < j, m = w mod 4} L_jm L_jm^T into LDS; barrier
//   (b) every wave, redundantly and in registers: A_jj = G_jj - sum_w P_w,
//       its 16 x 16 Cholesky factor (pivot check: lane- and wave-uniform, so
//       "not PD" is block-uniform with no further barrier) and W = L_jj^-1
//   (c) the waves share tile rows i > j and the rhs (one more row):
//       A_ij^T = G_ij^T - sum_m L_jm L_im^T, L_ij^T = W A_ij^T, stored; barrier
// then the back substitution x_j = W_jj^T (z_j - sum_{i > j} L_ij^T x_i) walks
// the tile columns in reverse on the vector ALU (two barriers per column).
#include "mr_internal.h"

namespace mr {
namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int kMaxT = (kMaxKLarge + 1 + 15) / 16;   // 33 tile rows at K = 513

__device__ __forceinline__ int64_t lt_off(int i, int j) {   // j <= i
  return ((int64_t)i * (i + 1) / 2 + j) * 256;
}

// natural coordinate of factor index f (>= K: padding)
__device__ __forceinline__ int ncoord(int f, int k, int nb) {
  return f < 16 * nb ? nb * (f & 15) + (f >> 4) : k + (f - 16 * nb);
}

// lane `src` (compile-time constant after unrolling) of v, to every lane
__device__ __forceinline__ double bcast(double v, int src) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
  return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double sum16(double v) {   // over the 16 lanes sharing lane >> 4
  v += __shfl_xor(v, 8, 16);
  v += __shfl_xor(v, 4, 16);
  v += __shfl_xor(v, 2, 16);
  v += __shfl_xor(v, 1, 16);
  return v;
}

template <bool USER>
struct Entity {
  const float* G;    // tri16
  const float* Gs;   // user side: bias row
  const float* Gn;   // user side: bias corner
  const float* C;
  const float* Cb;
  int k, nb;
  double ridge;

  // element (fa, fb) of the matrix being factored, in factor coordinates
  __device__ __forceinline__ double a(int fa, int fb) const {
    const int last = USER ? k : k - 1;
    const int na = ncoord(fa, k, nb), nc = ncoord(fb, k, nb);
    if (na > last || nc > last) return fa == fb ? 1.0 : 0.0;
    if (USER && (na == k || nc == k)) {
      if (na == nc) return (double)Gn[0] + ridge;
      return (double)Gs[na == k ? nc : na];
    }
    const double v = G[packed_offset_virt(fa, fb, nb)];
    return fa == fb ? v + ridge : v;
  }
  __device__ __forceinline__ double c(int f) const {
    const int n = ncoord(f, k, nb);
    if (n < k) return (double)C[n];
    if (USER && n == k) return (double)Cb[0];
    return 0.0;
  }
};

template <bool USER>
__global__ __launch_bounds__(256, 2) void solve_blocked_kernel(
    int64_t E, int k, int ldk, double ridge, const float* __restrict__ G,
    const float* __restrict__ Gs, const float* __restrict__ Gn,
    const float* __restrict__ C, const float* __restrict__ Cb,
    float* __restrict__ x, float* __restrict__ xb, int* __restrict__ nonpd,
    double* __restrict__ scratch, int64_t slot_doubles) {
  __shared__ double s_part[4][256];
  __shared__ double s_z[16 * kMaxT];
  __shared__ double s_x[16 * kMaxT];
  __shared__ double s_v[16];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int g = lane >> 4, c16 = lane & 15;
  const int K = USER ? k + 1 : k;
  const int T = (K + 15) / 16;
  const int nb = nb16_of(k);
  double* __restrict__ Ls = scratch + (int64_t)blockIdx.x * slot_doubles;

  for (int64_t e = blockIdx.x; e < E; e += gridDim.x) {
    Entity<USER> ent;
    ent.G = G + e * gsize_of(k);
    ent.Gs = USER ? Gs + e * ldk : nullptr;
    ent.Gn = USER ? Gn + e : nullptr;
    ent.C = C + e * ldk;
    ent.Cb = USER ? Cb + e : nullptr;
    ent.k = k;
    ent.nb = nb;
    ent.ridge = ridge;
    bool bad = false;

    for (int j = 0; j < T; ++j) {
      // (a) this wave's share of the diagonal tile's update
      d4 p = {0.0, 0.0, 0.0, 0.0};
      for (int m = w; m < j; m += 4) {
        const double* t = Ls + lt_off(j, m);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const double v = t[s * 64 + lane];
          p = __builtin_amdgcn_mfma_f64_16x16x4f64(v, v, p, 0, 0, 0);
        }
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) s_part[w][s * 64 + lane] = p[s];
      __syncthreads();

      // (b) lane r = c16 holds row r of A_jj (every 16-lane group and every
      // wave the same values), then of L_jj, then of W = L_jj^-1
      double a[16], l[16];
      double rs_own = 1.0;   // lane c16 keeps 1 / L[c16][c16]
      {
        const int base = (c16 >> 2) * 64 + (c16 & 3) * 16;   // fragment index of (c16, 0)
#pragma unroll
        for (int c = 0; c < 16; ++c)
          a[c] = ent.a(16 * j + c16, 16 * j + c) -
                 (((s_part[0][base + c] + s_part[1][base + c]) + s_part[2][base + c]) +
                  s_part[3][base + c]);
      }
#pragma unroll
      for (int jj = 0; jj < 16; ++jj) {
        const double d = bcast(a[jj], jj);
        bad = bad || !(d > 0.0);
        const double rs = d > 0.0 ? 1.0 / sqrt(d) : 1.0;
        if (c16 == jj) rs_own = rs;
        const double lr = c16 >= jj ? a[jj] * rs : 0.0;
        l[jj] = lr;
#pragma unroll
        for (int c = jj + 1; c < 16; ++c) a[c] = fma(-lr, bcast(lr, c), a[c]);
      }
      if (bad) break;   // block-uniform
      double y[16];     // y[c] = W[c16][c]: L^T y = e_{c16}
#pragma unroll
      for (int c = 15; c >= 0; --c) {
        double sum = c16 == c ? 1.0 : 0.0;
#pragma unroll
        for (int t = c + 1; t < 16; ++t) sum = fma(-bcast(l[c], t), y[t], sum);
        y[c] = sum * bcast(rs_own, c);
      }
      double wa[4];     // A operand of k-step s: W[c16][g + 4 s]
#pragma unroll
      for (int s = 0; s < 4; ++s)
        wa[s] = g == 0 ? y[4 * s] : g == 1 ? y[4 * s + 1] : g == 2 ? y[4 * s + 2] : y[4 * s + 3];
      if (w == (j & 3)) {
        double* t = Ls + lt_off(j, j);
#pragma unroll
        for (int s = 0; s < 4; ++s) t[s * 64 + lane] = wa[s];
      }

      // (c) the panel: tile rows i = j + 1 + q, and the rhs as row q = rows
      const int rows = T - 1 - j;
      for (int q = w; q <= rows; q += 4) {
        const bool rhs = q == rows;
        const int i = j + 1 + q;
        d4 S = {0.0, 0.0, 0.0, 0.0};
        for (int m = 0; m < j; ++m) {
          const double* tj = Ls + lt_off(j, m);
          const double* ti = Ls + lt_off(rhs ? j : i, m);
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const double av = tj[s * 64 + lane];
            double bv;
            if (rhs) bv = c16 == 0 ? s_z[16 * m + g + 4 * s] : 0.0;
            else bv = ti[s * 64 + lane];
            S = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, S, 0, 0, 0);
          }
        }
        d4 acc;   // A_ij^T: row g + 4 s of block j, column c16 of block i
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int fj = 16 * j + g + 4 * s;
          double v;
          if (rhs) v = c16 == 0 ? ent.c(fj) : 0.0;
          else v = ent.a(16 * i + c16, fj);
          acc[s] = v - S[s];
        }
        d4 res = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < 4; ++s)
          res = __builtin_amdgcn_mfma_f64_16x16x4f64(wa[s], acc[s], res, 0, 0, 0);
        if (rhs) {
          if (c16 == 0) {
#pragma unroll
            for (int s = 0; s < 4; ++s) s_z[16 * j + g + 4 * s] = res[s];
          }
        } else {
          double* t = Ls + lt_off(i, j);
#pragma unroll
          for (int s = 0; s < 4; ++s) t[s * 64 + lane] = res[s];
        }
      }
      __syncthreads();
    }

    if (bad) {   // keeps its previous x
      if (tid == 0) atomicAdd(nonpd, 1);
      __syncthreads();   // s_part is the next entity's
      continue;
    }

    // back substitution; thread tid owns fragment element tid of every tile:
    // row r = tid & 15 of the tile, column kk of the tile column
    {
      const int r = tid & 15;
      const int kk = ((tid >> 4) & 3) + 4 * (tid >> 6);
      for (int j = T - 1; j >= 0; --j) {
        double sum = 0.0;
        for (int i = j + 1; i < T; ++i) sum = fma(Ls[lt_off(i, j) + tid], s_x[16 * i + r], sum);
        sum = sum16(sum);
        if (r == 0) s_v[kk] = s_z[16 * j + kk] - sum;
        __syncthreads();
        const double t = sum16(Ls[lt_off(j, j) + tid] * s_v[r]);   // W_jj[r][kk] v[r]
        if (r == 0) s_x[16 * j + kk] = t;
        __syncthreads();
      }
    }
    for (int f = tid; f < 16 * T; f += 256) {
      const int n = ncoord(f, k, nb);
      if (n < k) x[e * ldk + n] = (float)s_x[f];
      else if (USER && n == k) xb[e] = (float)s_x[f];
    }
    __syncthreads();   // s_x, s_z and the slot are the next entity's
  }
}

}  // namespace

int64_t solve_slot_bytes(int K) {
  const int64_t T = (K + 15) / 16;
  return T * (T + 1) / 2 * 256 * (int64_t)sizeof(double);
}

int launch_solve_blocked(hipStream_t s, bool user_side, int64_t E, int k, double ridge,
                         const float* G, const float* Gs, const float* Gn, const float* C,
                         const float* Cb, float* x, float* xb, int* nonpd, double* scratch,
                         int slots) {
  if (E <= 0) return 0;
  MR_CHECK(k >= 1 && k <= kMaxKLarge, "the blocked exact solver runs 1 <= k <= 512");
  MR_CHECK(scratch && slots >= 1, "the blocked exact solver needs its scratch slots");
  const int64_t slot_doubles = solve_slot_bytes(user_side ? k + 1 : k) / (int64_t)sizeof(double);
  const unsigned grid = (unsigned)std::min<int64_t>(E, slots);
  if (user_side)
    MR_LAUNCH(solve_blocked_kernel<true>, dim3(grid), dim3(256), 0, s,
        E, k, ldk_of(k), ridge, G, Gs, Gn, C, Cb, x, xb, nonpd, scratch, slot_doubles);
  else
    MR_LAUNCH(solve_blocked_kernel<false>, dim3(grid), dim3(256), 0, s,
        E, k, ldk_of(k), ridge, G, Gs, Gn, C, Cb, x, xb, nonpd, scratch, slot_doubles);
  MR_HIP(hipGetLastError());
  return 0;
}

}  // namespace mr
