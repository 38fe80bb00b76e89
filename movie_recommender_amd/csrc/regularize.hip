// Regularised ALS (DESIGN.md "Regularised ALS"): the ridge pass over the
// tri16 normal equations, the device objective (training SSE + the two
// penalties) and the held-out squared error.  Nothing here touches the Gram
// or CG kernels: the pass runs between them, the objective beside them.
#include <algorithm>

#include "mr_internal.h"
#include "reduce_f64.h"

namespace mr {

// ---------------------------------------------------------------------------
// Ridge pass: G_e <- G_e + lambda w_e I_k on the k factor coordinates (the
// user bias -- Gs, Gn, C, Cb -- is not penalised).  w_e = 1 (constant) or
// the entity's rating count off[e+1] - off[e] (weighted, "ALS-WR").
//
// One thread per VIRTUAL factor index v = 16 b + r of an entity (ldk = 16 NB
// threads per entity, so a wave holds 64 / ldk entities or a 64-wide part of
// one): the 16 lanes of a group own the diagonal of one 16 x 16 diagonal
// block.  In the tri16 storage (mr_internal.h) that is, for an even block
// (and the unfolded last block of an odd NB), tile[r][r] -- 16 floats 68
// bytes apart, each on a 64-byte line of its own -- and for an odd block the
// 16 contiguous floats of the fold's side array (one or two lines).  Every
// line holding a diagonal entry is read and written once; nothing else of G
// moves.  Padding coordinates (natural index >= k) are not touched: they
// stay zero.  Each entry is rounded once: (float)((double)G_ii + lambda w_e),
// product and sum as separate fp64 operations (no fma contraction).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ridge_diag_kernel(int64_t E, int k, int nb, int64_t gsz,
                                                         double lambda, int weighted,
                                                         const int64_t* __restrict__ off,
                                                         float* __restrict__ G) {
  const int ldk = 16 * nb;
  const int64_t n = E * ldk;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = t / ldk;
    const int v = (int)(t - e * ldk);
    const int i = nat_of(v, nb);
    if (i >= k) continue;
    const int64_t cnt = weighted ? off[e + 1] - off[e] : 1;
    if (cnt == 0) continue;   // weighted, no ratings: G_e stays as it is (zero)
    float* g = G + e * gsz + packed_offset(i, i, nb);
    {
#pragma clang fp contract(off)   // two roundings in fp64, then one to fp32: no fma
      const double add = lambda * (double)cnt;
      *g = (float)((double)*g + add);
    }
  }
}

int launch_ridge_diag(hipStream_t s, int64_t E, int k, double lambda, bool weighted,
                      const int64_t* off, float* G) {
  if (E <= 0) return 0;
  const int nb = nb16_of(k);
  const int64_t n = E * 16 * nb;
  const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 8192);
  MR_LAUNCH(ridge_diag_kernel, dim3(grid), dim3(256), 0, s, E, k, nb, gsize_of(k), lambda,
            weighted ? 1 : 0, off, G);
  MR_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------
// Objective pieces (row loads and fixed-order fp64 sums: reduce_f64.h).
// ---------------------------------------------------------------------------
// Training SSE over the user-view CSR, walking the users' Gram work list: one
// wave per work item (a heavy user's chunks go to different waves), 64 / GL
// ratings at a time, kObjUnroll gathered V rows in flight per group.
// part[2 b] = sum (r - u.v - b_u)^2, part[2 b + 1] = ratings visited.
template <int GL>
__global__ __launch_bounds__(64 * kObjWaves) void objective_kernel(
    const WorkItem* __restrict__ work, int64_t n_work, const int32_t* __restrict__ idx,
    const float* __restrict__ val, const float* __restrict__ Uloc,
    const float* __restrict__ Ubloc, const float* __restrict__ V, int ldk,
    double* __restrict__ part) {
  constexpr int NG = 64 / GL;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int sub = lane % GL, grp = lane / GL;
  const int nq = ldk >> 2;
  const int64_t wi = (int64_t)blockIdx.x * kObjWaves + wave;
  double acc[2] = {0.0, 0.0};
  if (wi < n_work) {
    const WorkItem it = work[wi];
    const Row2 u = load_row<GL>(Uloc + (int64_t)it.entity * ldk, nq, sub, true);
    const double bu = (double)Ubloc[it.entity];
    for (int t0 = 0; t0 < it.len; t0 += NG * kObjUnroll) {
      Row2 v[kObjUnroll];
      float w[kObjUnroll];
#pragma unroll
      for (int j = 0; j < kObjUnroll; ++j) {
        const int t = t0 + j * NG + grp;
        const bool on = t < it.len;
        const int64_t at = it.begin + (on ? t : 0);
        const int64_t row = on ? (int64_t)idx[at] : 0;
        w[j] = on ? val[at] : 0.f;
        v[j] = load_row<GL>(V + row * ldk, nq, sub, on);
      }
#pragma unroll
      for (int j = 0; j < kObjUnroll; ++j) {
        const double d = group_sum<GL>(dot_rows<GL>(u, v[j]));
        const double e = (double)w[j] - d - bu;
        if (sub == 0 && t0 + j * NG + grp < it.len) acc[0] += e * e;
      }
    }
    if (lane == 0) acc[1] = (double)it.len;
  }
  block_partials<2>(acc, part);
}

// Penalty of one table: part[b] = the block's sum of w_e |x_e|^2 over rows
// e < E (x: the side's local rows; padding columns are zero), one lane group
// per row, a fixed grid.
template <int GL>
__global__ __launch_bounds__(64 * kObjWaves) void penalty_kernel(
    int64_t E, const float* __restrict__ X, int ldk, int weighted,
    const int64_t* __restrict__ off, double* __restrict__ part) {
  constexpr int NG = 64 * kObjWaves / GL;   // rows per block and round
  const int sub = threadIdx.x % GL, grp = threadIdx.x / GL;
  const int nq = ldk >> 2;
  double acc[1] = {0.0};
  for (int64_t e0 = (int64_t)blockIdx.x * NG; e0 < E; e0 += (int64_t)gridDim.x * NG) {
    const int64_t e = e0 + grp;
    const bool on = e < E;
    const Row2 x = load_row<GL>(X + (on ? e : 0) * ldk, nq, sub, on);
    const double s = group_sum<GL>(dot_rows<GL>(x, x));
    if (on && sub == 0) acc[0] += (weighted ? (double)(off[e + 1] - off[e]) : 1.0) * s;
  }
  block_partials<1>(acc, part);
}

// Held-out squared error of n (user, item, rating) triples (ids validated
// by the caller): part[b] = the block's sum of (r - u.v - b_u)^2.
template <int GL>
__global__ __launch_bounds__(64 * kObjWaves) void sse_kernel(
    int64_t n, const int32_t* __restrict__ uid, const int32_t* __restrict__ iid,
    const double* __restrict__ r, const float* __restrict__ U, const float* __restrict__ Ub,
    const float* __restrict__ V, int ldk, double* __restrict__ part) {
  constexpr int NG = 64 * kObjWaves / GL;
  const int sub = threadIdx.x % GL, grp = threadIdx.x / GL;
  const int nq = ldk >> 2;
  double acc[1] = {0.0};
  for (int64_t t0 = (int64_t)blockIdx.x * NG; t0 < n; t0 += (int64_t)gridDim.x * NG) {
    const int64_t t = t0 + grp;
    const bool on = t < n;
    const int64_t ur = on ? (int64_t)uid[t] : 0, ir = on ? (int64_t)iid[t] : 0;
    const Row2 u = load_row<GL>(U + ur * ldk, nq, sub, on);
    const Row2 v = load_row<GL>(V + ir * ldk, nq, sub, on);
    const double d = group_sum<GL>(dot_rows<GL>(u, v));
    if (on && sub == 0) {
      const double e = r[t] - d - (double)Ub[ur];
      acc[0] += e * e;
    }
  }
  block_partials<1>(acc, part);
}

// out[c] = sum over blocks b < nblk of part[nc b + c], in block order:
// thread t adds its contiguous run of blocks in order, thread 0 the 256 run
// sums in order -- a fixed association for a given nblk.
__global__ __launch_bounds__(256) void sum_partials_kernel(const double* __restrict__ part,
                                                           int64_t nblk, int nc,
                                                           double* __restrict__ out) {
  __shared__ double sm[256];
  const int64_t run = (nblk + 255) / 256;
  const int64_t lo = run * threadIdx.x;
  const int64_t b0 = lo < nblk ? lo : nblk;
  const int64_t b1 = b0 + run < nblk ? b0 + run : nblk;
  for (int c = 0; c < nc; ++c) {
    double s = 0.0;
    for (int64_t b = b0; b < b1; ++b) s += part[nc * b + c];
    sm[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      double tot = 0.0;
      for (int t = 0; t < 256; ++t) tot += sm[t];
      out[c] = tot;
    }
    __syncthreads();
  }
}

int launch_sum_partials(hipStream_t s, const double* part, int64_t nblk, int nc, double* out) {
  MR_LAUNCH(sum_partials_kernel, dim3(1), dim3(256), 0, s, part, nblk, nc, out);
  MR_HIP(hipGetLastError());
  return 0;
}

int64_t objective_blocks(int64_t n_work) { return (n_work + kObjWaves - 1) / kObjWaves; }

int64_t row_blocks(int64_t rows, int ldk) {
  const int64_t per = 64 * kObjWaves / lanes_for(ldk);
  return std::max<int64_t>(1, std::min<int64_t>((rows + per - 1) / per, kRowGridCap));
}

int launch_objective(hipStream_t s, const WorkItem* work, int64_t n_work, const int32_t* idx,
                     const float* val, const float* Uloc, const float* Ubloc, const float* V,
                     int ldk, double* part, double* out2) {
  MR_CHECK(ldk >= 16 && ldk % 16 == 0 && ldk <= 512, "objective: bad row stride");
  const int64_t nblk = objective_blocks(n_work);
  if (nblk > 0) {
#define MR_OBJ(GL)                                                                        \
  MR_LAUNCH(objective_kernel<GL>, dim3((unsigned)nblk), dim3(64 * kObjWaves), 0, s, work, \
            n_work, idx, val, Uloc, Ubloc, V, ldk, part)
    MR_BY_LANES(lanes_for(ldk), MR_OBJ)
#undef MR_OBJ
  }
  MR_LAUNCH(sum_partials_kernel, dim3(1), dim3(256), 0, s, part, nblk, 2, out2);
  MR_HIP(hipGetLastError());
  return 0;
}

int launch_penalty(hipStream_t s, int64_t E, const float* X, int ldk, bool weighted,
                   const int64_t* off, double* part, double* out1) {
  MR_CHECK(ldk >= 16 && ldk % 16 == 0 && ldk <= 512, "penalty: bad row stride");
  const int64_t nblk = E > 0 ? row_blocks(E, ldk) : 0;
  if (nblk > 0) {
#define MR_PEN(GL)                                                                         \
  MR_LAUNCH(penalty_kernel<GL>, dim3((unsigned)nblk), dim3(64 * kObjWaves), 0, s, E, X, ldk, \
            weighted ? 1 : 0, off, part)
    MR_BY_LANES(lanes_for(ldk), MR_PEN)
#undef MR_PEN
  }
  MR_LAUNCH(sum_partials_kernel, dim3(1), dim3(256), 0, s, part, nblk, 1, out1);
  MR_HIP(hipGetLastError());
  return 0;
}

int launch_sse(hipStream_t s, int64_t n, const int32_t* uid, const int32_t* iid, const double* r,
               const float* U, const float* Ub, const float* V, int ldk, double* part,
               double* out1) {
  MR_CHECK(ldk >= 16 && ldk % 16 == 0 && ldk <= 512, "sse: bad row stride");
  const int64_t nblk = n > 0 ? row_blocks(n, ldk) : 0;
  if (nblk > 0) {
#define MR_SSE(GL)                                                                         \
  MR_LAUNCH(sse_kernel<GL>, dim3((unsigned)nblk), dim3(64 * kObjWaves), 0, s, n, uid, iid, r, U, \
            Ub, V, ldk, part)
    MR_BY_LANES(lanes_for(ldk), MR_SSE)
#undef MR_SSE
  }
  MR_LAUNCH(sum_partials_kernel, dim3(1), dim3(256), 0, s, part, nblk, 1, out1);
  MR_HIP(hipGetLastError());
  return 0;
}

}  // namespace mr
