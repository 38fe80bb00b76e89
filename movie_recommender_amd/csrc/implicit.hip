// Implicit-feedback ALS (DESIGN.md "Implicit feedback"): Hu, Koren and
// Volinsky's confidence-weighted half-step on the engine's tri16 normal
// equations.  For an entity e with stored pairs j (opposite row y_j, stored
// value r_ej >= 0, w_ej = alpha r_ej) and S = Y^T Y over ALL opposite rows:
//   G_e = S + sum_j w_ej y_j y_j^T        c_e = sum_j (1 + w_ej) y_j
// Three kernels build that -- the weighted normal equations over the side's
// Gram work list (wnormal_kernel), S packed once in tri16 (yty_partial_kernel,
// yty_combine_kernel) and the add pass (add_s_kernel) -- and three more the
// objective's data term.  Everything behind the normal equations (slab_reduce,
// ridge pass, CG, Cholesky) is the explicit engine's, unchanged.
#include <algorithm>

#include "mr_internal.h"
#include "reduce_f64.h"

namespace mr {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Upper blocks (bi <= bj) of the NB x NB block grid, row-major.
__host__ __device__ constexpr int n_upper(int nb) { return nb * (nb + 1) / 2; }
__host__ __device__ constexpr int upper_index(int bi, int bj, int nb) {
  return bi * nb - bi * (bi - 1) / 2 + (bj - bi);
}

// NB contiguous floats (a lane's segment of a factor row), widest aligned loads.
template <int NB>
__device__ __forceinline__ void load_seg(const float* __restrict__ p, float (&y)[NB]) {
  if constexpr (NB % 4 == 0) {
#pragma unroll
    for (int q = 0; q < NB / 4; ++q) {
      const float4 v = reinterpret_cast<const float4*>(p)[q];
      y[4 * q] = v.x; y[4 * q + 1] = v.y; y[4 * q + 2] = v.z; y[4 * q + 3] = v.w;
    }
  } else if constexpr (NB % 2 == 0) {
#pragma unroll
    for (int q = 0; q < NB / 2; ++q) {
      const float2 v = reinterpret_cast<const float2*>(p)[q];
      y[2 * q] = v.x; y[2 * q + 1] = v.y;
    }
  } else {
#pragma unroll
    for (int q = 0; q < NB; ++q) y[q] = p[q];
  }
}

// One rank-4 update of every upper block: acc(bi, bj) += A_bi B_bj with
// A_b[i][kk] = a[b], B_b[kk][j] = y[b] of lane 16 kk + i (j).  The
// accumulator layout is the 16x16x4 f32 MFMA's: lane l holds rows
// 4 (l >> 4) + 0..3 of column l & 15.  MFMA: the exact f32-input matrix
// instruction; otherwise (k < 32) the same sums on the VALU, operands by
// cross-lane reads.
template <int NB, bool MFMA>
__device__ __forceinline__ void rank4_update(const float (&a)[NB], const float (&y)[NB],
                                             f32x4 (&acc)[n_upper(NB)], int lane) {
  if constexpr (MFMA) {
#pragma unroll
    for (int bi = 0; bi < NB; ++bi)
#pragma unroll
      for (int bj = bi; bj < NB; ++bj) {
        const int t = upper_index(bi, bj, NB);
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[bi], y[bj], acc[t], 0, 0, 0);
      }
  } else {
    const int col = lane & 15, r0 = 4 * (lane >> 4);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      float ar[NB][4], bc[NB];
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        bc[b] = __shfl(y[b], 16 * kk + col, 64);
#pragma unroll
        for (int r = 0; r < 4; ++r) ar[b][r] = __shfl(a[b], 16 * kk + r0 + r, 64);
      }
#pragma unroll
      for (int bi = 0; bi < NB; ++bi)
#pragma unroll
        for (int bj = bi; bj < NB; ++bj) {
          const int t = upper_index(bi, bj, NB);
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[t][r] = fmaf(ar[bi][r], bc[bj], acc[t][r]);
        }
    }
  }
}

// sum over rows t < len of w_t y_t y_t^T into acc (and of (1 + w_t) y_t into
// cacc), four rows per rank-4 update: lane 16 kk + i holds the NB floats
// y[NB i .. NB i + NB) of the update's row kk -- virtual columns 16 b + i, b <
// NB, the tri16 permutation (mr_internal.h).  Row ids and weights come 64 rows
// at a time (one coalesced load each, fetched one batch ahead) and are handed
// out by cross-lane reads; a step is UNR updates, and step s + 1's gathers are
// issued before step s's updates, so a wave that is alone on its SIMD (NB = 8
// holds 144 accumulator registers) still computes under its own loads.  Rows
// past the end are the table's all-zero row `zrow` with weight 0.
// DENSE: rows begin .. begin + len of F itself with weight 1 (S = F^T F), no rhs.
template <int NB, bool MFMA, bool DENSE>
__device__ __forceinline__ void accumulate_rows(int64_t begin, int len,
                                                const int32_t* __restrict__ idx,
                                                const float* __restrict__ val, float alpha,
                                                const float* __restrict__ F, int zrow, int lane,
                                                f32x4 (&acc)[n_upper(NB)], float (&cacc)[NB]) {
  constexpr int LD = 16 * NB;
  constexpr int UNR = NB <= 4 ? 4 : 2;
  constexpr int R = 4 * UNR;      // rows per step
  constexpr int SPB = 64 / R;     // steps per batch of 64 rows
  const int i = lane & 15, kk = lane >> 4;
  int id_cur, id_nxt;
  float w_cur = 0.f, w_nxt = 0.f;
  auto load_batch = [&](int b, int& id, float& w) {
    const int t = 64 * b + lane;
    const bool on = t < len;
    if constexpr (DENSE) {
      id = on ? (int)(begin + t) : zrow;
    } else {
      id = on ? idx[begin + t] : zrow;
      w = on ? alpha * val[begin + t] : 0.f;
    }
  };
  // step s of the batch held in (id_cur, w_cur); a step past the end gathers zrow
  auto fetch = [&](int s, float (&y)[UNR][NB], float (&w)[UNR]) {
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int src = (s % SPB) * R + 4 * u + kk;   // < 64
      const int row = __shfl(id_cur, src, 64);
      w[u] = __shfl(w_cur, src, 64);
      load_seg<NB>(F + (int64_t)row * LD + NB * i, y[u]);
    }
  };
  const int nsteps = (len + R - 1) / R;
  if (nsteps == 0) return;
  load_batch(0, id_cur, w_cur);
  load_batch(1, id_nxt, w_nxt);
  float ya[UNR][NB], wa[UNR], yb[UNR][NB], wb[UNR];
  fetch(0, ya, wa);
  for (int s = 0; s < nsteps; ++s) {
    if ((s + 1) % SPB == 0) {   // step s + 1 opens the next batch
      id_cur = id_nxt;
      w_cur = w_nxt;
      load_batch((s + 1) / SPB + 1, id_nxt, w_nxt);
    }
    fetch(s + 1, yb, wb);
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      if constexpr (DENSE) {
        rank4_update<NB, MFMA>(ya[u], ya[u], acc, lane);
      } else {
        float a[NB];
        const float w1 = 1.0f + wa[u];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          a[b] = wa[u] * ya[u][b];
          cacc[b] = fmaf(w1, ya[u][b], cacc[b]);
        }
        rank4_update<NB, MFMA>(a, ya[u], acc, lane);
      }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      wa[u] = wb[u];
#pragma unroll
      for (int b = 0; b < NB; ++b) ya[u][b] = yb[u][b];
    }
  }
}

// The accumulators as one tri16 block at Gt (mr_internal.h): strictly-upper
// tiles in full; diagonal blocks folded in pairs -- D_2m where col >= row,
// D_2m+1 where col < row, D_2m+1's diagonal in the side array; an odd last
// diagonal block in full.  Each store instruction writes four 64-byte rows.
template <int NB>
__device__ __forceinline__ void store_tri16(const f32x4 (&acc)[n_upper(NB)],
                                            float* __restrict__ Gt, int lane) {
  const int col = lane & 15, r0 = 4 * (lane >> 4);
#pragma unroll
  for (int bi = 0; bi < NB; ++bi)
#pragma unroll
    for (int bj = bi + 1; bj < NB; ++bj) {
      float* T = Gt + off_index(bi, bj, NB) * 256;
#pragma unroll
      for (int r = 0; r < 4; ++r) T[(r0 + r) * 16 + col] = acc[upper_index(bi, bj, NB)][r];
    }
  constexpr int base = NB * (NB - 1) / 2;   // n_off_of(NB)
#pragma unroll
  for (int m = 0; m < NB / 2; ++m) {
    float* T = Gt + (base + m) * 256;
    const f32x4 ev = acc[upper_index(2 * m, 2 * m, NB)];
    const f32x4 od = acc[upper_index(2 * m + 1, 2 * m + 1, NB)];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = r0 + r;
      T[row * 16 + col] = col >= row ? ev[r] : od[r];
      if (col == row) Gt[n_tiles_of(NB) * 256 + m * 16 + row] = od[r];
    }
  }
  if constexpr (NB & 1) {
    float* T = Gt + (base + NB / 2) * 256;
#pragma unroll
    for (int r = 0; r < 4; ++r) T[(r0 + r) * 16 + col] = acc[upper_index(NB - 1, NB - 1, NB)][r];
  }
}

// ---------------------------------------------------------------------------
// Weighted normal equations: one wave per Gram work item, four per block.
// Writes sum w y y^T (tri16) and sum (1 + w) y to the item's entity (direct)
// or slab record, as the explicit Gram does; the user side's bias slots (Gs,
// Cb, Gn) are written as zero so that slab_reduce sums defined values -- the
// add pass sets them afterwards.
// ---------------------------------------------------------------------------
template <int NB, bool MFMA>
__global__ __launch_bounds__(256) void wnormal_kernel(
    const WorkItem* __restrict__ work, int64_t n_work, const int32_t* __restrict__ idx,
    const float* __restrict__ val, float alpha, const float* __restrict__ F, int zrow, int user,
    GramDst direct, GramDst slab) {
  const int lane = threadIdx.x & 63;
  const int64_t wi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wi >= n_work) return;
  const WorkItem it = work[wi];
  f32x4 acc[n_upper(NB)];
#pragma unroll
  for (int t = 0; t < n_upper(NB); ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  float cacc[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) cacc[b] = 0.f;
  accumulate_rows<NB, MFMA, false>(it.begin, it.len, idx, val, alpha, F, zrow, lane, acc, cacc);
  const bool to_slab = it.slab >= 0;
  const int64_t di = to_slab ? (int64_t)it.slab : (int64_t)it.entity;
  const GramDst& D = to_slab ? slab : direct;
  store_tri16<NB>(acc, D.G + di * D.sG, lane);
  // rhs: the four row groups of a step hold the same columns
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    cacc[b] += __shfl_xor(cacc[b], 16, 64);
    cacc[b] += __shfl_xor(cacc[b], 32, 64);
  }
  if (lane < 16) {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      D.C[di * D.sV + NB * lane + b] = cacc[b];   // natural column of virtual (b, lane)
      if (user) D.Gs[di * D.sV + NB * lane + b] = 0.f;
    }
  }
  if (user && lane == 0) {
    D.Cb[di * D.sS] = 0.f;
    D.Gn[di * D.sS] = 0.f;
  }
}

int launch_wnormal(hipStream_t s, bool user_side, int k, const WorkItem* work, int64_t n_work,
                   const int32_t* idx, const float* val, float alpha, const float* F, int zrow,
                   GramDst direct, GramDst slab) {
  MR_CHECK(k >= 1 && k <= kMaxK, "implicit feedback needs k <= 128");
  if (n_work <= 0) return 0;
  const dim3 grid((unsigned)((n_work + 3) / 4));
  const int user = user_side ? 1 : 0;
#define MR_WN(NB, MF)                                                                        \
  MR_LAUNCH((wnormal_kernel<NB, MF>), grid, dim3(256), 0, s, work, n_work, idx, val, alpha, F, \
            zrow, user, direct, slab)
  const bool mfma = k >= kMfmaMinK;
  switch (nb16_of(k)) {
    case 1: MR_WN(1, false); break;
    case 2: if (mfma) MR_WN(2, true); else MR_WN(2, false); break;
    case 3: MR_WN(3, true); break;
    case 4: MR_WN(4, true); break;
    case 5: MR_WN(5, true); break;
    case 6: MR_WN(6, true); break;
    case 7: MR_WN(7, true); break;
    default: MR_WN(8, true); break;
  }
#undef MR_WN
  MR_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------
// S = F^T F over all `rows` rows of a factor table, packed in tri16.  Wave p
// of n_part sums rows [p rows / n_part, (p + 1) rows / n_part) in fp32 (the
// weighted kernel's accumulation with weight 1) into part[p]; the combine
// kernel adds the n_part partials of every tri16 word in a fixed order in fp64
// and rounds once.  Fixed grid, fixed order: the same table gives the same bits.
// ---------------------------------------------------------------------------
template <int NB, bool MFMA>
__global__ __launch_bounds__(256) void yty_partial_kernel(const float* __restrict__ F,
                                                          int64_t rows, int n_part,
                                                          float* __restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= n_part) return;
  const int64_t r0 = rows * p / n_part, r1 = rows * (p + 1) / n_part;
  f32x4 acc[n_upper(NB)];
#pragma unroll
  for (int t = 0; t < n_upper(NB); ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  float unused[NB];
  accumulate_rows<NB, MFMA, true>(r0, (int)(r1 - r0), nullptr, nullptr, 0.f, F, (int)rows, lane,
                                  acc, unused);
  store_tri16<NB>(acc, part + (int64_t)p * gsize_of(16 * NB), lane);
}

// 64 tri16 words x 4 slices of the partials per block: slice q adds its
// contiguous run of partials in order, then the four slice sums are added in
// slice order.
__global__ __launch_bounds__(256) void yty_combine_kernel(const float* __restrict__ part,
                                                          int n_part, int64_t gsz,
                                                          float* __restrict__ S16) {
  __shared__ double sm[4][64];
  const int w = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int64_t t = (int64_t)blockIdx.x * 64 + w;
  const int run = (n_part + 3) / 4;
  const int p0 = min(run * q, n_part), p1 = min(p0 + run, n_part);
  double s = 0.0;
  if (t < gsz)
    for (int p = p0; p < p1; ++p) s += (double)part[(int64_t)p * gsz + t];
  sm[q][w] = s;
  __syncthreads();
  if (q == 0 && t < gsz) S16[t] = (float)(((sm[0][w] + sm[1][w]) + sm[2][w]) + sm[3][w]);
}

int yty_parts(int64_t rows) {
  return (int)std::max<int64_t>(1, std::min<int64_t>((rows + 63) / 64, 512));
}

// F: rows + 1 rows of ldk floats, row `rows` all zero (the engine's tables).
int launch_yty16(hipStream_t s, int k, const float* F, int64_t rows, float* part, float* S16) {
  MR_CHECK(k >= 1 && k <= kMaxK, "implicit feedback needs k <= 128");
  MR_CHECK(rows < (int64_t)1 << 31, "too many rows");
  const int n_part = yty_parts(rows);
  const dim3 grid((unsigned)((n_part + 3) / 4));
#define MR_YTY(NB, MF) \
  MR_LAUNCH((yty_partial_kernel<NB, MF>), grid, dim3(256), 0, s, F, rows, n_part, part)
  const bool mfma = k >= kMfmaMinK;
  switch (nb16_of(k)) {
    case 1: MR_YTY(1, false); break;
    case 2: if (mfma) MR_YTY(2, true); else MR_YTY(2, false); break;
    case 3: MR_YTY(3, true); break;
    case 4: MR_YTY(4, true); break;
    case 5: MR_YTY(5, true); break;
    case 6: MR_YTY(6, true); break;
    case 7: MR_YTY(7, true); break;
    default: MR_YTY(8, true); break;
  }
#undef MR_YTY
  const int64_t gsz = gsize_of(k);
  MR_LAUNCH(yty_combine_kernel, dim3((unsigned)((gsz + 63) / 64)), dim3(256), 0, s, part,
            n_part, gsz, S16);
  MR_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------
// Add pass: G_e[t] = fl32(G_e[t] + S16[t]) for every local entity and tri16
// word -- S is pre-packed, so this is one coalesced elementwise pass (a block
// is 64 float4 columns x 4 entities; each thread keeps its S words and walks
// the entities).  User side: the bias slots of every entity are set to
// Gs_e = 0, Gn_e = 1, Cb_e = 0, which pins the bias at exactly zero in both
// solvers.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void add_s_kernel(int64_t E, int64_t gsz4, int ldk,
                                                    const float4* __restrict__ S4,
                                                    float4* __restrict__ G4,
                                                    float* __restrict__ Gs,
                                                    float* __restrict__ Gn,
                                                    float* __restrict__ Cb) {
  const int64_t c = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63);
  const int64_t ey = (int64_t)blockIdx.y * 4 + (threadIdx.x >> 6);
  const int64_t estep = (int64_t)gridDim.y * 4;
  if (c < gsz4) {
    const float4 sv = S4[c];
    for (int64_t e = ey; e < E; e += estep) {
      float4 g = G4[e * gsz4 + c];
      g.x += sv.x; g.y += sv.y; g.z += sv.z; g.w += sv.w;
      G4[e * gsz4 + c] = g;
    }
  }
  if (Gs) {   // user side
    const int64_t tid = ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 256 + threadIdx.x;
    const int64_t nth = (int64_t)gridDim.x * gridDim.y * 256;
    for (int64_t t = tid; t < E * ldk; t += nth) Gs[t] = 0.f;
    for (int64_t e = tid; e < E; e += nth) {
      Gn[e] = 1.f;
      Cb[e] = 0.f;
    }
  }
}

int launch_add_s(hipStream_t s, int64_t E, int k, const float* S16, float* G, float* Gs,
                 float* Gn, float* Cb) {
  if (E <= 0) return 0;
  const int64_t gsz4 = gsize_of(k) / 4;
  const dim3 grid((unsigned)((gsz4 + 63) / 64),
                  (unsigned)std::max<int64_t>(1, std::min<int64_t>((E + 3) / 4, 1024)));
  MR_LAUNCH(add_s_kernel, grid, dim3(256), 0, s, E, gsz4, ldk_of(k),
            reinterpret_cast<const float4*>(S16), reinterpret_cast<float4*>(G), Gs, Gn, Cb);
  MR_HIP(hipGetLastError());
  return 0;
}

// flag = 1 if any of n values is negative (or not a number)
__global__ __launch_bounds__(256) void any_negative_kernel(int64_t n,
                                                           const float* __restrict__ val,
                                                           int* __restrict__ flag) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n;
       t += (int64_t)gridDim.x * blockDim.x)
    if (!(val[t] >= 0.f)) *flag = 1;
}

int launch_any_negative(hipStream_t s, int64_t n, const float* val, int* flag) {
  if (n <= 0) return 0;
  const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 4096);
  MR_LAUNCH(any_negative_kernel, dim3(grid), dim3(256), 0, s, n, val, flag);
  MR_HIP(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------
// Objective.  The loss over ALL (u, i) pairs is
//   J_data = sum_u x_u^T S x_u + sum_obs [(1 + w)(1 - d)^2 - d^2],  d = x_u . y_i,
// S = Y^T Y (items), w = alpha r.  Both terms in fp64 with fixed reduction
// orders (reduce_f64.h).
// ---------------------------------------------------------------------------
// Observed term over the users' work list (objective_kernel's walk):
// part[2 b] = sum (1 + w)(1 - d)^2 - d^2, part[2 b + 1] = pairs visited.
template <int GL>
__global__ __launch_bounds__(64 * kObjWaves) void implicit_obs_kernel(
    const WorkItem* __restrict__ work, int64_t n_work, const int32_t* __restrict__ idx,
    const float* __restrict__ val, double alpha, const float* __restrict__ Uloc,
    const float* __restrict__ V, int ldk, double* __restrict__ part) {
  constexpr int NG = 64 / GL;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int sub = lane % GL, grp = lane / GL;
  const int nq = ldk >> 2;
  const int64_t wi = (int64_t)blockIdx.x * kObjWaves + wave;
  double acc[2] = {0.0, 0.0};
  if (wi < n_work) {
    const WorkItem it = work[wi];
    const Row2 u = load_row<GL>(Uloc + (int64_t)it.entity * ldk, nq, sub, true);
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
        const double c = 1.0 + alpha * (double)w[j];
        const double e = 1.0 - d;
        if (sub == 0 && t0 + j * NG + grp < it.len) acc[0] += c * e * e - d * d;
      }
    }
    if (lane == 0) acc[1] = (double)it.len;
  }
  block_partials<2>(acc, part);
}

// fp64 S = F^T F, natural ldk x ldk: block b sums rows [b rows / nblk, ...)
// into part[b] (16-row chunks staged in LDS; thread t owns entries t + 256 q).
template <int NB>
__global__ __launch_bounds__(256) void yty64_partial_kernel(const float* __restrict__ F,
                                                            int64_t rows,
                                                            double* __restrict__ part) {
  constexpr int LD = 16 * NB, NQ = NB * NB, CH = 16;
  __shared__ float sh[CH][LD];
  const int64_t r0 = rows * blockIdx.x / gridDim.x, r1 = rows * (blockIdx.x + 1) / gridDim.x;
  double acc[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
  for (int64_t rb = r0; rb < r1; rb += CH) {
    const int n = r1 - rb < CH ? (int)(r1 - rb) : CH;
    __syncthreads();
    for (int t = threadIdx.x; t < n * LD; t += 256) sh[t / LD][t % LD] = F[rb * LD + t];
    __syncthreads();
    for (int r = 0; r < n; ++r) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int e = threadIdx.x + 256 * q;
        acc[q] += (double)sh[r][e / LD] * (double)sh[r][e % LD];
      }
    }
  }
  double* out = part + (int64_t)blockIdx.x * (LD * LD);
#pragma unroll
  for (int q = 0; q < NQ; ++q) out[threadIdx.x + 256 * q] = acc[q];
}

__global__ __launch_bounds__(256) void yty64_combine_kernel(const double* __restrict__ part,
                                                            int nblk, int n,
                                                            double* __restrict__ S) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += part[(int64_t)b * n + t];
  S[t] = s;
}

// part[b] = the block's sum of x_e^T S x_e: one wave per row (row e of wave
// slot e mod (4 gridDim.x), in row order), lane l the columns l, l + 64.
__global__ __launch_bounds__(64 * kObjWaves) void xsx_kernel(int64_t E,
                                                             const float* __restrict__ X,
                                                             int ldk,
                                                             const double* __restrict__ S,
                                                             double* __restrict__ part) {
  __shared__ float xs[kObjWaves][kMaxK];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double acc[1] = {0.0};
  for (int64_t e = (int64_t)blockIdx.x * kObjWaves + wave; e < E;
       e += (int64_t)gridDim.x * kObjWaves) {
    __builtin_amdgcn_wave_barrier();
    for (int j = lane; j < ldk; j += 64) xs[wave][j] = X[e * ldk + j];
    __builtin_amdgcn_wave_barrier();
    for (int j = lane; j < ldk; j += 64) {
      double t = 0.0;
      for (int i = 0; i < ldk; ++i) t += (double)xs[wave][i] * S[(int64_t)i * ldk + j];
      acc[0] += (double)xs[wave][j] * t;
    }
  }
  block_partials<1>(acc, part);
}

int64_t yty64_blocks(int64_t rows) {
  return std::max<int64_t>(1, std::min<int64_t>((rows + 63) / 64, 256));
}

// out2 = {observed term, pairs visited}; work: 2 objective_blocks(n_work) doubles.
int launch_implicit_obs(hipStream_t s, const WorkItem* work, int64_t n_work, const int32_t* idx,
                        const float* val, double alpha, const float* Uloc, const float* V,
                        int ldk, double* part, double* out2) {
  MR_CHECK(ldk >= 16 && ldk % 16 == 0 && ldk <= kMaxK, "implicit objective: bad row stride");
  const int64_t nblk = objective_blocks(n_work);
  if (nblk > 0) {
#define MR_IOBJ(GL)                                                                          \
  MR_LAUNCH(implicit_obs_kernel<GL>, dim3((unsigned)nblk), dim3(64 * kObjWaves), 0, s, work, \
            n_work, idx, val, alpha, Uloc, V, ldk, part)
    MR_BY_LANES(lanes_for(ldk), MR_IOBJ)
#undef MR_IOBJ
  }
  return launch_sum_partials(s, part, nblk, 2, out2);
}

// out1 = sum over E rows of X of x^T (Y^T Y) x, Y: `rows` rows.  part:
// yty64_blocks(rows) ldk^2 doubles, then row_blocks(E, ldk); S64: ldk^2.
int launch_xsx(hipStream_t s, int k, const float* Y, int64_t rows, int64_t E, const float* X,
               double* part, double* S64, double* out1) {
  MR_CHECK(k >= 1 && k <= kMaxK, "implicit feedback needs k <= 128");
  const int ldk = ldk_of(k), n = ldk * ldk;
  const int64_t nb_s = yty64_blocks(rows);
#define MR_Y64(NB) \
  MR_LAUNCH(yty64_partial_kernel<NB>, dim3((unsigned)nb_s), dim3(256), 0, s, Y, rows, part)
  switch (nb16_of(k)) {
    case 1: MR_Y64(1); break;
    case 2: MR_Y64(2); break;
    case 3: MR_Y64(3); break;
    case 4: MR_Y64(4); break;
    case 5: MR_Y64(5); break;
    case 6: MR_Y64(6); break;
    case 7: MR_Y64(7); break;
    default: MR_Y64(8); break;
  }
#undef MR_Y64
  MR_LAUNCH(yty64_combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part,
            (int)nb_s, n, S64);
  double* xpart = part + nb_s * n;
  const int64_t nb_x = E > 0 ? row_blocks(E, ldk) : 0;
  if (nb_x > 0)
    MR_LAUNCH(xsx_kernel, dim3((unsigned)nb_x), dim3(64 * kObjWaves), 0, s, E, X, ldk, S64,
              xpart);
  return launch_sum_partials(s, xpart, nb_x, 1, out1);
}

}  // namespace mr
