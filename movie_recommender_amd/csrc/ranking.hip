// Ranking evaluation and implicit fold-in on MI355X (gfx950).
// C ABI: include/mr_ranking.h.  DESIGN.md "Ranking evaluation and implicit
// fold-in".
//
// Rank counts: for every held-out (user, item) pair the number of the user's
// eligible items that score above / equal to it.  Scores are the fp64
// expression of serving.hip (sum from 0 in index order, separate multiply and
// add, + bias, + offset), formed tile by tile and compared in registers; no
// score is stored.  A pair's threshold comes from a gather-dot with the same
// summation, so the tile's own (u, i) entry equals it bit for bit.
//
// Exclusions are SUBTRACTED: the tile kernel counts over all items, the
// excluded items are scored by the same gather-dot and taken out of the
// counts of their user's pairs afterwards (bit-equal scores again, so what is
// subtracted is exactly what the tile kernel added).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/mr_als.h"
#include "../../include/mr_ranking.h"
#include "mr_internal.h"

namespace mr {

// separately rounded multiply and add (serving.hip mul_rn / add_rn)
__device__ __forceinline__ double rk_mul(double a, double b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ double rk_add(double a, double b) {
#pragma clang fp contract(off)
  return a + b;
}

__device__ __forceinline__ double lane_value(double v, int lane) {   // lane: wave-uniform
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), lane);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// ---------------------------------------------------------------------------
// K-R1: score of n (user, item) pairs, one thread per pair, the reference
// order.  COUNTS: the pair is a test pair -- its counters are initialised
// (tied starts at -1: the tile kernel meets the pair's own item once, with an
// equal score, unless the score is NaN and compares equal to nothing).
// ---------------------------------------------------------------------------
template <bool COUNTS>
__global__ __launch_bounds__(256) void rank_pair_score_kernel(
    int64_t n, int k, const double* __restrict__ X, const double* __restrict__ bias,
    const double* __restrict__ Y, const double* __restrict__ moff,
    const int* __restrict__ user_of, const int* __restrict__ item, double* __restrict__ score,
    int* __restrict__ above, int* __restrict__ tied, int* __restrict__ tbefore) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const int u = user_of[p], i = item[p];
  const double* x = X + (int64_t)u * k;
  const double* y = Y + (int64_t)i * k;
  double s = 0.0;
  int j = 0;
  for (; j + 4 <= k; j += 4) {   // 8 loads in flight, the adds in index order
    double a[4], b[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      a[t] = x[j + t];
      b[t] = y[j + t];
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) s = rk_add(s, rk_mul(a[t], b[t]));
  }
  for (; j < k; ++j) s = rk_add(s, rk_mul(x[j], y[j]));
  s = rk_add(rk_add(s, bias[u]), moff[i]);
  score[p] = s;
  if constexpr (COUNTS) {
    above[p] = 0;
    tied[p] = (s != s) ? 0 : -1;
    tbefore[p] = 0;
  }
}

// Order-preserving 64-bit key of a score that is not NaN (larger score ->
// larger key; -0.0 and +0.0 share a key, as they compare equal).  No such key
// is ~0: that one stands for a NaN threshold, which nothing reaches or equals.
__device__ __forceinline__ uint64_t rk_key(double s) {
  if (s == 0.0) s = 0.0;
  const uint64_t b = (uint64_t)__double_as_longlong(s);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

constexpr int RK_U = 32, RK_C = 256, RK_KC = 16, RK_LC = 2048;
constexpr uint32_t RK_PAD = 0x7fffffffu;

// A user's pairs take the sorted path when they lie inside the first
// lds_pairs pair slots of their 32-user tile (slot = pair - first pair of the
// tile); the other users take the compare path.  Both kernels below use this.
__device__ __forceinline__ bool rk_sorted_user(const int64_t* toff, int u, int lds_pairs) {
  return toff[u + 1] - toff[u / RK_U * RK_U] <= lds_pairs;
}

// ---------------------------------------------------------------------------
// K-R1s: a sorted-path user's thresholds as keys in ascending (key, pair)
// order, one block per user: bitonic sort in LDS.  skey / sidx are aligned
// with the pairs; sidx[r] = the pair (offset inside the user's list) at sorted
// position r.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rank_sort_kernel(int lds_pairs,
                                                        const int64_t* __restrict__ toff,
                                                        const double* __restrict__ thr,
                                                        uint64_t* __restrict__ skey,
                                                        int* __restrict__ sidx) {
  __shared__ uint64_t sk[RK_LC];
  __shared__ uint32_t si[RK_LC];
  const int u = blockIdx.x, tid = threadIdx.x;
  const int64_t beg = toff[u], end = toff[u + 1];
  if (beg == end || !rk_sorted_user(toff, u, lds_pairs)) return;   // block-uniform
  const int n = (int)(end - beg);   // <= lds_pairs <= RK_LC
  int sz = 2;
  while (sz < n) sz <<= 1;
  for (int i = tid; i < sz; i += 256) {
    uint64_t key = ~0ull;
    if (i < n) {
      const double t = thr[beg + i];
      if (t == t) key = rk_key(t);
    }
    sk[i] = key;
    si[i] = i < n ? (uint32_t)i : RK_PAD;
  }
  __syncthreads();
  for (int w = 2; w <= sz; w <<= 1) {
    for (int j = w >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < sz; i += 256) {
        const int l = i ^ j;
        if (l > i) {
          const bool up = (i & w) == 0;
          const uint64_t ka = sk[i], kb = sk[l];
          const uint32_t ma = si[i], mb = si[l];
          const bool a_greater = ka > kb || (ka == kb && ma > mb);
          if (a_greater == up) {
            sk[i] = kb;
            sk[l] = ka;
            si[i] = mb;
            si[l] = ma;
          }
        }
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < n; i += 256) {
    skey[beg + i] = sk[i];
    sidx[beg + i] = (int)si[i];
  }
}

// ---------------------------------------------------------------------------
// K-R2: counts of a tile of 32 users x 256 items.  The score part is
// rec_score_kernel's (serving.hip K-S1): thread (tx = lane, ty = wave) owns
// users ty*8 .. ty*8+7 and items tx + 64q, 32 fp64 accumulators, k staged 16
// factors at a time, one chunk ahead.  Block (bx, by) walks item tiles by,
// by + gridDim.y, ... for user tile bx.
//
// Epilogue per user (wave-uniform), sorted path: the user's sorted threshold
// keys sit in LDS; every lane finds, for each of its 4 scores, the number lo
// of thresholds below it by a branch-free binary search (the same steps in
// every lane) and adds 1 to the user's LDS histogram at lo - 1: "this item is
// above the pairs at sorted positions 0 .. lo-1".  A score that equals a
// threshold (rare) adds to tied / tied_before of those pairs in memory.  When
// the block has walked its item tiles, above = the suffix sum of the
// histogram, added to memory once per pair.
//
// Compare path (users whose pairs do not fit the LDS slots; any number of
// pairs): the pairs are walked 64 at a time -- lane l holds pair l's threshold
// and item id and its three counters; for each pair the wave compares its 256
// scores with the threshold (the compare masks are the ballots, counted on
// the scalar unit) and lane l adds the totals, then adds them to memory.
//
// A user belongs to one wave, so LDS slots are never shared between waves.
// Items past n_items score NaN: no compare holds, and NaN scores are skipped.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rank_count_kernel(
    int n_users, int n_items, int k, int n_item_tiles, int lds_pairs,
    const double* __restrict__ X, const double* __restrict__ bias,
    const double* __restrict__ Y, const double* __restrict__ moff,
    const int64_t* __restrict__ toff, const double* __restrict__ thr,
    const int* __restrict__ titem, const uint64_t* __restrict__ skey,
    const int* __restrict__ sidx, int* __restrict__ above, int* __restrict__ tied,
    int* __restrict__ tbefore) {
  __shared__ __attribute__((aligned(16))) double xs[RK_KC][RK_U + 2];
  __shared__ double vs[RK_KC][RK_C + 1];
  __shared__ uint64_t skeys[RK_LC];
  __shared__ int hist[RK_LC];
  const int tid = threadIdx.x, tx = tid & 63, ty = tid >> 6;
  const int u0 = blockIdx.x * RK_U;
  // first and one-past-last test pair of this user tile: nothing to count
  // for a tile without test pairs (block-uniform exit before any barrier)
  const int64_t pbase = toff[u0], pend = toff[min(u0 + RK_U, n_users)];
  if (pbase == pend) return;
  const int nl = (int)min((int64_t)lds_pairs, pend - pbase);
  for (int i = tid; i < nl; i += 256) {   // visible after the first barrier below
    skeys[i] = skey[pbase + i];           // (slots of compare-path users: unused)
    hist[i] = 0;
  }
  const int jj = tid & 15, rr = tid >> 4;
  for (int it = blockIdx.y; it < n_item_tiles; it += gridDim.y) {
    const int c0 = it * RK_C;
    double acc[8][4];
#pragma unroll
    for (int p = 0; p < 8; ++p)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[p][q] = 0.0;
    double vreg[RK_C / 16], xreg[2];
    auto load_chunk = [&](int j0) {
      const int kc = min(RK_KC, k - j0);
      const bool jok = jj < kc;
      const double* src = Y + (int64_t)(c0 + rr) * k + j0 + jj;
#pragma unroll
      for (int i = 0; i < RK_C / 16; ++i) {
        const bool ok = jok && (c0 + rr + 16 * i) < n_items;
        vreg[i] = ok ? src[(int64_t)16 * i * k] : 0.0;
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int u = u0 + rr + 16 * i;
        xreg[i] = (jok && u < n_users) ? X[(int64_t)u * k + j0 + jj] : 0.0;
      }
    };
    load_chunk(0);
    for (int j0 = 0; j0 < k; j0 += RK_KC) {
      const int kc = min(RK_KC, k - j0);
#pragma unroll
      for (int i = 0; i < RK_C / 16; ++i) vs[jj][rr + 16 * i] = vreg[i];
#pragma unroll
      for (int i = 0; i < 2; ++i) xs[jj][rr + 16 * i] = xreg[i];
      __syncthreads();
      if (j0 + RK_KC < k) load_chunk(j0 + RK_KC);
      for (int j = 0; j < kc; ++j) {
        double xv[8], vv[4];
        const double2* xp = reinterpret_cast<const double2*>(&xs[j][ty * 8]);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const double2 t = xp[p];
          xv[2 * p] = t.x;
          xv[2 * p + 1] = t.y;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) vv[q] = vs[j][tx + 64 * q];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          double pr[4][4];
#pragma unroll
          for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) pr[p][q] = rk_mul(xv[4 * h + p], vv[q]);
#pragma unroll
          for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[4 * h + p][q] = rk_add(acc[4 * h + p][q], pr[p][q]);
        }
      }
      __syncthreads();
    }
    double medv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = c0 + tx + 64 * q;
      medv[q] = moff[c < n_items ? c : n_items - 1];
    }
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      const int u = __builtin_amdgcn_readfirstlane(u0 + ty * 8 + p);   // wave-uniform
      if (u >= n_users) continue;
      const int64_t beg = toff[u], end = toff[u + 1];
      if (beg == end) continue;
      const double bu = bias[u];
      double s[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double v = rk_add(rk_add(acc[p][q], bu), medv[q]);
        s[q] = (c0 + tx + 64 * q) < n_items ? v : NAN;
      }
      if (end - pbase <= lds_pairs) {   // sorted path
        const int slot0 = (int)(beg - pbase), n = (int)(end - beg);
        const uint64_t* ks = skeys + slot0;
        uint64_t key[4];
        int lo[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          key[q] = rk_key(s[q]);
          lo[q] = 0;
        }
        int len = n;   // lower bound: lo = number of thresholds below the score
        while (len > 1) {
          const int half = len >> 1;
#pragma unroll
          for (int q = 0; q < 4; ++q) lo[q] += ks[lo[q] + half - 1] < key[q] ? half : 0;
          len -= half;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) lo[q] += ks[lo[q]] < key[q] ? 1 : 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (!(s[q] == s[q])) continue;
          if (lo[q] > 0) atomicAdd(&hist[slot0 + lo[q] - 1], 1);
          for (int r = lo[q]; r < n && ks[r] == key[q]; ++r) {   // ties
            const int64_t pi = beg + sidx[beg + r];
            atomicAdd(&tied[pi], 1);
            if (c0 + tx + 64 * q > titem[pi]) atomicAdd(&tbefore[pi], 1);
          }
        }
        continue;
      }
      for (int64_t pc = beg; pc < end; pc += 64) {   // compare path
        const int n = (int)min((int64_t)64, end - pc);
        const double my_t = tx < n ? thr[pc + tx] : NAN;
        const int my_i = tx < n ? titem[pc + tx] : 0;
        int ca = 0, ce = 0, cb = 0;
        for (int pl = 0; pl < n; ++pl) {
          const double t = lane_value(my_t, pl);
          const int ti = __builtin_amdgcn_readlane(my_i, pl);
          int na = 0, ng = 0, nb = 0;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const unsigned long long mgt = __ballot(s[q] > t);
            const unsigned long long mge = __ballot(s[q] >= t);
            na += __popcll(mgt);
            ng += __popcll(mge);
            if (mge != mgt)   // ties are rare: the id compare only then
              nb += __popcll(__ballot(s[q] == t && (c0 + tx + 64 * q) > ti));
          }
          if (tx == pl) {
            ca += na;
            ce += ng - na;
            cb += nb;
          }
        }
        if (tx < n) {
          if (ca) atomicAdd(&above[pc + tx], ca);
          if (ce) atomicAdd(&tied[pc + tx], ce);
          if (cb) atomicAdd(&tbefore[pc + tx], cb);
        }
      }
    }
  }
  __syncthreads();
  // above = suffix sums of the histogram, per sorted-path user (wave ty's 8)
  for (int p = 0; p < 8; ++p) {
    const int u = u0 + ty * 8 + p;
    if (u >= n_users) break;
    const int64_t beg = toff[u], end = toff[u + 1];
    if (beg == end || end - pbase > lds_pairs) continue;
    const int slot0 = (int)(beg - pbase), n = (int)(end - beg);
    int carry = 0;   // histogram total of the positions after this chunk
    for (int base = (n - 1) / 64 * 64; base >= 0; base -= 64) {
      const int r = base + tx;
      int v = r < n ? hist[slot0 + r] : 0;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_down(v, o, 64);
        if (tx + o < 64) v += t;
      }
      const int a = v + carry;
      if (r < n && a) atomicAdd(&above[beg + sidx[beg + r]], a);
      carry += __shfl(v, 0, 64);
    }
  }
}

// ---------------------------------------------------------------------------
// K-R3: the excluded items leave the counts.  One block per user: the user's
// excluded scores go through LDS RK_EX at a time, thread t owns test pairs
// t, t + 256, ... and subtracts what the tile kernel counted for them.
// ---------------------------------------------------------------------------
constexpr int RK_EX = 1024;

__global__ __launch_bounds__(256) void rank_exclude_kernel(
    const int64_t* __restrict__ toff, const double* __restrict__ thr,
    const int* __restrict__ titem, const int64_t* __restrict__ eoff,
    const double* __restrict__ escore, const int* __restrict__ eitem, int* __restrict__ above,
    int* __restrict__ tied, int* __restrict__ tbefore) {
  __shared__ double es[RK_EX];
  __shared__ int ei[RK_EX];
  const int u = blockIdx.x, tid = threadIdx.x;
  const int64_t tb = toff[u], te = toff[u + 1], eb = eoff[u], ee = eoff[u + 1];
  if (tb == te || eb == ee) return;   // block-uniform
  for (int64_t e0 = eb; e0 < ee; e0 += RK_EX) {
    const int ne = (int)min((int64_t)RK_EX, ee - e0);
    __syncthreads();
    for (int i = tid; i < ne; i += 256) {
      es[i] = escore[e0 + i];
      ei[i] = eitem[e0 + i];
    }
    __syncthreads();
    for (int64_t p = tb + tid; p < te; p += 256) {
      const double t = thr[p];
      const int ti = titem[p];
      int a = 0, e = 0, b = 0;
      for (int i = 0; i < ne; ++i) {
        const double s = es[i];
        a += s > t ? 1 : 0;
        const bool eq = s == t;
        e += eq ? 1 : 0;
        b += (eq && ei[i] > ti) ? 1 : 0;
      }
      if (a) above[p] -= a;
      if (e) tied[p] -= e;
      if (b) tbefore[p] -= b;
    }
  }
}

// ---------------------------------------------------------------------------
// Implicit fold-in
// ---------------------------------------------------------------------------
// K-F1: fp64 S = Y^T Y, natural k x k.  Block (b, g) sums rows
// [rows b / nblk, rows (b+1) / nblk) in row order into entries 2048 g ..
// 2048 g + 2047 of part[b] (thread t owns entries 2048 g + t + 256 q); the
// combine adds the partials in block order: a fixed order, and S is exactly
// symmetric (y_i y_j and y_j y_i are the same products in the same order).
__global__ __launch_bounds__(256) void fold_yty_partial_kernel(const double* __restrict__ Y,
                                                               int64_t rows, int k,
                                                               double* __restrict__ part) {
  __shared__ double sh[FY_CH][kMaxK];
  const int64_t r0 = rows * blockIdx.x / gridDim.x, r1 = rows * (blockIdx.x + 1) / gridDim.x;
  const int kk = k * k, e0 = blockIdx.y * (256 * FY_NQ) + threadIdx.x;
  int ei[FY_NQ], ej[FY_NQ];
  double acc[FY_NQ];
#pragma unroll
  for (int q = 0; q < FY_NQ; ++q) {
    const int e = e0 + 256 * q;
    acc[q] = 0.0;
    ei[q] = e < kk ? e / k : 0;
    ej[q] = e < kk ? e % k : 0;
  }
  for (int64_t rb = r0; rb < r1; rb += FY_CH) {
    const int n = r1 - rb < FY_CH ? (int)(r1 - rb) : FY_CH;
    __syncthreads();
    for (int t = threadIdx.x; t < n * k; t += 256) sh[t / k][t % k] = Y[rb * k + t];
    __syncthreads();
    for (int r = 0; r < n; ++r) {
#pragma unroll
      for (int q = 0; q < FY_NQ; ++q) acc[q] = fma(sh[r][ei[q]], sh[r][ej[q]], acc[q]);
    }
  }
  double* out = part + (int64_t)blockIdx.x * kk;
#pragma unroll
  for (int q = 0; q < FY_NQ; ++q)
    if (e0 + 256 * q < kk) out[e0 + 256 * q] = acc[q];
}

__global__ __launch_bounds__(256) void fold_yty_combine_kernel(const double* __restrict__ part,
                                                               int nblk, int n,
                                                               double* __restrict__ S) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += part[(int64_t)b * n + t];
  S[t] = s;
}

// K-F2: one block per user, the shape of fold_in_kernel (serving.hip K-S4)
// without the bias column.  Rows [y | w] are staged rows_per_stage at a time;
// each thread owns IF_NE entries of the upper triangle of sum w y y^T in
// registers (row order), threads 0 .. k-1 also one entry of c = sum (1 + w) y.
// Then G = (S + sum) + lambda_u I is formed in LDS ([k][k+1], the rhs in
// column k), factored, and solved.
constexpr int IF_NE = 9;

__global__ __launch_bounds__(256) void implicit_fold_in_kernel(
    int k, int rows_per_stage, double alpha, double reg, int weighted,
    const int64_t* __restrict__ off, const int* __restrict__ item, const double* __restrict__ r,
    const double* __restrict__ Y, const double* __restrict__ S, double* __restrict__ X,
    int* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  __shared__ int s_bad;
  const int W = k + 1;   // row width: k factors, then the weight (LDS) / the rhs (G)
  const int u = blockIdx.x, tid = threadIdx.x;
  const int64_t b = off[u];
  const int M = (int)(off[u + 1] - b);
  if (M == 0) {   // block-uniform: an entity without ratings is the zero row
    for (int i = tid; i < k; i += 256) X[(int64_t)u * k + i] = 0.0;
    if (tid == 0) status[u] = 1;
    return;
  }
  const int T = k * (k + 1) / 2;
  double* G = lds;              // [k][W]
  double* As = lds + k * W;     // [rows_per_stage][W]
  const double lam = weighted ? reg * (double)M : reg;
  for (int g0 = 0; g0 < T; g0 += 256 * IF_NE) {
    const bool rhs_pass = g0 == 0;
    int ei[IF_NE], ej[IF_NE];
    double acc[IF_NE], cacc = 0.0;
#pragma unroll
    for (int t = 0; t < IF_NE; ++t) {
      int f = g0 + tid + 256 * t;
      acc[t] = 0.0;
      ei[t] = -1;
      ej[t] = -1;
      if (f < T) {
        int i = 0, len = k;
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
      for (int q = tid; q < nr * W; q += 256) {
        const int row = q / W, j = q % W;
        As[row * W + j] = j < k ? Y[(int64_t)item[b + r0 + row] * k + j]
                                : alpha * r[b + r0 + row];
      }
      __syncthreads();
#pragma unroll
      for (int t = 0; t < IF_NE; ++t) {
        if (ei[t] < 0) continue;
        double s = acc[t];
        for (int row = 0; row < nr; ++row)
          s = fma(As[row * W + k] * As[row * W + ei[t]], As[row * W + ej[t]], s);
        acc[t] = s;
      }
      if (rhs_pass && tid < k)
        for (int row = 0; row < nr; ++row)
          cacc = fma(1.0 + As[row * W + k], As[row * W + tid], cacc);
      __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < IF_NE; ++t) {
      if (ei[t] < 0) continue;
      double g = S[ei[t] * k + ej[t]] + acc[t];
      if (ei[t] == ej[t]) g += lam;
      G[ei[t] * W + ej[t]] = g;
      G[ej[t] * W + ei[t]] = g;
    }
    if (rhs_pass && tid < k) G[tid * W + k] = cacc;
  }
  if (tid == 0) s_bad = 0;
  __syncthreads();
  for (int j = 0; j < k; ++j) {
    if (tid == 0) {
      const double d = G[j * W + j];
      if (!(d > 0.0)) s_bad = 1;
      else G[j * W + j] = sqrt(d);
    }
    __syncthreads();
    if (s_bad) break;
    const double ljj = G[j * W + j];
    for (int i = j + 1 + tid; i < k; i += 256) G[i * W + j] /= ljj;
    __syncthreads();
    const int m = k - j - 1;
    for (int q = tid; q < m * m; q += 256) {
      const int ii = j + 1 + q / m, ll = j + 1 + q % m;
      if (ll <= ii) G[ii * W + ll] -= G[ii * W + j] * G[ll * W + j];
    }
    __syncthreads();
  }
  if (s_bad) {   // block-uniform (read after the barrier that follows its last write)
    for (int i = tid; i < k; i += 256) X[(int64_t)u * k + i] = 0.0;
    if (tid == 0) status[u] = 0;
    return;
  }
  // L y = c (right-looking), then L^T x = y
  for (int p = 0; p < k; ++p) {
    if (tid == 0) G[p * W + k] /= G[p * W + p];
    __syncthreads();
    for (int i = p + 1 + tid; i < k; i += 256) G[i * W + k] -= G[i * W + p] * G[p * W + k];
    __syncthreads();
  }
  for (int p = k - 1; p >= 0; --p) {
    if (tid == 0) G[p * W + k] /= G[p * W + p];
    __syncthreads();
    for (int i = tid; i < p; i += 256) G[i * W + k] -= G[p * W + i] * G[p * W + k];
    __syncthreads();
  }
  for (int i = tid; i < k; i += 256) X[(int64_t)u * k + i] = G[i * W + k];
  if (tid == 0) status[u] = 1;
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
// mr_rank_set_tuning: 0 = default
static int g_user_chunk = 0, g_item_groups = 0, g_lds_pairs = RK_LC;

// users per launch: the X chunk stays below 256 MiB
static int64_t rank_user_chunk(int k) {
  if (g_user_chunk > 0) return ((int64_t)g_user_chunk + RK_U - 1) / RK_U * RK_U;
  const int64_t per = (int64_t)k * 8;
  return std::max<int64_t>(RK_U, std::min<int64_t>(65535LL * RK_U, (1LL << 28) / per / RK_U * RK_U));
}

static int rank_counts(int device, int k, int n_users, int n_items, const double* X,
                       const double* user_bias, const double* Y, const double* item_offset,
                       const long long* test_off, const int* test_item,
                       const long long* excl_off, const int* excl_item, int* above, int* tied,
                       int* tied_before, double* score, int* n_eligible, double* kernel_ms) {
  MR_CHECK(k >= 1 && k <= kMaxKLarge, "rank_counts: k must be in 1..512");
  MR_CHECK(n_users >= 0 && n_items >= 0, "rank_counts: negative sizes");
  MR_CHECK(n_users < 0x7fffffff, "rank_counts: too many users");
  MR_CHECK(test_off && n_eligible, "rank_counts: test_off and n_eligible are required");
  MR_CHECK(rk_offsets_ok(test_off, n_users), "rank_counts: test offsets must start at 0 and not decrease");
  MR_CHECK(!excl_off || rk_offsets_ok(excl_off, n_users),
           "rank_counts: exclusion offsets must start at 0 and not decrease");
  const int64_t n_test = test_off[n_users], n_excl = excl_off ? excl_off[n_users] : 0;
  MR_CHECK(n_test == 0 || (test_item && above && tied && tied_before),
           "rank_counts: test_item, above, tied and tied_before are required");
  MR_CHECK(n_excl == 0 || excl_item, "rank_counts: excl_item is required");
  MR_CHECK(n_users == 0 || n_items == 0 || (X && Y), "rank_counts: X and Y are required");
  for (int64_t i = 0; i < n_test; ++i)
    MR_CHECK(test_item[i] >= 0 && test_item[i] < n_items, "rank_counts: test item id out of range");
  for (int64_t i = 0; i < n_excl; ++i)
    MR_CHECK(excl_item[i] >= 0 && excl_item[i] < n_items,
             "rank_counts: excluded item id out of range");
  if (n_excl > 0) {
    std::vector<int> mark((size_t)n_items, 0);   // mark[i] == u + 1: user u excludes item i
    for (int u = 0; u < n_users; ++u) {
      for (int64_t i = excl_off[u]; i < excl_off[u + 1]; ++i) {
        MR_CHECK(mark[excl_item[i]] != u + 1, "rank_counts: duplicate item in an exclusion list");
        mark[excl_item[i]] = u + 1;
      }
      for (int64_t i = test_off[u]; i < test_off[u + 1]; ++i)
        MR_CHECK(mark[test_item[i]] != u + 1, "rank_counts: a test item is also excluded");
    }
  }
  if (kernel_ms) kernel_ms[0] = kernel_ms[1] = kernel_ms[2] = 0.0;
  for (int u = 0; u < n_users; ++u)
    n_eligible[u] = n_items - (excl_off ? (int)(excl_off[u + 1] - excl_off[u]) : 0);
  if (n_test == 0) return 0;

  RkScope sc;
  if (sc.init(device)) return -1;
  hipStream_t s = sc.s;
  RkBuf<double> dY, dM;
  if (dY.upload(Y, (int64_t)n_items * k, s)) return -1;
  if (item_offset ? dM.upload(item_offset, n_items, s) : dM.zeros(n_items, s)) return -1;
  const int n_item_tiles = (n_items + RK_C - 1) / RK_C;
  const int64_t B = std::min<int64_t>(rank_user_chunk(k), ((int64_t)n_users + RK_U - 1) / RK_U * RK_U);
  std::vector<int64_t> loc;
  std::vector<int> who;
  // user ids (local to the chunk) of the pairs of CSR rows [u0, u0 + nb)
  auto owners = [&](const long long* off, int64_t u0, int nb) {
    who.resize((size_t)(off[u0 + nb] - off[u0]));
    loc.assign(nb + 1, 0);
    for (int i = 0; i < nb; ++i) {
      loc[i + 1] = off[u0 + i + 1] - off[u0];
      std::fill(who.begin() + loc[i], who.begin() + loc[i + 1], i);
    }
  };
  for (int64_t u0 = 0; u0 < n_users; u0 += B) {
    const int nb = (int)std::min<int64_t>(B, n_users - u0);
    const int64_t t0 = test_off[u0], nt = test_off[u0 + nb] - t0;
    if (nt == 0) continue;
    const int64_t e0 = excl_off ? excl_off[u0] : 0, ne = excl_off ? excl_off[u0 + nb] - e0 : 0;
    RkBuf<double> dX, dB, dthr, descore;
    RkBuf<int64_t> dtoff, deoff;
    RkBuf<int> dtitem, dtwho, deitem, dewho, dab, dti, dtb, dsidx;
    RkBuf<uint64_t> dskey;
    if (dX.upload(X + u0 * k, (int64_t)nb * k, s)) return -1;
    if (user_bias ? dB.upload(user_bias + u0, nb, s) : dB.zeros(nb, s)) return -1;
    owners(test_off, u0, nb);
    if (dtoff.upload(loc.data(), nb + 1, s) || dtwho.upload(who.data(), nt, s) ||
        dtitem.upload(test_item + t0, nt, s) || dthr.alloc(nt) || dab.alloc(nt) ||
        dti.alloc(nt) || dtb.alloc(nt) || dskey.alloc(nt) || dsidx.alloc(nt))
      return -1;
    if (ne > 0) {
      owners(excl_off, u0, nb);
      if (deoff.upload(loc.data(), nb + 1, s) || dewho.upload(who.data(), ne, s) ||
          deitem.upload(excl_item + e0, ne, s) || descore.alloc(ne))
        return -1;
    }
    if (sc.timed(kernel_ms ? kernel_ms + 0 : nullptr, [&]() {
          rank_pair_score_kernel<true><<<(unsigned)((nt + 255) / 256), 256, 0, s>>>(
              nt, k, dX.p, dB.p, dY.p, dM.p, dtwho.p, dtitem.p, dthr.p, dab.p, dti.p, dtb.p);
          rank_sort_kernel<<<nb, 256, 0, s>>>(g_lds_pairs, dtoff.p, dthr.p, dskey.p, dsidx.p);
          if (ne > 0)
            rank_pair_score_kernel<false><<<(unsigned)((ne + 255) / 256), 256, 0, s>>>(
                ne, k, dX.p, dB.p, dY.p, dM.p, dewho.p, deitem.p, descore.p, nullptr, nullptr,
                nullptr);
        }))
      return -1;
    const int user_tiles = (nb + RK_U - 1) / RK_U;
    // about 8192 blocks: several rounds of the 512 a chip holds, so uneven
    // tiles even out, while a block still walks many item tiles and its
    // counts leave LDS once (measured: DESIGN.md)
    int groups = g_item_groups > 0 ? g_item_groups : (8192 + user_tiles - 1) / user_tiles;
    groups = std::max(1, std::min(groups, std::min(n_item_tiles, 65535)));
    if (sc.timed(kernel_ms ? kernel_ms + 1 : nullptr, [&]() {
          rank_count_kernel<<<dim3(user_tiles, groups), 256, 0, s>>>(
              nb, n_items, k, n_item_tiles, g_lds_pairs, dX.p, dB.p, dY.p, dM.p, dtoff.p, dthr.p,
              dtitem.p, dskey.p, dsidx.p, dab.p, dti.p, dtb.p);
        }))
      return -1;
    if (ne > 0 &&
        sc.timed(kernel_ms ? kernel_ms + 2 : nullptr, [&]() {
          rank_exclude_kernel<<<nb, 256, 0, s>>>(dtoff.p, dthr.p, dtitem.p, deoff.p, descore.p,
                                                 deitem.p, dab.p, dti.p, dtb.p);
        }))
      return -1;
    MR_D2H(above + t0, dab.p, nt * 4, s);
    MR_D2H(tied + t0, dti.p, nt * 4, s);
    MR_D2H(tied_before + t0, dtb.p, nt * 4, s);
    if (score) MR_D2H(score + t0, dthr.p, nt * 8, s);
    MR_HIP(hipStreamSynchronize(s));
  }
  return 0;
}

static int implicit_fold_in(int device, int k, int n_items, const double* Y, double alpha,
                            double reg, int reg_mode, int n_users, const long long* off,
                            const int* item, const double* r, double* x_out, int* status) {
  MR_CHECK(k >= 1 && k <= kMaxK, "implicit fold-in: k must be in 1..128");
  MR_CHECK(n_users >= 0 && n_items >= 0, "implicit fold-in: negative sizes");
  MR_CHECK(std::isfinite(alpha) && alpha >= 0.0, "implicit fold-in: alpha must be finite and >= 0");
  MR_CHECK(std::isfinite(reg) && reg >= 0.0, "implicit fold-in: reg must be finite and >= 0");
  MR_CHECK(reg_mode == MR_REG_CONSTANT || reg_mode == MR_REG_WEIGHTED,
           "implicit fold-in: unknown regularization mode");
  if (n_users == 0) return 0;
  MR_CHECK(off && x_out, "implicit fold-in: off and x_out are required");
  MR_CHECK(rk_offsets_ok(off, n_users), "implicit fold-in: offsets must start at 0 and not decrease");
  const int64_t nnz = off[n_users];
  MR_CHECK(nnz == 0 || (item && r && Y), "implicit fold-in: item, r and Y are required");
  for (int u = 0; u < n_users; ++u)
    MR_CHECK(off[u + 1] - off[u] < 0x7fffffff, "implicit fold-in: list too long");
  for (int64_t i = 0; i < nnz; ++i) {
    MR_CHECK(item[i] >= 0 && item[i] < n_items, "implicit fold-in: item id out of range");
    MR_CHECK(std::isfinite(r[i]) && r[i] >= 0.0, "implicit fold-in: r must be finite and >= 0");
  }
  RkScope sc;
  if (sc.init(device)) return -1;
  hipStream_t s = sc.s;
  const int kk = k * k;
  const int nblk = (int)std::max<int64_t>(1, std::min<int64_t>(((int64_t)n_items + 63) / 64, 256));
  RkBuf<double> dY, dpart, dS, dr, dX;
  RkBuf<int64_t> doff;
  RkBuf<int> ditem, dstat;
  if (dY.upload(Y, (int64_t)n_items * k, s) || dpart.alloc((int64_t)nblk * kk) || dS.alloc(kk) ||
      doff.upload(reinterpret_cast<const int64_t*>(off), (int64_t)n_users + 1, s) ||
      ditem.upload(item, nnz, s) || dr.upload(r, nnz, s) || dX.alloc((int64_t)n_users * k) ||
      dstat.alloc(n_users))
    return -1;
  fold_yty_partial_kernel<<<dim3(nblk, (kk + 256 * FY_NQ - 1) / (256 * FY_NQ)), 256, 0, s>>>(
      dY.p, n_items, k, dpart.p);
  fold_yty_combine_kernel<<<(kk + 255) / 256, 256, 0, s>>>(dpart.p, nblk, kk, dS.p);
  MR_HIP(hipGetLastError());
  // LDS: G [k][k+1] plus a row stage of up to 32 rows (fewer at k = 128)
  const size_t W = (size_t)k + 1, gbytes = (size_t)k * W * sizeof(double);
  const size_t budget = 150 * 1024;
  MR_CHECK(gbytes + 8 * W * sizeof(double) <= budget, "implicit fold-in: k too large");
  const int rows = (int)std::min<size_t>(32, (budget - gbytes) / (W * sizeof(double)));
  const size_t lds = gbytes + (size_t)rows * W * sizeof(double);
  if (lds > 64 * 1024)
    MR_HIP(hipFuncSetAttribute((const void*)implicit_fold_in_kernel,
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  implicit_fold_in_kernel<<<n_users, 256, lds, s>>>(k, rows, alpha, reg,
                                                    reg_mode == MR_REG_WEIGHTED ? 1 : 0, doff.p,
                                                    ditem.p, dr.p, dY.p, dS.p, dX.p, dstat.p);
  MR_HIP(hipGetLastError());
  MR_D2H(x_out, dX.p, (size_t)n_users * k * 8, s);
  if (status) MR_D2H(status, dstat.p, (size_t)n_users * 4, s);
  MR_HIP(hipStreamSynchronize(s));
  return 0;
}

}  // namespace mr

extern "C" {

int mr_rank_counts(int device, int k, int n_users, int n_items, const double* X,
                   const double* user_bias, const double* Y, const double* item_offset,
                   const long long* test_off, const int* test_item, const long long* excl_off,
                   const int* excl_item, int* above, int* tied, int* tied_before, double* score,
                   int* n_eligible, double* kernel_ms) {
  return mr::rk_guard([&]() {
    return mr::rank_counts(device, k, n_users, n_items, X, user_bias, Y, item_offset, test_off,
                           test_item, excl_off, excl_item, above, tied, tied_before, score,
                           n_eligible, kernel_ms);
  });
}

int mr_rank_set_tuning(int user_chunk, int item_groups, int lds_pairs) {
  return mr::rk_guard([&]() -> int {
    MR_CHECK(user_chunk >= 0 && item_groups >= 0 && item_groups <= 65535 &&
                 lds_pairs <= mr::RK_LC,
             "rank tuning: user_chunk >= 0, item_groups in 0..65535, lds_pairs <= 2048");
    mr::g_user_chunk = user_chunk;
    mr::g_item_groups = item_groups;
    mr::g_lds_pairs = lds_pairs == 0 ? mr::RK_LC : std::max(lds_pairs, 0);
    return 0;
  });
}

int mr_implicit_fold_in(int device, int k, int n_items, const double* Y, double alpha, double reg,
                        int reg_mode, int n_users, const long long* off, const int* item,
                        const double* r, double* x_out, int* status) {
  return mr::rk_guard([&]() {
    return mr::implicit_fold_in(device, k, n_items, Y, alpha, reg, reg_mode, n_users, off, item,
                                r, x_out, status);
  });
}

}  // extern "C"
