// fp64 reduction helpers shared by the objective kernels (regularize.hip,
// implicit.hip): factor-row loads by lane groups, fixed-order sums.
#pragma once
#include "mr_internal.h"

namespace mr {

// ---------------------------------------------------------------------------
// Objective pieces.  Factor rows are ldk fp32 (padding columns zero), read as
// float4 by groups of GL lanes (GL: the power of two >= ldk / 4, 4 .. 64; two
// float4 per lane for ldk > 256); products and sums in fp64.  Every sum is
// reduced in a fixed order: lanes by a xor butterfly, the block's four waves
// in wave order into one fp64 partial per block, the partials in block order
// (launch_sum_partials) -- two calls on the same state give the same bits.
// ---------------------------------------------------------------------------
constexpr int kObjWaves = 4;      // waves per block, one Gram work item each
constexpr int kObjUnroll = 4;     // gathered rows in flight per lane group
constexpr int kRowGridCap = 1024; // blocks of the per-row kernels (fixed per size)

struct Row2 {
  float4 a, b;
};

template <int GL>
__device__ inline Row2 load_row(const float* __restrict__ row, int nq, int sub, bool on) {
  Row2 r;
  r.a = make_float4(0.f, 0.f, 0.f, 0.f);
  r.b = r.a;
  const float4* p = reinterpret_cast<const float4*>(row);
  if (on && sub < nq) r.a = p[sub];
  if (GL == 64 && on && sub + 64 < nq) r.b = p[sub + 64];
  return r;
}

template <int GL>
__device__ inline double dot_rows(const Row2& x, const Row2& y) {
  double d = (double)x.a.x * y.a.x;
  d += (double)x.a.y * y.a.y;
  d += (double)x.a.z * y.a.z;
  d += (double)x.a.w * y.a.w;
  if (GL == 64) {
    d += (double)x.b.x * y.b.x;
    d += (double)x.b.y * y.b.y;
    d += (double)x.b.z * y.b.z;
    d += (double)x.b.w * y.b.w;
  }
  return d;
}

// sum over the GL lanes of a group (every lane gets it)
template <int GL>
__device__ inline double group_sum(double d) {
#pragma unroll
  for (int m = GL / 2; m >= 1; m >>= 1) d += __shfl_xor(d, m, 64);
  return d;
}

__device__ inline double wave_sum(double d) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) d += __shfl_xor(d, m, 64);
  return d;
}

// part[NC * block + c] = the block's sum of component c (waves in order)
template <int NC>
__device__ inline void block_partials(const double (&acc)[NC], double* __restrict__ part) {
  __shared__ double sm[kObjWaves][NC];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const double s = wave_sum(acc[c]);
    if (lane == 0) sm[wave][c] = s;
  }
  __syncthreads();
  if (threadIdx.x < NC) {
    double s = 0.0;
    for (int w = 0; w < kObjWaves; ++w) s += sm[w][threadIdx.x];
    part[(int64_t)NC * blockIdx.x + threadIdx.x] = s;
  }
}

inline int lanes_for(int ldk) {
  int gl = 4;
  while (gl < 64 && gl < ldk / 4) gl <<= 1;
  return gl;
}

#define MR_BY_LANES(gl, CALL)                 \
  switch (gl) {                               \
    case 4: CALL(4); break;                   \
    case 8: CALL(8); break;                   \
    case 16: CALL(16); break;                 \
    case 32: CALL(32); break;                 \
    default: CALL(64); break;                 \
  }

}  // namespace mr
