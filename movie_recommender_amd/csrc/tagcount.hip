// Content model on MI355X (gfx950): the reference's per-user tag-count
// recommender.  C ABI and the model's definition: include/mr_tagcount.h.
// Reference behaviour:
//   model   python/app_local/models.py:24-336 (== full_data/tag_count_predictor.py)
//   eval    python/full_data/worker_process.py:231-258, 344-418
//
// One wave per user throughout the fit.  K-T1 accumulates the user's tag
// profile into a dense row of an HBM scratch (one f64 per distinct tag of the
// table) and the genre profile in LDS, rating by rating in list order, then
// divides by the counts.  K-T2 builds the rows of A0 / A1 from those profiles
// and solves both systems: Householder QR of [A | b] with the column sums taken
// over the wave in a fixed order, then a one-sided Jacobi SVD of the small R
// with a fixed sweep order, the rank cut and the minimum-norm x.  K-T3 compacts
// the dense row into the CSR the caller gets.  Scoring scatters a model's CSR
// profile back into a dense row and gathers from it per candidate tag (K-T4 /
// K-T5); top-N and the agreement are the kernels of serving.hip.
//
// Every floating-point sum has an order that depends on the user's own list
// only, so a list gives the same bits alone, in any batch and from run to run.
// No multiply-add is contracted anywhere in this file.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/mr_als.h"
#include "../../include/mr_tagcount.h"
#include "mr_internal.h"
#include "serving_device.h"

namespace mr {

constexpr int TC_MAXG = MR_TAGCOUNT_MAX_GENRES;
constexpr int TC_WAVE = 64;   // block size of K-T1 .. K-T3: one wave, never more
static_assert(TC_WAVE == 64, "K-T1 .. K-T3 are written for a block of exactly one 64-wide wave");

// The table as the kernels see it.
struct TcTable {
  const int64_t* goff;
  const int* gidx;
  const int64_t* toff;
  const int* tidx;
  const double* tval;
  const double* med;
  const double* gcount;
  const double* tcount;
  int n_genres, n_tags;
};

__device__ __forceinline__ double tc_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int tc_wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// tag_dot / genre_dot of candidate c (models.py:125-150): the movie's entries
// in stored order, sum from +0.  `row` is the user's dense tag profile; a tag
// the profile lacks reads 0 there, and adding +-0 to a sum that started at +0
// never changes a bit.
__device__ __forceinline__ double tc_tag_dot(const TcTable& t, int c,
                                             const double* __restrict__ row) {
  double s = 0.0;
  const int64_t e1 = t.toff[c + 1];
  for (int64_t e = t.toff[c]; e < e1; ++e) s = add_rn(s, mul_rn(row[t.tidx[e]], t.tval[e]));
  return s;
}
__device__ __forceinline__ double tc_genre_dot(const TcTable& t, int c, const double* gp) {
  double s = 0.0;
  const int64_t e1 = t.goff[c + 1];
  for (int64_t e = t.goff[c]; e < e1; ++e) s = add_rn(s, gp[t.gidx[e]]);
  return s;
}

// ---------------------------------------------------------------------------
// K-T1: profiles of one user per wave (models.py:67-122).  The ratings are
// taken one after the other in list order; the lanes take the entries of the
// rating's movie, which are distinct inside a movie, so two lanes never meet
// on a profile entry within a step.  rows: zeroed by the host before the
// launch, slot-major, n_tags doubles per user of the launch.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(TC_WAVE) void tagcount_profile_kernel(
    int u0, const int64_t* __restrict__ off, const int* __restrict__ cand,
    const double* __restrict__ rating, TcTable t, double* __restrict__ rows,
    double* __restrict__ gp_out, int* __restrict__ cnt_out) {
  __shared__ double gp[TC_MAXG];
  const int slot = blockIdx.x, u = u0 + slot, lane = threadIdx.x;
  double* row = rows + (int64_t)slot * t.n_tags;
  const int64_t b = off[u], e = off[u + 1];
  for (int g = lane; g < t.n_genres; g += TC_WAVE) gp[g] = 0.0;
  __syncthreads();
  for (int64_t i = b; i < e; ++i) {
    const double offset = rating[i] - 3.0;
    if (offset == 0.0) continue;   // the same for every lane: `offset` is one value per step
    const int c = cand[i];
    const int64_t t0 = t.toff[c], g0 = t.goff[c];
    const int nt = (int)(t.toff[c + 1] - t0), ng = (int)(t.goff[c + 1] - g0);
    for (int k = lane; k < nt; k += TC_WAVE) {
      const int idx = t.tidx[t0 + k];
      row[idx] = add_rn(row[idx], mul_rn(offset, t.tval[t0 + k]));
    }
    for (int k = lane; k < ng; k += TC_WAVE) {
      const int idx = t.gidx[g0 + k];
      gp[idx] = add_rn(gp[idx], offset);
    }
    // Two consecutive movies may share a tag (or a genre), and then a
    // DIFFERENT lane reads the entry in the next step that this step wrote.
    // The barrier carries a workgroup-scope release / acquire: this step's
    // global and LDS writes are complete and visible to every lane of the
    // block before any lane starts the next step's reads.
    __syncthreads();
  }
  int cnt = 0;
  for (int k = lane; k < t.n_tags; k += TC_WAVE) {
    const double v = row[k] / t.tcount[k];   // 0 / count = 0: untouched entries stay 0
    row[k] = v;
    cnt += v != 0.0 ? 1 : 0;
  }
  cnt = tc_wave_sum_int(cnt);
  if (lane == 0) cnt_out[slot] = cnt;
  for (int g = lane; g < t.n_genres; g += TC_WAVE)
    gp_out[(int64_t)u * t.n_genres + g] = gp[g] / t.gcount[g];
}

// ---------------------------------------------------------------------------
// K-T2: rows and fit of one user per wave (models.py:153-215).
//
// Row i belongs to lane i mod 64 from the first write to the last read, so no
// lane ever reads what another lane wrote to the scratch; pivot-row values
// travel by shuffle from their owner.  The scratch holds 7 columns of length
// n per user: A0 = [tag_dot, genre_dot, 1 | b] with the rows that fail
// tag_dot > 0.1 written as zero rows (a zero row changes neither R nor Q^T b,
// so this is the system of the n0 kept rows), then A1 = [genre_dot, 1 | b].
//
// tc_qr_solve: Householder QR of the NC + 1 columns at `a` (LAPACK dlarfg's
// reflector; a column that is already zero below its pivot is left alone),
// then R = V-rotated by one-sided Jacobi (Hestenes) in the fixed pair order
// (0,1), (0,2), (1,2) until a sweep rotates nothing, at most TC_SWEEPS times.
// Singular values <= eps * max(m_cut, NC) * s_max count as zero; x is the
// minimum-norm solution over the others.  Every lane computes the small SVD
// redundantly on the same values.
// ---------------------------------------------------------------------------
constexpr int TC_SWEEPS = 30;

template <int NC>
__device__ void tc_qr_solve(double* __restrict__ a, int n, int lane, int m_cut, double* x,
                            int* rank) {
  for (int k = 0; k < NC; ++k) {
    double* ak = a + (int64_t)k * n;
    const int first = lane > k ? lane : lane + TC_WAVE;   // this lane's first row below k
    double ss = 0.0;
    for (int i = first; i < n; i += TC_WAVE) ss += ak[i] * ak[i];
    ss = tc_wave_sum(ss);
    if (ss == 0.0) continue;
    const double alpha = __shfl(lane == k ? ak[k] : 0.0, k, 64);
    const double beta = -copysign(sqrt(alpha * alpha + ss), alpha);
    const double tau = (beta - alpha) / beta, scale = 1.0 / (alpha - beta);
    for (int i = first; i < n; i += TC_WAVE) ak[i] = ak[i] * scale;
    if (lane == k) ak[k] = beta;
    for (int j = k + 1; j <= NC; ++j) {
      double* aj = a + (int64_t)j * n;
      double w = 0.0;
      for (int i = first; i < n; i += TC_WAVE) w += ak[i] * aj[i];
      const double akj = __shfl(lane == k ? aj[k] : 0.0, k, 64);
      w = tc_wave_sum(w) + akj;
      const double tw = tau * w;
      if (lane == k) aj[k] = akj - tw;
      for (int i = first; i < n; i += TC_WAVE) aj[i] = aj[i] - tw * ak[i];
    }
  }
  // R (upper triangle, rows 0 .. NC-1 owned by lanes 0 .. NC-1) and c = (Q^T b)[0 .. NC)
  double G[NC][NC], V[NC][NC], c[NC];
#pragma unroll
  for (int r = 0; r < NC; ++r) {
#pragma unroll
    for (int q = 0; q < NC; ++q) {
      G[r][q] = q >= r ? __shfl(lane == r ? a[(int64_t)q * n + r] : 0.0, r, 64) : 0.0;
      V[r][q] = r == q ? 1.0 : 0.0;
    }
    c[r] = __shfl(lane == r ? a[(int64_t)NC * n + r] : 0.0, r, 64);
  }
  const double eps = 2.220446049250313e-16;
  for (int sweep = 0; sweep < TC_SWEEPS; ++sweep) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < NC - 1; ++p) {
#pragma unroll
      for (int q = p + 1; q < NC; ++q) {
        double app = 0.0, aqq = 0.0, apq = 0.0;
#pragma unroll
        for (int r = 0; r < NC; ++r) {
          app += G[r][p] * G[r][p];
          aqq += G[r][q] * G[r][q];
          apq += G[r][p] * G[r][q];
        }
        if (apq == 0.0 || fabs(apq) <= eps * sqrt(app * aqq)) continue;
        rotated = true;
        const double zeta = (aqq - app) / (2.0 * apq);
        const double tn = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double cs = 1.0 / sqrt(1.0 + tn * tn), sn = cs * tn;
#pragma unroll
        for (int r = 0; r < NC; ++r) {
          const double gp_ = G[r][p], gq_ = G[r][q];
          G[r][p] = cs * gp_ - sn * gq_;
          G[r][q] = sn * gp_ + cs * gq_;
          const double vp_ = V[r][p], vq_ = V[r][q];
          V[r][p] = cs * vp_ - sn * vq_;
          V[r][q] = sn * vp_ + cs * vq_;
        }
      }
    }
    if (!rotated) break;
  }
  double sig[NC], smax = 0.0;
#pragma unroll
  for (int q = 0; q < NC; ++q) {
    double s2 = 0.0;
#pragma unroll
    for (int r = 0; r < NC; ++r) s2 += G[r][q] * G[r][q];
    sig[q] = sqrt(s2);
    smax = fmax(smax, sig[q]);
  }
  const double cut = eps * (double)max(m_cut, NC) * smax;
  int rk = 0;
#pragma unroll
  for (int r = 0; r < NC; ++r) x[r] = 0.0;
#pragma unroll
  for (int q = 0; q < NC; ++q) {
    if (!(sig[q] > cut)) continue;
    ++rk;
    double d = 0.0;
#pragma unroll
    for (int r = 0; r < NC; ++r) d += G[r][q] * c[r];
    const double f = (d / sig[q]) / sig[q];
#pragma unroll
    for (int r = 0; r < NC; ++r) x[r] += V[r][q] * f;
  }
  *rank = rk;
}

__global__ __launch_bounds__(TC_WAVE) void tagcount_fit_kernel(
    int u0, const int64_t* __restrict__ off, const int* __restrict__ cand,
    const double* __restrict__ rating, TcTable t, const double* __restrict__ rows,
    const double* __restrict__ gp_all, double* __restrict__ work, double* __restrict__ x0_out,
    double* __restrict__ x1_out, int* __restrict__ has0, int* __restrict__ has1,
    int* __restrict__ n0_out, int* __restrict__ rank0, int* __restrict__ rank1) {
  __shared__ double gp[TC_MAXG];
  const int slot = blockIdx.x, u = u0 + slot, lane = threadIdx.x;
  const double* row = rows + (int64_t)slot * t.n_tags;
  const int64_t b = off[u];
  const int n = (int)(off[u + 1] - b);
  double* w = work + 7 * (b - off[u0]);
  for (int g = lane; g < t.n_genres; g += TC_WAVE) gp[g] = gp_all[(int64_t)u * t.n_genres + g];
  __syncthreads();
  int kept = 0;
  for (int i = lane; i < n; i += TC_WAVE) {
    const int c = cand[b + i];
    const double td = tc_tag_dot(t, c, row), gd = tc_genre_dot(t, c, gp);
    const double bi = rating[b + i] - t.med[c];
    const bool in0 = td > 0.1;   // the reference's math.fabs(tag_dot > 0.1): no absolute value
    w[(int64_t)0 * n + i] = in0 ? td : 0.0;
    w[(int64_t)1 * n + i] = in0 ? gd : 0.0;
    w[(int64_t)2 * n + i] = in0 ? 1.0 : 0.0;
    w[(int64_t)3 * n + i] = in0 ? bi : 0.0;
    w[(int64_t)4 * n + i] = gd;
    w[(int64_t)5 * n + i] = 1.0;
    w[(int64_t)6 * n + i] = bi;
    kept += in0 ? 1 : 0;
  }
  const int n0 = tc_wave_sum_int(kept);
  double x0[3] = {0.0, 0.0, 0.0}, x1[2] = {0.0, 0.0};
  int r0 = 0, r1 = 0;
  if (n0 >= 3) tc_qr_solve<3>(w, n, lane, n0, x0, &r0);
  if (n >= 2) tc_qr_solve<2>(w + (int64_t)4 * n, n, lane, n, x1, &r1);
  if (lane == 0) {
    for (int j = 0; j < 3; ++j) x0_out[(int64_t)u * 3 + j] = x0[j];
    for (int j = 0; j < 2; ++j) x1_out[(int64_t)u * 2 + j] = x1[j];
    has0[u] = n0 >= 3 ? 1 : 0;
    has1[u] = n >= 2 ? 1 : 0;
    n0_out[u] = n0;
    rank0[u] = r0;
    rank1[u] = r1;
  }
}

// ---------------------------------------------------------------------------
// K-T3: the dense row's entries that are not 0, in ascending tag index, to
// idx / val from the user's offset (of the launch's CSR) on.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(TC_WAVE) void tagcount_compact_kernel(
    int n_tags, const double* __restrict__ rows, const int64_t* __restrict__ coff,
    int* __restrict__ idx, double* __restrict__ val) {
  const int slot = blockIdx.x, lane = threadIdx.x;
  const double* row = rows + (int64_t)slot * n_tags;
  int64_t pos = coff[slot];
  const int64_t end = coff[slot + 1];
  for (int k0 = 0; k0 < n_tags; k0 += TC_WAVE) {
    const int k = k0 + lane;
    const double v = k < n_tags ? row[k] : 0.0;
    const bool nz = v != 0.0;
    const unsigned long long mask = __ballot(nz);
    const int64_t at = pos + __popcll(mask & ((1ull << lane) - 1ull));
    if (nz && at < end) {   // `at < end` holds by the count K-T1 took of the same row
      idx[at] = k;
      val[at] = v;
    }
    pos += __popcll(mask);
  }
}

// ---------------------------------------------------------------------------
// K-T4 / K-T5: scores from a model (models.py:218-262; order of the sums as
// include/mr_tagcount.h defines it).  The model's CSR tag profile is scattered
// into a zeroed dense row first; a model without x0 never reads it.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tagcount_scatter_kernel(
    int n_tags, const int64_t* __restrict__ poff, const int* __restrict__ pidx,
    const double* __restrict__ pval, double* __restrict__ rows) {
  const int slot = blockIdx.x;
  double* row = rows + (int64_t)slot * n_tags;
  const int64_t e = poff[slot + 1];
  for (int64_t i = poff[slot] + threadIdx.x; i < e; i += 256) row[pidx[i]] = pval[i];
}

struct TcModelLds {
  double gp[TC_MAXG];
  double x0[3], x1[2];
  int has0, has1;
};

__device__ __forceinline__ void tc_load_model(int u, int n_genres, const double* __restrict__ gp,
                                              const double* __restrict__ x0,
                                              const double* __restrict__ x1,
                                              const int* __restrict__ has0,
                                              const int* __restrict__ has1, TcModelLds& m) {
  for (int g = threadIdx.x; g < n_genres; g += blockDim.x) m.gp[g] = gp[(int64_t)u * n_genres + g];
  if (threadIdx.x < 3) m.x0[threadIdx.x] = x0[(int64_t)u * 3 + threadIdx.x];
  if (threadIdx.x < 2) m.x1[threadIdx.x] = x1[(int64_t)u * 2 + threadIdx.x];
  if (threadIdx.x == 0) {
    m.has0 = has0[u];
    m.has1 = has1[u];
  }
  __syncthreads();
}

__device__ __forceinline__ double tc_score(const TcTable& t, int c, const TcModelLds& m,
                                           const double* __restrict__ row) {
  const double med = t.med[c];
  // tag_product only decides and feeds model 0
  const double tp = m.has0 ? tc_tag_dot(t, c, row) : 0.0;
  if (m.has0 && !(tp < 1e-6)) {
    const double gd = tc_genre_dot(t, c, m.gp);
    double s = add_rn(0.0, mul_rn(tp, m.x0[0]));
    s = add_rn(s, mul_rn(gd, m.x0[1]));
    s = add_rn(s, m.x0[2]);
    return add_rn(s, med);
  }
  if (m.has1) {
    const double gd = tc_genre_dot(t, c, m.gp);
    double s = add_rn(0.0, mul_rn(gd, m.x1[0]));
    s = add_rn(s, m.x1[1]);
    return add_rn(s, med);
  }
  return med;
}

template <bool KEYS>
__global__ __launch_bounds__(256) void tagcount_score_kernel(
    int n_cand, TcTable t, const double* __restrict__ gp, const double* __restrict__ x0,
    const double* __restrict__ x1, const int* __restrict__ has0, const int* __restrict__ has1,
    const double* __restrict__ rows, void* __restrict__ out, unsigned long long* __restrict__ kmin,
    unsigned long long* __restrict__ kmax) {
  __shared__ TcModelLds m;
  const int u = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  tc_load_model(u, t.n_genres, gp, x0, x1, has0, has1, m);
  unsigned long long lo = ~0ull, hi = 0ull;
  if (c < n_cand) {
    const double s = tc_score(t, c, m, rows + (int64_t)u * t.n_tags);
    if constexpr (KEYS) {
      const uint64_t key = score_key(s);
      reinterpret_cast<uint64_t*>(out)[(int64_t)u * n_cand + c] = key;
      lo = hi = key;
    } else {
      reinterpret_cast<double*>(out)[(int64_t)u * n_cand + c] = s;
    }
  }
  if constexpr (KEYS) {   // per-user key range for the select
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo = min(lo, (unsigned long long)__shfl_xor(lo, o, 64));
      hi = max(hi, (unsigned long long)__shfl_xor(hi, o, 64));
    }
    if ((threadIdx.x & 63) == 0 && hi != 0ull) {
      atomicMin(&kmin[u], lo);
      atomicMax(&kmax[u], hi);
    }
  }
}

// one block per test user of the chunk: predictions of its test ratings (NaN:
// no median); off / cand / pred are the whole call's, t0 the chunk's first user
__global__ __launch_bounds__(256) void tagcount_pred_kernel(
    int t0, TcTable t, const double* __restrict__ gp, const double* __restrict__ x0,
    const double* __restrict__ x1, const int* __restrict__ has0, const int* __restrict__ has1,
    const double* __restrict__ rows, const int64_t* __restrict__ off,
    const int* __restrict__ cand, double* __restrict__ pred) {
  __shared__ TcModelLds m;
  const int slot = blockIdx.x;
  tc_load_model(slot, t.n_genres, gp, x0, x1, has0, has1, m);
  const double* row = rows + (int64_t)slot * t.n_tags;
  const int64_t e = off[t0 + slot + 1];
  for (int64_t i = off[t0 + slot] + threadIdx.x; i < e; i += 256) {
    const int c = cand[i];
    pred[i] = c >= 0 ? tc_score(t, c, m, row) : NAN;
  }
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
enum { TC_PROFILE = 0, TC_FIT, TC_COMPACT, TC_SCATTER, TC_SCORE, TC_EXCL, TC_SELECT, TC_EVAL, TC_N };

struct TagCount {
  int device = 0, n_cand = 0, n_genres = 0, n_tags = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  int *mid = nullptr, *gidx = nullptr, *tidx = nullptr;
  double *med = nullptr, *tval = nullptr, *gcount = nullptr, *tcount = nullptr;
  int64_t *goff = nullptr, *toff = nullptr;
  double ms[TC_N] = {0};
  ~TagCount() {
    if (stream) {
      (void)hipFree(mid);
      (void)hipFree(gidx);
      (void)hipFree(tidx);
      (void)hipFree(med);
      (void)hipFree(tval);
      (void)hipFree(gcount);
      (void)hipFree(tcount);
      (void)hipFree(goff);
      (void)hipFree(toff);
      (void)hipStreamDestroy(stream);
    }
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  TcTable table() const {
    return TcTable{goff, gidx, toff, tidx, tval, med, gcount, tcount, n_genres, n_tags};
  }
  // doubles of one user's dense row (at least one, so an empty table still indexes)
  int64_t row_len() const { return std::max(n_tags, 1); }
};

template <typename F>
static int tc_timed(TagCount* r, int cls, F&& launch) {
  MR_HIP(hipEventRecord(r->ev[0], r->stream));
  launch();
  MR_HIP(hipGetLastError());
  MR_HIP(hipEventRecord(r->ev[1], r->stream));
  MR_HIP(hipEventSynchronize(r->ev[1]));
  float ms = 0.f;
  MR_HIP(hipEventElapsedTime(&ms, r->ev[0], r->ev[1]));
  r->ms[cls] += ms;
  return 0;
}

template <typename T>
static int tc_dev_copy(T** dst, const T* src, int64_t n, hipStream_t s) {
  MR_HIP(hipMalloc((void**)dst, (size_t)std::max<int64_t>(n, 1) * sizeof(T)));
  if (n > 0) MR_H2D(*dst, src, (size_t)n * sizeof(T), s);
  return 0;
}

// entries [off[c], off[c+1]) of idx: inside 0 .. limit-1 and distinct per candidate
static bool tc_entries_ok(const long long* off, const int* idx, int n_cand, int limit) {
  std::vector<int> stamp((size_t)std::max(limit, 1), -1);
  for (int c = 0; c < n_cand; ++c)
    for (int64_t i = off[c]; i < off[c + 1]; ++i) {
      if (idx[i] < 0 || idx[i] >= limit || stamp[idx[i]] == c) return false;
      stamp[idx[i]] = c;
    }
  return true;
}

static int tagcount_init(TagCount* r, int device, int n_cand, const int* cand_mid,
                         const double* cand_med, const long long* genre_off,
                         const int* genre_idx, const long long* tag_off, const int* tag_idx,
                         const double* tag_val, int n_genres, const double* genre_count,
                         int n_tags, const double* tag_count) {
  MR_CHECK(n_cand >= 0, "tagcount: negative n_cand");
  MR_CHECK(n_genres >= 0 && n_genres <= TC_MAXG, "tagcount: n_genres must be in 0..1024");
  MR_CHECK(n_tags >= 0, "tagcount: negative n_tags");
  MR_CHECK(rk_offsets_ok(genre_off, n_cand) && rk_offsets_ok(tag_off, n_cand),
           "tagcount: genre / tag offsets must start at 0 and not decrease");
  {
    std::vector<int> seen(cand_mid, cand_mid + n_cand);
    std::sort(seen.begin(), seen.end());
    MR_CHECK(std::adjacent_find(seen.begin(), seen.end()) == seen.end(),
             "tagcount: candidate movie ids must be unique");
    MR_CHECK(n_cand == 0 || seen.front() >= 0, "tagcount: movie ids must be >= 0");
  }
  MR_CHECK(tc_entries_ok(genre_off, genre_idx, n_cand, n_genres),
           "tagcount: genre indices must be in range and distinct inside a candidate");
  MR_CHECK(tc_entries_ok(tag_off, tag_idx, n_cand, n_tags),
           "tagcount: tag indices must be in range and distinct inside a candidate");
  const double lim = 9007199254740992.0;   // 2^53
  for (int g = 0; g < n_genres; ++g)
    MR_CHECK(genre_count[g] > 0.0 && genre_count[g] < lim,
             "tagcount: genre counts must be positive and below 2^53");
  for (int t = 0; t < n_tags; ++t)
    MR_CHECK(tag_count[t] > 0.0 && tag_count[t] < lim,
             "tagcount: tag counts must be positive and below 2^53");
  r->device = device;
  r->n_cand = n_cand;
  r->n_genres = n_genres;
  r->n_tags = n_tags;
  MR_HIP(hipSetDevice(device));
  MR_HIP(hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking));
  MR_HIP(hipEventCreate(&r->ev[0]));
  MR_HIP(hipEventCreate(&r->ev[1]));
  if (tc_dev_copy(&r->mid, cand_mid, n_cand, r->stream) ||
      tc_dev_copy(&r->med, cand_med, n_cand, r->stream) ||
      tc_dev_copy(&r->goff, reinterpret_cast<const int64_t*>(genre_off), n_cand + 1, r->stream) ||
      tc_dev_copy(&r->gidx, genre_idx, genre_off[n_cand], r->stream) ||
      tc_dev_copy(&r->toff, reinterpret_cast<const int64_t*>(tag_off), n_cand + 1, r->stream) ||
      tc_dev_copy(&r->tidx, tag_idx, tag_off[n_cand], r->stream) ||
      tc_dev_copy(&r->tval, tag_val, tag_off[n_cand], r->stream) ||
      tc_dev_copy(&r->gcount, genre_count, n_genres, r->stream) ||
      tc_dev_copy(&r->tcount, tag_count, n_tags, r->stream))
    return -1;
  MR_HIP(hipStreamSynchronize(r->stream));
  return 0;
}

static void tc_reset_ms(TagCount* r) {
  for (double& m : r->ms) m = 0.0;
}

// bytes of dense tag rows per launch (fit) or chunk (scores, evaluation)
constexpr int64_t kRowScratch = int64_t(1) << 30;

static int64_t tc_row_users(const TagCount* r) {
  return std::max<int64_t>(1, kRowScratch / (r->row_len() * 8));
}

static int tagcount_fit(TagCount* r, int n_users, const long long* off, const int* cand,
                        const double* ratings, double* genre_profile, long long* tp_off,
                        int* tp_idx, double* tp_val, long long tp_cap, double* x0, double* x1,
                        int* has0, int* has1, int* n0, int* rank0, int* rank1) {
  MR_CHECK(n_users >= 0, "tagcount: negative n_users");
  MR_CHECK(tp_cap >= 0, "tagcount: negative tp_cap");
  tc_reset_ms(r);
  tp_off[0] = 0;
  if (n_users == 0) return 0;
  MR_CHECK(rk_offsets_ok(off, n_users), "tagcount: rating offsets must start at 0 and not decrease");
  const int64_t nnz = off[n_users];
  for (int u = 0; u < n_users; ++u)
    MR_CHECK(off[u + 1] - off[u] <= (1 << 30), "tagcount: rating list too long");
  for (int64_t i = 0; i < nnz; ++i)
    MR_CHECK(cand[i] >= 0 && cand[i] < r->n_cand, "tagcount: rated candidate out of range");
  const int64_t B = std::min<int64_t>(tc_row_users(r), n_users), L = r->row_len();
  int64_t max_nnz = 0;
  for (int64_t u0 = 0; u0 < n_users; u0 += B)
    max_nnz = std::max<int64_t>(max_nnz, off[std::min<int64_t>(u0 + B, n_users)] - off[u0]);
  RkBuf<int> dcand, dcnt, dhas0, dhas1, dn0, drk0, drk1, cidx;
  RkBuf<int64_t> doff, dcoff;
  RkBuf<double> drat, drows, dgp, dwork, dx0, dx1, cval;
  if (doff.upload(reinterpret_cast<const int64_t*>(off), n_users + 1, r->stream) ||
      dcand.upload(cand, nnz, r->stream) || drat.upload(ratings, nnz, r->stream) ||
      drows.alloc(B * L) || dgp.alloc((int64_t)n_users * r->n_genres) ||
      dwork.alloc(7 * max_nnz) || dcnt.alloc(B) || dcoff.alloc(B + 1) ||
      dx0.alloc((int64_t)n_users * 3) || dx1.alloc((int64_t)n_users * 2) ||
      dhas0.alloc(n_users) || dhas1.alloc(n_users) || dn0.alloc(n_users) ||
      drk0.alloc(n_users) || drk1.alloc(n_users))
    return -1;
  const TcTable t = r->table();
  std::vector<int> cnt;
  std::vector<int64_t> coff;
  for (int64_t u0 = 0; u0 < n_users; u0 += B) {
    const int nb = (int)std::min<int64_t>(B, n_users - u0);
    MR_HIP(hipMemsetAsync(drows.p, 0, (size_t)nb * L * 8, r->stream));
    if (tc_timed(r, TC_PROFILE, [&]() {
          tagcount_profile_kernel<<<nb, TC_WAVE, 0, r->stream>>>(
              (int)u0, doff.p, dcand.p, drat.p, t, drows.p, dgp.p, dcnt.p);
        }) ||
        tc_timed(r, TC_FIT, [&]() {
          tagcount_fit_kernel<<<nb, TC_WAVE, 0, r->stream>>>(
              (int)u0, doff.p, dcand.p, drat.p, t, drows.p, dgp.p, dwork.p, dx0.p, dx1.p, dhas0.p,
              dhas1.p, dn0.p, drk0.p, drk1.p);
        }))
      return -1;
    cnt.assign(nb, 0);
    MR_D2H(cnt.data(), dcnt.p, (size_t)nb * 4, r->stream);
    MR_HIP(hipStreamSynchronize(r->stream));
    coff.assign(nb + 1, 0);
    for (int i = 0; i < nb; ++i) {
      coff[i + 1] = coff[i] + cnt[i];
      tp_off[u0 + i + 1] = tp_off[u0] + coff[i + 1];
    }
    MR_CHECK(tp_off[u0 + nb] <= tp_cap, "tagcount: tp_cap is too small for the tag profiles");
    if (coff[nb] == 0) continue;
    MR_H2D(dcoff.p, coff.data(), (size_t)(nb + 1) * 8, r->stream);
    if (cidx.alloc(coff[nb]) || cval.alloc(coff[nb])) return -1;
    if (tc_timed(r, TC_COMPACT, [&]() {
          tagcount_compact_kernel<<<nb, TC_WAVE, 0, r->stream>>>(r->n_tags, drows.p, dcoff.p,
                                                                 cidx.p, cval.p);
        }))
      return -1;
    MR_D2H(tp_idx + tp_off[u0], cidx.p, (size_t)coff[nb] * 4, r->stream);
    MR_D2H(tp_val + tp_off[u0], cval.p, (size_t)coff[nb] * 8, r->stream);
  }
  if (r->n_genres > 0)
    MR_D2H(genre_profile, dgp.p, (size_t)n_users * r->n_genres * 8, r->stream);
  MR_D2H(x0, dx0.p, (size_t)n_users * 3 * 8, r->stream);
  MR_D2H(x1, dx1.p, (size_t)n_users * 2 * 8, r->stream);
  MR_D2H(has0, dhas0.p, (size_t)n_users * 4, r->stream);
  MR_D2H(has1, dhas1.p, (size_t)n_users * 4, r->stream);
  MR_D2H(n0, dn0.p, (size_t)n_users * 4, r->stream);
  MR_D2H(rank0, drk0.p, (size_t)n_users * 4, r->stream);
  MR_D2H(rank1, drk1.p, (size_t)n_users * 4, r->stream);
  MR_HIP(hipStreamSynchronize(r->stream));
  return 0;
}

// The model arrays of a scoring call, as the caller passed them.
struct TcModels {
  int n;
  const double* gp;
  const long long* poff;
  const int* pidx;
  const double* pval;
  const double *x0, *x1;
  const int *has0, *has1;
};

static int tc_check_models(const TagCount* r, const TcModels& m) {
  MR_CHECK(m.n >= 0, "tagcount: negative n_users");
  if (m.n == 0) return 0;
  MR_CHECK(rk_offsets_ok(m.poff, m.n), "tagcount: profile offsets must start at 0 and not decrease");
  for (int u = 0; u < m.n; ++u) {
    MR_CHECK((m.has0[u] | m.has1[u] | 1) == 1, "tagcount: has0 / has1 must be 0 or 1");
    for (int64_t i = m.poff[u]; i < m.poff[u + 1]; ++i) {
      MR_CHECK(m.pidx[i] >= 0 && m.pidx[i] < r->n_tags, "tagcount: profile tag index out of range");
      MR_CHECK(i == m.poff[u] || m.pidx[i] > m.pidx[i - 1],
               "tagcount: profile tag indices must increase inside a user");
    }
  }
  return 0;
}

// Device copies of the models of one chunk of users, and their dense rows.
struct TcChunk {
  RkBuf<double> gp, x0, x1, pval, rows;
  RkBuf<int> has0, has1, pidx;
  RkBuf<int64_t> poff;
  std::vector<int64_t> loc;
  int alloc(const TagCount* r, const TcModels& m, int64_t B) {
    int64_t max_p = 0;
    for (int64_t u0 = 0; u0 < m.n; u0 += B)
      max_p = std::max<int64_t>(max_p, m.poff[std::min<int64_t>(u0 + B, m.n)] - m.poff[u0]);
    return gp.alloc(B * r->n_genres) || x0.alloc(B * 3) || x1.alloc(B * 2) || has0.alloc(B) ||
           has1.alloc(B) || poff.alloc(B + 1) || pidx.alloc(max_p) || pval.alloc(max_p) ||
           rows.alloc(B * r->row_len());
  }
  // users [u0, u0 + nb): uploads, then the profiles scattered into zeroed rows
  // (skipped when no model of the chunk has an x0: nothing reads them then)
  int load(TagCount* r, const TcModels& m, int64_t u0, int nb) {
    hipStream_t s = r->stream;
    if (r->n_genres > 0)
      MR_H2D(gp.p, m.gp + u0 * r->n_genres, (size_t)nb * r->n_genres * 8, s);
    MR_H2D(x0.p, m.x0 + u0 * 3, (size_t)nb * 3 * 8, s);
    MR_H2D(x1.p, m.x1 + u0 * 2, (size_t)nb * 2 * 8, s);
    MR_H2D(has0.p, m.has0 + u0, (size_t)nb * 4, s);
    MR_H2D(has1.p, m.has1 + u0, (size_t)nb * 4, s);
    if (!std::any_of(m.has0 + u0, m.has0 + u0 + nb, [](int h) { return h != 0; })) return 0;
    loc.assign(nb + 1, 0);
    for (int i = 0; i <= nb; ++i) loc[i] = m.poff[u0 + i] - m.poff[u0];   // offsets follow the chunk
    MR_H2D(poff.p, loc.data(), (size_t)(nb + 1) * 8, s);
    if (loc[nb] > 0) {
      MR_H2D(pidx.p, m.pidx + m.poff[u0], (size_t)loc[nb] * 4, s);
      MR_H2D(pval.p, m.pval + m.poff[u0], (size_t)loc[nb] * 8, s);
    }
    MR_HIP(hipMemsetAsync(rows.p, 0, (size_t)nb * r->row_len() * 8, s));
    if (loc[nb] == 0) return 0;
    return tc_timed(r, TC_SCATTER, [&]() {
      tagcount_scatter_kernel<<<nb, 256, 0, s>>>(r->n_tags, poff.p, pidx.p, pval.p, rows.p);
    });
  }
};

// users per score / select launch: the dense rows, the score grid's y extent
// and ~1 GiB of keys bound it
static int64_t tc_user_chunk(const TagCount* r) {
  const int64_t per = std::max<int64_t>(r->n_cand, 1) * 8;
  return std::max<int64_t>(
      1, std::min<int64_t>({tc_row_users(r), int64_t(65535), (int64_t(1) << 30) / per}));
}

static int tagcount_scores(TagCount* r, const TcModels& m, double* out) {
  if (tc_check_models(r, m)) return -1;
  tc_reset_ms(r);
  if (m.n == 0 || r->n_cand == 0) return 0;
  const int64_t B = std::min<int64_t>(tc_user_chunk(r), m.n);
  TcChunk ch;
  RkBuf<double> S;
  if (ch.alloc(r, m, B) || S.alloc(B * r->n_cand)) return -1;
  const TcTable t = r->table();
  for (int64_t u0 = 0; u0 < m.n; u0 += B) {
    const int nb = (int)std::min<int64_t>(B, m.n - u0);
    if (ch.load(r, m, u0, nb)) return -1;
    const dim3 grid((r->n_cand + 255) / 256, nb);
    if (tc_timed(r, TC_SCORE, [&]() {
          tagcount_score_kernel<false><<<grid, 256, 0, r->stream>>>(
              r->n_cand, t, ch.gp.p, ch.x0.p, ch.x1.p, ch.has0.p, ch.has1.p, ch.rows.p, S.p,
              nullptr, nullptr);
        }))
      return -1;
    MR_D2H(out + u0 * r->n_cand, S.p, (size_t)nb * r->n_cand * 8, r->stream);
  }
  MR_HIP(hipStreamSynchronize(r->stream));
  return 0;
}

static int tagcount_top_n(TagCount* r, const TcModels& m, const long long* excl_off,
                          const int* excl_cand, int N, int* out_mid, double* out_score,
                          int* out_count) {
  if (tc_check_models(r, m)) return -1;
  MR_CHECK(N >= 1 && N <= kRecMaxResults, "tagcount: num_results must be in 1..1024");
  tc_reset_ms(r);
  if (m.n == 0) return 0;
  if (r->n_cand == 0) {
    std::fill(out_count, out_count + m.n, 0);
    return 0;
  }
  const int64_t B = std::min<int64_t>(tc_user_chunk(r), m.n);
  TcChunk ch;
  if (ch.alloc(r, m, B)) return -1;
  const TcTable t = r->table();
  return top_n_chunked(
      "tagcount", r->stream, r->n_cand, r->mid, m.n, B, excl_off, excl_cand, N, out_mid,
      out_score, out_count,
      [&](int64_t u0, int nb, uint64_t* keys, unsigned long long* kmin,
          unsigned long long* kmax) -> int {
        if (ch.load(r, m, u0, nb)) return -1;
        const dim3 grid((r->n_cand + 255) / 256, nb);
        return tc_timed(r, TC_SCORE, [&]() {
          launch_rec_range_init(r->stream, nb, kmin, kmax);
          tagcount_score_kernel<true><<<grid, 256, 0, r->stream>>>(
              r->n_cand, t, ch.gp.p, ch.x0.p, ch.x1.p, ch.has0.p, ch.has1.p, ch.rows.p, keys, kmin,
              kmax);
        });
      },
      [&](int stage, auto&& launch) {
        return tc_timed(r, stage == TOPN_EXCL ? TC_EXCL : TC_SELECT, launch);
      });
}

static int tagcount_evaluate(TagCount* r, const TcModels& m, const long long* off,
                             const int* cand, const double* actual, double* agreement,
                             long long* n_agree, long long* n_dis, double* pred, double* sse,
                             long long* n_pred) {
  if (tc_check_models(r, m)) return -1;
  tc_reset_ms(r);
  const int n_test = m.n;
  if (n_test == 0) return 0;
  MR_CHECK(rk_offsets_ok(off, n_test), "tagcount: test offsets must start at 0 and not decrease");
  const int64_t nnz = off[n_test];
  for (int64_t i = 0; i < nnz; ++i)
    MR_CHECK(cand[i] >= -1 && cand[i] < r->n_cand, "tagcount: evaluation candidate out of range");
  const int64_t B = std::min<int64_t>(tc_row_users(r), n_test);
  TcChunk ch;
  RkBuf<int> dcand;
  RkBuf<int64_t> doff;
  RkBuf<double> dact, dpred, dagr, dsse;
  RkBuf<long long> dag, ddis, dnp;
  if (ch.alloc(r, m, B) ||
      doff.upload(reinterpret_cast<const int64_t*>(off), n_test + 1, r->stream) ||
      dcand.upload(cand, nnz, r->stream) || dact.upload(actual, nnz, r->stream) ||
      dpred.alloc(nnz) || dagr.alloc(n_test) || dsse.alloc(n_test) || dag.alloc(n_test) ||
      ddis.alloc(n_test) || dnp.alloc(n_test))
    return -1;
  const TcTable t = r->table();
  for (int64_t u0 = 0; u0 < n_test; u0 += B) {
    const int nb = (int)std::min<int64_t>(B, n_test - u0);
    if (ch.load(r, m, u0, nb)) return -1;
    if (tc_timed(r, TC_EVAL, [&]() {
          tagcount_pred_kernel<<<nb, 256, 0, r->stream>>>((int)u0, t, ch.gp.p, ch.x0.p, ch.x1.p,
                                                          ch.has0.p, ch.has1.p, ch.rows.p, doff.p,
                                                          dcand.p, dpred.p);
        }))
      return -1;
  }
  if (tc_timed(r, TC_EVAL, [&]() {
        launch_rank_agreement(r->stream, n_test, doff.p, dact.p, dpred.p, dagr.p, dag.p, ddis.p,
                              dsse.p, dnp.p);
      }))
    return -1;
  MR_D2H(agreement, dagr.p, (size_t)n_test * 8, r->stream);
  MR_D2H(n_agree, dag.p, (size_t)n_test * 8, r->stream);
  MR_D2H(n_dis, ddis.p, (size_t)n_test * 8, r->stream);
  if (pred && nnz > 0) MR_D2H(pred, dpred.p, (size_t)nnz * 8, r->stream);
  if (sse) MR_D2H(sse, dsse.p, (size_t)n_test * 8, r->stream);
  if (n_pred) MR_D2H(n_pred, dnp.p, (size_t)n_test * 8, r->stream);
  MR_HIP(hipStreamSynchronize(r->stream));
  return 0;
}

}  // namespace mr

// ---------------------------------------------------------------------------
// C ABI (include/mr_tagcount.h)
// ---------------------------------------------------------------------------
struct mr_tagcount {
  mr::TagCount r;
};

extern "C" {

mr_tagcount* mr_tagcount_create(int device, int n_cand, const int* cand_mid,
                                const double* cand_med, const long long* genre_off,
                                const int* genre_idx, const long long* tag_off,
                                const int* tag_idx, const double* tag_val, int n_genres,
                                const double* genre_count, int n_tags, const double* tag_count) {
  mr_tagcount* ctx = nullptr;
  const int rc = mr::rk_guard([&]() -> int {
    ctx = new mr_tagcount();
    return mr::tagcount_init(&ctx->r, device, n_cand, cand_mid, cand_med, genre_off, genre_idx,
                             tag_off, tag_idx, tag_val, n_genres, genre_count, n_tags, tag_count);
  });
  if (rc) {
    delete ctx;
    return nullptr;
  }
  return ctx;
}

void mr_tagcount_destroy(mr_tagcount* ctx) { delete ctx; }

int mr_tagcount_num_candidates(const mr_tagcount* ctx) { return ctx ? ctx->r.n_cand : -1; }

int mr_tagcount_fit(mr_tagcount* ctx, int n_users, const long long* off, const int* cand,
                    const double* ratings, double* genre_profile, long long* tp_off,
                    int* tp_idx, double* tp_val, long long tp_cap, double* x0, double* x1,
                    int* has0, int* has1, int* n0, int* rank0, int* rank1) {
  if (!ctx) return -1;
  return mr::rk_guard([&]() {
    return mr::tagcount_fit(&ctx->r, n_users, off, cand, ratings, genre_profile, tp_off, tp_idx,
                            tp_val, tp_cap, x0, x1, has0, has1, n0, rank0, rank1);
  });
}

int mr_tagcount_scores(mr_tagcount* ctx, int n_users, const double* genre_profile,
                       const long long* tp_off, const int* tp_idx, const double* tp_val,
                       const double* x0, const double* x1, const int* has0, const int* has1,
                       double* out) {
  if (!ctx) return -1;
  const mr::TcModels m{n_users, genre_profile, tp_off, tp_idx, tp_val, x0, x1, has0, has1};
  return mr::rk_guard([&]() { return mr::tagcount_scores(&ctx->r, m, out); });
}

int mr_tagcount_top_n(mr_tagcount* ctx, int n_users, const double* genre_profile,
                      const long long* tp_off, const int* tp_idx, const double* tp_val,
                      const double* x0, const double* x1, const int* has0, const int* has1,
                      const long long* excl_off, const int* excl_cand, int num_results,
                      int* out_mid, double* out_score, int* out_count) {
  if (!ctx) return -1;
  const mr::TcModels m{n_users, genre_profile, tp_off, tp_idx, tp_val, x0, x1, has0, has1};
  return mr::rk_guard([&]() {
    return mr::tagcount_top_n(&ctx->r, m, excl_off, excl_cand, num_results, out_mid, out_score,
                              out_count);
  });
}

int mr_tagcount_evaluate(mr_tagcount* ctx, int n_test, const double* genre_profile,
                         const long long* tp_off, const int* tp_idx, const double* tp_val,
                         const double* x0, const double* x1, const int* has0, const int* has1,
                         const long long* off, const int* cand, const double* actual,
                         double* agreement, long long* n_agree, long long* n_disagree,
                         double* pred, double* sse, long long* n_pred) {
  if (!ctx) return -1;
  const mr::TcModels m{n_test, genre_profile, tp_off, tp_idx, tp_val, x0, x1, has0, has1};
  return mr::rk_guard([&]() {
    return mr::tagcount_evaluate(&ctx->r, m, off, cand, actual, agreement, n_agree, n_disagree,
                                 pred, sse, n_pred);
  });
}

int mr_tagcount_last_kernel_ms(const mr_tagcount* ctx, double* ms8) {
  if (!ctx || !ms8) return -1;
  for (int i = 0; i < mr::TC_N; ++i) ms8[i] = ctx->r.ms[i];
  return 0;
}

}  // extern "C"
