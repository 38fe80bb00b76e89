// Content model on MI355X (gfx950): the reference's per-user tag least-squares
// recommender.  C ABI: include/mr_content.h.  Reference behaviour:
//   model   python/app_local/models.py:342-640 (== full_data/tag_ls_predictor.py)
//   eval    python/full_data/worker_process.py:421-461
//
// One wave per user throughout the fit.  K-C1 counts the feature ids of the
// user's rated movies (exact integers) and keeps the (count, id) descending
// prefix; K-C2 builds the user's sparse rows of A and runs LSQR (Paige &
// Saunders, as scipy.sparse.linalg.lsqr documents it) with the whole
// iteration loop inside the kernel.  Every floating-point sum has a fixed
// order that depends on the user's own list only -- lane-strided row
// partials, then a butterfly or an in-order column sum; no atomics -- so a
// list gives the same bits alone, in any batch and from run to run.
// K-C3 / K-C4 score candidates from (profile, x) in the order the header
// defines; top-N and the agreement are the kernels of serving.hip.
//
// No multiply-add is contracted anywhere in this file: the scores are defined
// with separate roundings, and LSQR follows SciPy's operation sequence.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

#include "../../include/mr_als.h"
#include "../../include/mr_content.h"
#include "mr_internal.h"
#include "serving_device.h"

namespace mr {

constexpr int CT_MAXF = MR_CONTENT_MAX_FACTORS, CT_ROW = MR_CONTENT_ROW;
constexpr int CT_CH = 4096;   // feature counters in LDS per pass of K-C1

// _decide_num_factors (models.py:416-442): 5 factors per bracket of 10, 20,
// 40, 80, 160 ratings, one per 2, 4, 8, 16, 32 ratings inside a bracket.
__host__ __device__ inline int content_num_factors(int64_t n) {
  int nf = 0;
  int64_t width = 10;
  int mult = 2;
  for (int b = 0; b < 5; ++b) {
    if (n <= width) return nf + (int)(n / mult);
    nf += 5;
    n -= width;
    width *= 2;
    mult *= 2;
  }
  return nf;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Position of feature id `id` in the candidate's ascending ids [f0, f0 + nf), or -1.
__device__ __forceinline__ int64_t find_feature(const int* __restrict__ fid, int64_t f0, int nf,
                                                int id) {
  int lo = 0, hi = nf;
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (fid[f0 + m] < id) lo = m + 1;
    else hi = m;
  }
  return (lo < nf && fid[f0 + lo] == id) ? f0 + lo : -1;
}

// ---------------------------------------------------------------------------
// K-C1: profile of one user per wave.  The table's distinct feature ids are
// numbered 0 .. nfd-1 in ascending id order (fidx = that number per feature
// entry).  Per pass the counters of CT_CH of them sit in LDS; the user's
// movies are walked one after the other, the lanes taking one movie's
// features -- distinct inside a movie, so two lanes never meet on a counter
// and a movie listed twice counts twice.  The running top list lives in
// registers, lane j holding the j-th largest key (count << 32 | id); a
// counter that beats the last kept key is inserted by a shift through the
// lanes.  Keys are distinct, so the result does not depend on insertion order.
//
// The counters are plain LDS read-modify-writes with no barrier between
// movies: two consecutive movies may share a feature, and then DIFFERENT
// lanes touch the same counter one movie after the other.  That is ordered
// only because the block is exactly one 64-wide wave (CT_WAVE), whose LDS
// operations complete in program order; with a second wave in the block it
// would be a race.  The kernel and its launch both take the block size from
// CT_WAVE, and the lane shuffles of the top list assume the same.
// ---------------------------------------------------------------------------
constexpr int CT_WAVE = 64;   // block size of K-C1 and K-C2: one wave, never more
static_assert(CT_WAVE == 64, "K-C1 / K-C2 are written for a block of exactly one 64-wide wave");

__global__ __launch_bounds__(CT_WAVE) void content_profile_kernel(
    const int* __restrict__ order, const int64_t* __restrict__ off, const int* __restrict__ cand,
    const int64_t* __restrict__ foff, const int* __restrict__ fidx,
    const int* __restrict__ distinct_id, int nfd, int* __restrict__ p_out,
    int* __restrict__ profile_out) {
  __shared__ unsigned cnt[CT_CH];
  const int u = order[blockIdx.x], lane = threadIdx.x;
  const int64_t b = off[u];
  const int n = (int)(off[u + 1] - b);
  const int nfac = content_num_factors(n);
  unsigned long long key = 0;
  for (int lo = 0; lo < nfd && nfac > 0; lo += CT_CH) {
    const int lim = min(CT_CH, nfd - lo);
    for (int t = lane; t < CT_CH; t += CT_WAVE) cnt[t] = 0;
    __syncthreads();
    for (int i = 0; i < n; ++i) {
      const int c = cand[b + i];
      const int64_t f0 = foff[c];
      const int nf = (int)(foff[c + 1] - f0);
      for (int t = lane; t < nf; t += CT_WAVE) {
        const unsigned idx = (unsigned)(fidx[f0 + t] - lo);
        if (idx < (unsigned)CT_CH) cnt[idx] += 1;   // one wave: in program order (see above)
      }
    }
    __syncthreads();
    for (int t0 = 0; t0 < lim; t0 += 64) {
      const int t = t0 + lane;
      const unsigned cv = t < lim ? cnt[t] : 0u;
      const unsigned long long k =
          cv ? ((unsigned long long)cv << 32) | (unsigned)distinct_id[lo + min(t, lim - 1)] : 0ull;
      bool pending = k > (unsigned long long)__shfl(key, nfac - 1, 64);
      unsigned long long mask;
      while ((mask = __ballot(pending)) != 0) {
        const int src = __ffsll((long long)mask) - 1;
        const unsigned long long K = __shfl(k, src, 64);
        if (lane == src) pending = false;
        if (K > (unsigned long long)__shfl(key, nfac - 1, 64)) {
          const int pos = __popcll(__ballot(key > K));
          const unsigned long long up = __shfl_up(key, 1, 64);
          key = lane < pos ? key : (lane == pos ? K : up);
        }
      }
    }
    __syncthreads();
  }
  const bool kept = lane < nfac && (key >> 32) != 0;
  const int p = __popcll(__ballot(kept));
  if (lane < CT_MAXF) profile_out[(int64_t)u * CT_MAXF + lane] = kept ? (int)(unsigned)key : -1;
  if (lane == 0) p_out[u] = p;
}

// ---------------------------------------------------------------------------
// K-C2: LSQR of one user per wave (scipy/sparse/linalg/_isolve/lsqr.py with
// damp = 0, x0 = 0).  Row i of A belongs to lane i mod 64 in both products, so
// u_i is only ever touched by its own lane and lives in global scratch
// whatever the list length; A's row entries (column, value), at most pcap =
// num_factors(n) per row, are stored entry-major (entry e of row i at
// e * n + i) so the lanes read them coalesced.  v, w, x: lane j holds
// coordinate j (j = p is the bias); v is mirrored in LDS for the row dots.
// A^T u: every lane adds its rows into its own LDS column of partials, then
// lane j adds the 64 partials of coordinate j in lane order.
// ---------------------------------------------------------------------------
struct FitParams {
  double atol, btol, conlim;
  int iter_lim;
};

__global__ __launch_bounds__(CT_WAVE) void content_fit_kernel(
    const int* __restrict__ order, const int64_t* __restrict__ off, const int* __restrict__ cand,
    const double* __restrict__ rating, const int64_t* __restrict__ foff,
    const int* __restrict__ fid, const double* __restrict__ fval, const double* __restrict__ med,
    const int* __restrict__ p_in, const int* __restrict__ profile, FitParams prm,
    const int* __restrict__ iter_lim_each, const int64_t* __restrict__ abase,
    unsigned char* __restrict__ a_col, double* __restrict__ a_val, int* __restrict__ a_n,
    double* __restrict__ uvec, double* __restrict__ x_out, int* __restrict__ itn_out,
    int* __restrict__ istop_out) {
  __shared__ double part[CT_ROW][65];
  __shared__ double vs[CT_ROW];
  __shared__ int prof[CT_MAXF];
  const int slot = blockIdx.x, u = order[slot], lane = threadIdx.x;
  const int64_t b = off[u];
  const int n = (int)(off[u + 1] - b);
  const int p = p_in[u];
  const int iter_lim = iter_lim_each ? iter_lim_each[u] : prm.iter_lim;
  unsigned char* ac = a_col + abase[slot];
  double* av = a_val + abase[slot];
  int* an = a_n + b;
  double* uu = uvec + b;
  if (lane < CT_MAXF) prof[lane] = lane < p ? profile[(int64_t)u * CT_MAXF + lane] : -1;
  __syncthreads();
  // rows of A in profile order, b = rating - median (models.py:492-532)
  double bb = 0.0;
  for (int i = lane; i < n; i += 64) {
    const int c = cand[b + i];
    const int64_t f0 = foff[c];
    const int nf = (int)(foff[c + 1] - f0);
    int e = 0;
    for (int j = 0; j < p && nf > 0; ++j) {
      const int64_t pos = find_feature(fid, f0, nf, prof[j]);
      if (pos >= 0) {
        ac[(int64_t)e * n + i] = (unsigned char)j;
        av[(int64_t)e * n + i] = fval[pos];
        ++e;
      }
    }
    an[i] = e;
    const double bi = rating[b + i] - med[c];
    uu[i] = bi;
    bb += bi * bi;
  }
  const double eps = 2.220446049250313e-16;
  const double ctol = prm.conlim > 0.0 ? 1.0 / prm.conlim : 0.0;
  const double bnorm = sqrt(wave_sum_f64(bb));
  double x = 0.0, v = 0.0, w = 0.0;
  double beta = bnorm, alfa = 0.0;
  int itn = 0, istop = 0;

  // v_j = sum_i A_ij u_i for lane j <= p (0 on the other lanes)
  auto rmatvec = [&]() -> double {
    for (int j = 0; j <= p; ++j) part[j][lane] = 0.0;
    for (int i = lane; i < n; i += 64) {
      const double ui = uu[i];
      const int ne = an[i];
      for (int e = 0; e < ne; ++e) {
        const int j = ac[(int64_t)e * n + i];
        part[j][lane] += av[(int64_t)e * n + i] * ui;
      }
      part[p][lane] += ui;
    }
    __syncthreads();
    double s = 0.0;
    if (lane <= p)
      for (int t = 0; t < 64; ++t) s += part[lane][t];
    __syncthreads();
    return s;
  };

  if (beta > 0.0) {
    const double rb = 1.0 / beta;
    for (int i = lane; i < n; i += 64) uu[i] = rb * uu[i];
    v = rmatvec();
    alfa = sqrt(wave_sum_f64(v * v));
  }
  if (alfa > 0.0) v = (1.0 / alfa) * v;
  w = v;
  double rhobar = alfa, phibar = beta;
  double anorm = 0.0, ddnorm = 0.0, xnorm = 0.0, xxnorm = 0.0, z = 0.0, cs2 = -1.0, sn2 = 0.0;
  if (alfa * beta != 0.0) {
    while (itn < iter_lim) {
      ++itn;
      // u = A v - alfa u
      if (lane <= p) vs[lane] = v;
      __syncthreads();
      double uu2 = 0.0;
      for (int i = lane; i < n; i += 64) {
        const int ne = an[i];
        double s = 0.0;
        for (int e = 0; e < ne; ++e) s += av[(int64_t)e * n + i] * vs[ac[(int64_t)e * n + i]];
        s += vs[p];
        const double ui = s - alfa * uu[i];
        uu[i] = ui;
        uu2 += ui * ui;
      }
      __syncthreads();
      beta = sqrt(wave_sum_f64(uu2));
      if (beta > 0.0) {
        const double rb = 1.0 / beta;
        for (int i = lane; i < n; i += 64) uu[i] = rb * uu[i];
        anorm = sqrt(anorm * anorm + alfa * alfa + beta * beta + 0.0);
        v = rmatvec() - beta * v;
        alfa = sqrt(wave_sum_f64(v * v));
        if (alfa > 0.0) v = (1.0 / alfa) * v;
      }
      // plane rotation (_sym_ortho(rhobar, beta); beta >= 0)
      double cs, sn, rho;
      if (beta == 0.0) {
        cs = rhobar > 0.0 ? 1.0 : (rhobar < 0.0 ? -1.0 : 0.0);
        sn = 0.0;
        rho = fabs(rhobar);
      } else if (rhobar == 0.0) {
        cs = 0.0;
        sn = 1.0;
        rho = beta;
      } else if (beta > fabs(rhobar)) {
        const double tau = rhobar / beta;
        sn = 1.0 / sqrt(1.0 + tau * tau);
        cs = sn * tau;
        rho = beta / sn;
      } else {
        const double tau = beta / rhobar;
        cs = (rhobar > 0.0 ? 1.0 : -1.0) / sqrt(1.0 + tau * tau);
        sn = cs * tau;
        rho = rhobar / cs;
      }
      const double theta = sn * alfa;
      rhobar = -cs * alfa;
      const double phi = cs * phibar;
      phibar = sn * phibar;
      const double tau = sn * phi;
      const double t1 = phi / rho, t2 = -theta / rho;
      const double dk = (1.0 / rho) * w;
      x = x + t1 * w;
      w = v + t2 * w;
      const double nd = sqrt(wave_sum_f64(dk * dk));
      ddnorm = ddnorm + nd * nd;
      const double delta = sn2 * rho, gambar = -cs2 * rho;
      const double rhs = phi - delta * z;
      const double zbar = rhs / gambar;
      xnorm = sqrt(xxnorm + zbar * zbar);
      const double gamma = sqrt(gambar * gambar + theta * theta);
      cs2 = gambar / gamma;
      sn2 = theta / gamma;
      z = rhs / gamma;
      xxnorm = xxnorm + z * z;
      const double acond = anorm * sqrt(ddnorm);
      const double rnorm = sqrt(phibar * phibar + 0.0);
      const double arnorm = alfa * fabs(tau);
      const double test1 = rnorm / bnorm;
      const double test2 = arnorm / (anorm * rnorm + eps);
      const double test3 = 1.0 / (acond + eps);
      const double t1b = test1 / (1.0 + anorm * xnorm / bnorm);
      const double rtol = prm.btol + prm.atol * anorm * xnorm / bnorm;
      if (itn >= iter_lim) istop = 7;
      if (1.0 + test3 <= 1.0) istop = 6;
      if (1.0 + test2 <= 1.0) istop = 5;
      if (1.0 + t1b <= 1.0) istop = 4;
      if (test3 <= ctol) istop = 3;
      if (test2 <= prm.atol) istop = 2;
      if (test1 <= rtol) istop = 1;
      if (istop != 0) break;
    }
  }
  if (lane < CT_ROW) x_out[(int64_t)u * CT_ROW + lane] = lane <= p ? x : 0.0;
  if (lane == 0) {
    itn_out[u] = itn;
    istop_out[u] = istop;
  }
}

// ---------------------------------------------------------------------------
// K-C3 / K-C4: scores from (profile, x).  s = 0; for j = 0 .. p-1 in profile
// order, s += attr_j * x_j where the movie has feature j (a skipped zero term
// adds nothing to a finite sum); s += x_bias; s += median.  Profile ids must
// be distinct (a fit's are; check_models refuses others).
// ---------------------------------------------------------------------------
// The user's model in LDS: x, the profile, and the profile's ids in ascending
// order with their positions (for the search from a movie's feature).
struct ModelLds {
  double xs[CT_ROW];
  int prof[CT_MAXF];
  int sid[CT_MAXF];
  int sj[CT_MAXF];
};

__device__ __forceinline__ void load_model(int u, const int* __restrict__ p_in,
                                           const int* __restrict__ profile,
                                           const double* __restrict__ X, ModelLds& m) {
  const int p = p_in[u];
  for (int j = threadIdx.x; j < CT_ROW; j += blockDim.x) {
    m.xs[j] = X[(int64_t)u * CT_ROW + j];
    if (j < p) {
      // ids are distinct: an id's place in ascending order is the number below it
      const int id = profile[(int64_t)u * CT_MAXF + j];
      int rank = 0;
      for (int q = 0; q < p; ++q) rank += profile[(int64_t)u * CT_MAXF + q] < id ? 1 : 0;
      m.prof[j] = id;
      m.sid[rank] = id;
      m.sj[rank] = j;
    }
  }
  __syncthreads();
}

// The movie's features are matched against the profile first (one read per
// feature, the profile search in LDS); the matched profile positions are then
// added in ascending j, which is the defined order.  A match is found at
// feature t, but the terms are needed in order of j, not of t: keeping t per
// matched j would take a per-thread array of up to 25 positions indexed by a
// run-time j, which the compiler places in scratch memory.  So only the bit
// mask is kept and each matched j (few per movie) searches the movie's short
// id list again; those reads hit the lines the first loop just loaded.  The
// search cannot miss for distinct profile ids (check_models); `pos >= 0` only
// keeps a violated precondition from becoming a read before the table.
__device__ __forceinline__ double content_score(int c, int p, const ModelLds& m,
                                                const int64_t* __restrict__ foff,
                                                const int* __restrict__ fid,
                                                const double* __restrict__ fval,
                                                const double* __restrict__ med) {
  const int64_t f0 = foff[c];
  const int nf = (int)(foff[c + 1] - f0);
  unsigned match = 0;
  for (int t = 0; t < nf && p > 0; ++t) {
    const int id = fid[f0 + t];
    int lo = 0, hi = p;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (m.sid[mid] < id) lo = mid + 1;
      else hi = mid;
    }
    if (lo < p && m.sid[lo] == id) match |= 1u << m.sj[lo];
  }
  double s = 0.0;
  while (match) {
    const int j = __ffs((int)match) - 1;
    match &= match - 1;
    const int64_t pos = find_feature(fid, f0, nf, m.prof[j]);
    if (pos >= 0) s = add_rn(s, mul_rn(fval[pos], m.xs[j]));
  }
  return add_rn(add_rn(s, m.xs[p]), med[c]);
}

template <bool KEYS>
__global__ __launch_bounds__(256) void content_score_kernel(
    int n_cand, const int* __restrict__ p_in, const int* __restrict__ profile,
    const double* __restrict__ X, const int64_t* __restrict__ foff, const int* __restrict__ fid,
    const double* __restrict__ fval, const double* __restrict__ med, void* __restrict__ out,
    unsigned long long* __restrict__ kmin, unsigned long long* __restrict__ kmax) {
  __shared__ ModelLds m;
  const int u = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  load_model(u, p_in, profile, X, m);
  unsigned long long lo = ~0ull, hi = 0ull;
  if (c < n_cand) {
    const double s = content_score(c, p_in[u], m, foff, fid, fval, med);
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

// one block per test user: predictions of its test ratings (NaN: no median)
__global__ __launch_bounds__(256) void content_pred_kernel(
    const int* __restrict__ p_in, const int* __restrict__ profile, const double* __restrict__ X,
    const int64_t* __restrict__ off, const int* __restrict__ cand,
    const int64_t* __restrict__ foff, const int* __restrict__ fid,
    const double* __restrict__ fval, const double* __restrict__ med, double* __restrict__ pred) {
  __shared__ ModelLds m;
  const int t = blockIdx.x;
  load_model(t, p_in, profile, X, m);
  const int p = p_in[t];
  const int64_t e = off[t + 1];
  for (int64_t i = off[t] + threadIdx.x; i < e; i += 256) {
    const int c = cand[i];
    pred[i] = c >= 0 ? content_score(c, p, m, foff, fid, fval, med) : NAN;
  }
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
enum { CT_PROFILE = 0, CT_FIT, CT_SCORE, CT_EXCL, CT_SELECT, CT_EVAL, CT_N };

struct Content {
  int device = 0, n_cand = 0, nfd = 0;
  int64_t n_feat = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  int *mid = nullptr, *fid = nullptr, *fidx = nullptr, *distinct_id = nullptr;
  double *med = nullptr, *fval = nullptr;
  int64_t* foff = nullptr;
  std::vector<int64_t> h_foff;
  double ms[CT_N] = {0};
  ~Content() {
    if (stream) {
      (void)hipFree(mid);
      (void)hipFree(fid);
      (void)hipFree(fidx);
      (void)hipFree(distinct_id);
      (void)hipFree(med);
      (void)hipFree(fval);
      (void)hipFree(foff);
      (void)hipStreamDestroy(stream);
    }
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

template <typename F>
static int ct_timed(Content* r, int cls, F&& launch) {
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
static int ct_dev_copy(T** dst, const T* src, int64_t n, hipStream_t s) {
  MR_HIP(hipMalloc((void**)dst, (size_t)std::max<int64_t>(n, 1) * sizeof(T)));
  if (n > 0) MR_H2D(*dst, src, (size_t)n * sizeof(T), s);
  return 0;
}

static int content_init(Content* r, int device, int n_cand, const int* cand_mid,
                        const double* cand_med, const long long* feat_off, const int* feat_id,
                        const double* feat_val) {
  MR_CHECK(n_cand >= 0, "content: negative n_cand");
  MR_CHECK(rk_offsets_ok(feat_off, n_cand), "content: feature offsets must start at 0 and not decrease");
  const int64_t nf = feat_off[n_cand];
  {
    std::vector<int> seen(cand_mid, cand_mid + n_cand);
    std::sort(seen.begin(), seen.end());
    MR_CHECK(std::adjacent_find(seen.begin(), seen.end()) == seen.end(),
             "content: candidate movie ids must be unique");
    MR_CHECK(n_cand == 0 || seen.front() >= 0, "content: movie ids must be >= 0");
  }
  for (int c = 0; c < n_cand; ++c)
    for (int64_t i = feat_off[c]; i < feat_off[c + 1]; ++i) {
      MR_CHECK(feat_id[i] >= 0, "content: feature ids must be >= 0");
      MR_CHECK(i == feat_off[c] || feat_id[i] > feat_id[i - 1],
               "content: feature ids must increase inside a candidate");
    }
  // distinct ids, ascending, and every entry's number among them
  std::vector<int> distinct(feat_id, feat_id + nf);
  std::sort(distinct.begin(), distinct.end());
  distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
  std::vector<int> fidx((size_t)nf);
  for (int64_t i = 0; i < nf; ++i)
    fidx[i] = (int)(std::lower_bound(distinct.begin(), distinct.end(), feat_id[i]) -
                    distinct.begin());
  r->device = device;
  r->n_cand = n_cand;
  r->n_feat = nf;
  r->nfd = (int)distinct.size();
  r->h_foff.assign(feat_off, feat_off + n_cand + 1);
  MR_HIP(hipSetDevice(device));
  MR_HIP(hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking));
  MR_HIP(hipEventCreate(&r->ev[0]));
  MR_HIP(hipEventCreate(&r->ev[1]));
  if (ct_dev_copy(&r->mid, cand_mid, n_cand, r->stream) ||
      ct_dev_copy(&r->med, cand_med, n_cand, r->stream) ||
      ct_dev_copy(&r->foff, r->h_foff.data(), n_cand + 1, r->stream) ||
      ct_dev_copy(&r->fid, feat_id, nf, r->stream) ||
      ct_dev_copy(&r->fval, feat_val, nf, r->stream) ||
      ct_dev_copy(&r->fidx, fidx.data(), nf, r->stream) ||
      ct_dev_copy(&r->distinct_id, distinct.data(), r->nfd, r->stream))
    return -1;
  MR_HIP(hipStreamSynchronize(r->stream));
  return 0;
}

static void ct_reset_ms(Content* r) {
  for (double& m : r->ms) m = 0.0;
}

// entries of A scratch per fit launch (9 bytes each)
constexpr int64_t kFitScratch = int64_t(48) << 20;

static int content_fit(Content* r, int n_users, const long long* off, const int* cand,
                       const double* ratings, double atol, double btol, double conlim,
                       int iter_lim, const int* iter_lim_each, int* p_out, int* profile_out,
                       double* x_out, int* itn_out, int* istop_out) {
  MR_CHECK(n_users >= 0, "content: negative n_users");
  MR_CHECK(iter_lim >= 0, "content: negative iter_lim");
  MR_CHECK(atol >= 0.0 && btol >= 0.0 && conlim >= 0.0, "content: atol, btol, conlim must be >= 0");
  ct_reset_ms(r);
  if (n_users == 0) return 0;
  MR_CHECK(rk_offsets_ok(off, n_users), "content: rating offsets must start at 0 and not decrease");
  const int64_t nnz = off[n_users];
  for (int u = 0; u < n_users; ++u) {
    MR_CHECK(off[u + 1] - off[u] >= 2, "content: a rating list needs at least 2 ratings");
    MR_CHECK(off[u + 1] - off[u] <= (1 << 30), "content: rating list too long");
    MR_CHECK(!iter_lim_each || iter_lim_each[u] >= 0, "content: negative iter_lim");
  }
  for (int64_t i = 0; i < nnz; ++i)
    MR_CHECK(cand[i] >= 0 && cand[i] < r->n_cand, "content: rated candidate out of range");
  // longest lists first (stable, so the schedule is a function of the lengths)
  std::vector<int> order(n_users);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
    return off[a + 1] - off[a] > off[b + 1] - off[b];
  });
  std::vector<int64_t> abase(n_users);
  int64_t max_scr = 1;
  for (int s0 = 0; s0 < n_users;) {   // launches: as many users as the A scratch holds
    int64_t tot = 0;
    int s1 = s0;
    while (s1 < n_users) {
      const int64_t n = off[order[s1] + 1] - off[order[s1]];
      const int64_t need = n * std::max(1, content_num_factors(n));
      if (s1 > s0 && tot + need > kFitScratch) break;
      abase[s1] = tot;
      tot += need;
      ++s1;
    }
    max_scr = std::max(max_scr, tot);
    s0 = s1;
  }
  RkBuf<int> dorder, dcand, dp, dprof, ditn, distop, dlim, dan;
  RkBuf<int64_t> doff, dabase;
  RkBuf<double> drat, dx, dav, duv;
  RkBuf<unsigned char> dac;
  if (dorder.upload(order.data(), n_users, r->stream) ||
      doff.upload(reinterpret_cast<const int64_t*>(off), n_users + 1, r->stream) ||
      dcand.upload(cand, nnz, r->stream) || drat.upload(ratings, nnz, r->stream) ||
      dabase.upload(abase.data(), n_users, r->stream) || dp.alloc(n_users) ||
      dprof.alloc((int64_t)n_users * CT_MAXF) || dx.alloc((int64_t)n_users * CT_ROW) ||
      ditn.alloc(n_users) || distop.alloc(n_users) || dan.alloc(nnz) || duv.alloc(nnz) ||
      dac.alloc(max_scr) || dav.alloc(max_scr))
    return -1;
  if (iter_lim_each && dlim.upload(iter_lim_each, n_users, r->stream)) return -1;
  if (ct_timed(r, CT_PROFILE, [&]() {
        content_profile_kernel<<<n_users, CT_WAVE, 0, r->stream>>>(dorder.p, doff.p, dcand.p, r->foff,
                                                              r->fidx, r->distinct_id, r->nfd,
                                                              dp.p, dprof.p);
      }))
    return -1;
  const FitParams prm{atol, btol, conlim, iter_lim};
  for (int s0 = 0; s0 < n_users;) {
    int s1 = s0 + 1;
    while (s1 < n_users && abase[s1] != 0) ++s1;
    if (ct_timed(r, CT_FIT, [&]() {
          content_fit_kernel<<<s1 - s0, CT_WAVE, 0, r->stream>>>(
              dorder.p + s0, doff.p, dcand.p, drat.p, r->foff, r->fid, r->fval, r->med, dp.p,
              dprof.p, prm, iter_lim_each ? dlim.p : nullptr, dabase.p + s0, dac.p, dav.p, dan.p,
              duv.p, dx.p, ditn.p, distop.p);
        }))
      return -1;
    s0 = s1;
  }
  MR_D2H(p_out, dp.p, (size_t)n_users * 4, r->stream);
  MR_D2H(profile_out, dprof.p, (size_t)n_users * CT_MAXF * 4, r->stream);
  MR_D2H(x_out, dx.p, (size_t)n_users * CT_ROW * 8, r->stream);
  MR_D2H(itn_out, ditn.p, (size_t)n_users * 4, r->stream);
  MR_D2H(istop_out, distop.p, (size_t)n_users * 4, r->stream);
  MR_HIP(hipStreamSynchronize(r->stream));
  return 0;
}

static int check_models(int n_users, const int* p, const int* profile) {
  MR_CHECK(n_users >= 0, "content: negative n_users");
  for (int u = 0; u < n_users; ++u) {
    MR_CHECK(p[u] >= 0 && p[u] <= CT_MAXF, "content: profile length must be in 0..25");
    const int* pr = profile + (int64_t)u * CT_MAXF;
    for (int j = 0; j < p[u]; ++j) {
      MR_CHECK(pr[j] >= 0, "content: profile ids must be >= 0");
      for (int q = 0; q < j; ++q)
        MR_CHECK(pr[q] != pr[j], "content: profile ids must be distinct");
    }
  }
  return 0;
}

// users per score / select launch: bounds the score scratch to ~1 GiB
static int64_t ct_user_chunk(const Content* r) {
  const int64_t per = std::max<int64_t>(r->n_cand, 1) * 8;
  return std::max<int64_t>(1, std::min<int64_t>(65535, (int64_t(1) << 30) / per));
}

struct ModelBufs {
  RkBuf<int> p, prof;
  RkBuf<double> x;
  int alloc(int64_t B) { return p.alloc(B) || prof.alloc(B * CT_MAXF) || x.alloc(B * CT_ROW); }
  int load(const int* ph, const int* profh, const double* xh, int64_t u0, int64_t nb,
           hipStream_t s) {
    MR_H2D(p.p, ph + u0, (size_t)nb * 4, s);
    MR_H2D(prof.p, profh + u0 * CT_MAXF, (size_t)nb * CT_MAXF * 4, s);
    MR_H2D(x.p, xh + u0 * CT_ROW, (size_t)nb * CT_ROW * 8, s);
    return 0;
  }
};

static int content_scores(Content* r, int n_users, const int* p, const int* profile,
                          const double* x, double* out) {
  if (check_models(n_users, p, profile)) return -1;
  ct_reset_ms(r);
  if (n_users == 0 || r->n_cand == 0) return 0;
  const int64_t B = std::min<int64_t>(ct_user_chunk(r), n_users);
  ModelBufs m;
  RkBuf<double> S;
  if (m.alloc(B) || S.alloc(B * r->n_cand)) return -1;
  for (int64_t u0 = 0; u0 < n_users; u0 += B) {
    const int nb = (int)std::min<int64_t>(B, n_users - u0);
    if (m.load(p, profile, x, u0, nb, r->stream)) return -1;
    const dim3 grid((r->n_cand + 255) / 256, nb);
    if (ct_timed(r, CT_SCORE, [&]() {
          content_score_kernel<false><<<grid, 256, 0, r->stream>>>(
              r->n_cand, m.p.p, m.prof.p, m.x.p, r->foff, r->fid, r->fval, r->med, S.p, nullptr,
              nullptr);
        }))
      return -1;
    MR_D2H(out + u0 * r->n_cand, S.p, (size_t)nb * r->n_cand * 8, r->stream);
  }
  MR_HIP(hipStreamSynchronize(r->stream));
  return 0;
}

static int content_top_n(Content* r, int n_users, const int* p, const int* profile,
                         const double* x, const long long* excl_off, const int* excl_cand, int N,
                         int* out_mid, double* out_score, int* out_count) {
  if (check_models(n_users, p, profile)) return -1;
  MR_CHECK(N >= 1 && N <= kRecMaxResults, "content: num_results must be in 1..1024");
  ct_reset_ms(r);
  if (n_users == 0) return 0;
  if (r->n_cand == 0) {
    std::fill(out_count, out_count + n_users, 0);
    return 0;
  }
  ModelBufs m;
  if (m.alloc(std::min<int64_t>(ct_user_chunk(r), n_users))) return -1;
  return top_n_chunked(
      "content", r->stream, r->n_cand, r->mid, n_users, ct_user_chunk(r), excl_off, excl_cand, N,
      out_mid, out_score, out_count,
      [&](int64_t u0, int nb, uint64_t* keys, unsigned long long* kmin,
          unsigned long long* kmax) -> int {
        if (m.load(p, profile, x, u0, nb, r->stream)) return -1;
        const dim3 grid((r->n_cand + 255) / 256, nb);
        return ct_timed(r, CT_SCORE, [&]() {
          launch_rec_range_init(r->stream, nb, kmin, kmax);
          content_score_kernel<true><<<grid, 256, 0, r->stream>>>(
              r->n_cand, m.p.p, m.prof.p, m.x.p, r->foff, r->fid, r->fval, r->med, keys, kmin,
              kmax);
        });
      },
      [&](int stage, auto&& launch) {
        return ct_timed(r, stage == TOPN_EXCL ? CT_EXCL : CT_SELECT, launch);
      });
}

static int content_evaluate(Content* r, int n_test, const int* p, const int* profile,
                            const double* x, const long long* off, const int* cand,
                            const double* actual, double* agreement, long long* n_agree,
                            long long* n_dis, double* pred, double* sse, long long* n_pred) {
  if (check_models(n_test, p, profile)) return -1;
  ct_reset_ms(r);
  if (n_test == 0) return 0;
  MR_CHECK(rk_offsets_ok(off, n_test), "content: test offsets must start at 0 and not decrease");
  const int64_t nnz = off[n_test];
  for (int64_t i = 0; i < nnz; ++i)
    MR_CHECK(cand[i] >= -1 && cand[i] < r->n_cand, "content: evaluation candidate out of range");
  ModelBufs m;
  RkBuf<int> dcand;
  RkBuf<int64_t> doff;
  RkBuf<double> dact, dpred, dagr, dsse;
  RkBuf<long long> dag, ddis, dnp;
  if (m.alloc(n_test) || m.load(p, profile, x, 0, n_test, r->stream) ||
      doff.upload(reinterpret_cast<const int64_t*>(off), n_test + 1, r->stream) ||
      dcand.upload(cand, nnz, r->stream) || dact.upload(actual, nnz, r->stream) ||
      dpred.alloc(nnz) || dagr.alloc(n_test) || dsse.alloc(n_test) || dag.alloc(n_test) ||
      ddis.alloc(n_test) || dnp.alloc(n_test))
    return -1;
  if (ct_timed(r, CT_EVAL, [&]() {
        content_pred_kernel<<<n_test, 256, 0, r->stream>>>(m.p.p, m.prof.p, m.x.p, doff.p,
                                                           dcand.p, r->foff, r->fid, r->fval,
                                                           r->med, dpred.p);
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
// C ABI (include/mr_content.h)
// ---------------------------------------------------------------------------
struct mr_content {
  mr::Content r;
};

extern "C" {

mr_content* mr_content_create(int device, int n_cand, const int* cand_mid,
                              const double* cand_med, const long long* feat_off,
                              const int* feat_id, const double* feat_val) {
  mr_content* ctx = nullptr;
  const int rc = mr::rk_guard([&]() -> int {
    ctx = new mr_content();
    return mr::content_init(&ctx->r, device, n_cand, cand_mid, cand_med, feat_off, feat_id,
                            feat_val);
  });
  if (rc) {
    delete ctx;
    return nullptr;
  }
  return ctx;
}

void mr_content_destroy(mr_content* ctx) { delete ctx; }

int mr_content_num_candidates(const mr_content* ctx) { return ctx ? ctx->r.n_cand : -1; }

int mr_content_fit(mr_content* ctx, int n_users, const long long* off, const int* cand,
                   const double* ratings, double atol, double btol, double conlim, int iter_lim,
                   const int* iter_lim_each, int* p_out, int* profile_out, double* x_out,
                   int* itn_out, int* istop_out) {
  if (!ctx) return -1;
  return mr::rk_guard([&]() {
    return mr::content_fit(&ctx->r, n_users, off, cand, ratings, atol, btol, conlim, iter_lim,
                           iter_lim_each, p_out, profile_out, x_out, itn_out, istop_out);
  });
}

int mr_content_scores(mr_content* ctx, int n_users, const int* p, const int* profile,
                      const double* x, double* out) {
  if (!ctx) return -1;
  return mr::rk_guard(
      [&]() { return mr::content_scores(&ctx->r, n_users, p, profile, x, out); });
}

int mr_content_top_n(mr_content* ctx, int n_users, const int* p, const int* profile,
                     const double* x, const long long* excl_off, const int* excl_cand,
                     int num_results, int* out_mid, double* out_score, int* out_count) {
  if (!ctx) return -1;
  return mr::rk_guard([&]() {
    return mr::content_top_n(&ctx->r, n_users, p, profile, x, excl_off, excl_cand, num_results,
                             out_mid, out_score, out_count);
  });
}

int mr_content_evaluate(mr_content* ctx, int n_test, const int* p, const int* profile,
                        const double* x, const long long* off, const int* cand,
                        const double* actual, double* agreement, long long* n_agree,
                        long long* n_disagree, double* pred, double* sse, long long* n_pred) {
  if (!ctx) return -1;
  return mr::rk_guard([&]() {
    return mr::content_evaluate(&ctx->r, n_test, p, profile, x, off, cand, actual, agreement,
                                n_agree, n_disagree, pred, sse, n_pred);
  });
}

int mr_content_last_kernel_ms(const mr_content* ctx, double* ms6) {
  if (!ctx || !ms6) return -1;
  for (int i = 0; i < mr::CT_N; ++i) ms6[i] = ctx->r.ms[i];
  return 0;
}

}  // extern "C"
