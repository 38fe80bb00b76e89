// Pieces of the factor consumers (serving.hip) that the content models
// (content.hip) run on as well: the exact fp64 helpers, the order-preserving
// score key, and launchers of the exclusion, top-N select and ranking
// agreement kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "mr_internal.h"

namespace mr {

// The reference's Python evaluates u*v and s + (u*v) as two correctly rounded
// operations.  hipcc contracts a*b + c into v_fmac_f64 by default, which
// changes the last bit, so contraction is switched off for these two.
__device__ __forceinline__ double mul_rn(double a, double b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ double add_rn(double a, double b) {
#pragma clang fp contract(off)
  return a + b;
}

// Order-preserving 64-bit key of a score (larger score -> larger key); -0.0
// and +0.0 map to the same key as they compare equal in Python's sort.  Key 0
// is reserved for "excluded" (it would be a negative NaN with every bit set).
__device__ __forceinline__ uint64_t score_key(double s) {
  if (s == 0.0) s = 0.0;
  const uint64_t b = (uint64_t)__double_as_longlong(s);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double key_score(uint64_t key) {
  const uint64_t b = (key >> 63) ? (key & 0x7fffffffffffffffull) : ~key;
  return __longlong_as_double((long long)b);
}

constexpr int kRecMaxResults = 1024;   // largest num_results of the select

// rec_range_init_kernel: kmin[u] = ~0, kmax[u] = 0 for n users.
void launch_rec_range_init(hipStream_t s, int n, unsigned long long* kmin,
                           unsigned long long* kmax);
// rec_exclude_kernel: keys[u * ld + cand[i]] = 0 for i in off[u] .. off[u+1]-1.
void launch_rec_exclude(hipStream_t s, int n_users, uint64_t* keys, int64_t ld,
                        const int64_t* off, const int* cand);
// rec_select_kernel: per user the first N (<= kRecMaxResults) candidates by
// (key, movie id) descending; out_count[u] = -1 on an internal overflow.
void launch_rec_select(hipStream_t s, int n_users, const uint64_t* keys, int64_t ld, int n_cand,
                       const int* mid, const unsigned long long* kmin,
                       const unsigned long long* kmax, int N, int* out_mid, double* out_score,
                       int* out_count);
// rec_eval_kernel on given predictions (NaN: none): agreement, pair counts,
// squared error and number of predictions per user (the last two optional).
void launch_rank_agreement(hipStream_t s, int n_users, const int64_t* off, const double* actual,
                           double* pred, double* agreement, long long* n_agree,
                           long long* n_dis, double* sse, long long* n_pred);

// Host side of a top-N call, shared by mr_rec_top_n and mr_content_top_n: the
// users go through the device in chunks of B (the caller's bound on the key
// scratch and on the score grid).  Per chunk [u0, u0 + nb): score(u0, nb,
// keys, kmin, kmax) uploads the chunk's models and fills keys[nb][n_cand] and
// the key ranges (its launches timed by the caller); then the chunk's
// exclusions, rebased to the chunk, the select, and the read-back into rows
// u0 .. of the outputs.  timed(stage, launch) runs `launch` under the caller's
// timer for that stage.  `who` prefixes the error messages.
enum { TOPN_EXCL = 0, TOPN_SELECT = 1 };

template <class Score, class Timed>
int top_n_chunked(const char* who, hipStream_t s, int n_cand, const int* d_mid, int n_users,
                  int64_t B, const long long* excl_off, const int* excl_cand, int N, int* out_mid,
                  double* out_score, int* out_count, Score&& score, Timed&& timed) {
  const std::string w(who);
  B = std::min<int64_t>(B, n_users);
  RkBuf<uint64_t> S;
  RkBuf<unsigned long long> kmin, kmax;
  RkBuf<double> osc;
  RkBuf<int> omid, ocnt, ecand;
  RkBuf<int64_t> eoff;
  if (S.alloc(B * n_cand) || osc.alloc(B * N) || omid.alloc(B * N) || ocnt.alloc(B) ||
      eoff.alloc(B + 1) || kmin.alloc(B) || kmax.alloc(B))
    return -1;
  if (excl_off) {
    MR_CHECK(rk_offsets_ok(excl_off, n_users),
             w + ": exclusion offsets must start at 0 and not decrease");
    int64_t max_ex = 0;
    for (int64_t u0 = 0; u0 < n_users; u0 += B) {
      const int64_t nb = std::min<int64_t>(B, n_users - u0);
      max_ex = std::max<int64_t>(max_ex, excl_off[u0 + nb] - excl_off[u0]);
    }
    for (int64_t i = 0; i < excl_off[n_users]; ++i)
      MR_CHECK(excl_cand[i] >= 0 && excl_cand[i] < n_cand,
               w + ": excluded candidate out of range");
    if (ecand.alloc(max_ex)) return -1;
  }
  std::vector<int64_t> loc;
  for (int64_t u0 = 0; u0 < n_users; u0 += B) {
    const int nb = (int)std::min<int64_t>(B, n_users - u0);
    if (score(u0, nb, S.p, kmin.p, kmax.p)) return -1;
    if (excl_off) {
      loc.assign(nb + 1, 0);
      for (int i = 0; i <= nb; ++i) loc[i] = excl_off[u0 + i] - excl_off[u0];
      MR_H2D(eoff.p, loc.data(), (size_t)(nb + 1) * 8, s);
      if (loc[nb] > 0) MR_H2D(ecand.p, excl_cand + excl_off[u0], (size_t)loc[nb] * 4, s);
      if (timed(TOPN_EXCL, [&]() { launch_rec_exclude(s, nb, S.p, n_cand, eoff.p, ecand.p); }))
        return -1;
    }
    if (timed(TOPN_SELECT, [&]() {
          launch_rec_select(s, nb, S.p, n_cand, n_cand, d_mid, kmin.p, kmax.p, N, omid.p, osc.p,
                            ocnt.p);
        }))
      return -1;
    MR_D2H(out_mid + u0 * N, omid.p, (size_t)nb * N * 4, s);
    MR_D2H(out_score + u0 * N, osc.p, (size_t)nb * N * 8, s);
    MR_D2H(out_count + u0, ocnt.p, (size_t)nb * 4, s);
  }
  MR_HIP(hipStreamSynchronize(s));
  for (int u = 0; u < n_users; ++u)
    MR_CHECK(out_count[u] >= 0, w + ": top-N candidate buffer overflow (internal)");
  return 0;
}

}  // namespace mr
