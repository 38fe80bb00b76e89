// Explanations on MI355X (gfx950): per-rating contributions to the score of a
// target row, phi[t][j] = coef_j (A_t^T G^-1 A_j), from the Cholesky factor the
// fold-in leaves in LDS.  C ABI: include/mr_explain.h.  DESIGN.md
// "Explanations".
#include "../../include/mr_explain.h"
#include "foldin_device.h"

namespace mr {

// ---------------------------------------------------------------------------
// K-EX: one entity per 256-thread workgroup.
//
// Phase 1 is K-FI1's (foldin.hip): fi_build and fi_cholesky_solve of
// foldin_device.h on the same LDS layout, so x and status are mr_fold_in's
// bits.  It leaves L in the lower triangle of G[K][K+1] and x in column K.
//
// Phase 2 reads LDS only and has no block barrier (one precedes it, after the
// reciprocals of the diagonal of L go to the idle row stage).  The block is
// 16 groups of EX_G = 16 lanes, one target per group, so EX_TILE = 16 targets
// are solved at a time (4 per wave, in lockstep: the four groups of a wave
// read the same entries of L, which the LDS broadcasts).  A group keeps its right-hand side
// in registers, coordinate i in lane i % 16, slot i / 16 (EX_NS = 9 slots for
// K <= 129), and runs both substitutions column by column: the pivot
// coordinate is broadcast with one shuffle, every lane updates its own slots.
//   score = A_t . x           (index order, every lane the same sum)
//   L y = A_t, L^T z = y      (z replaces y in the registers; the pivot step
//                             multiplies by 1 / L_pp)
//   phi_j = coef_j (z . A_j)  A_j re-gathered from T (L2), 16 lanes a row, the
//                             partial sums combined by a 4-step butterfly
// EX_JB list entries are in flight per group.  phi goes out 16 entries (128 B)
// at a time.  The top list is kept in registers as well, entry i in lane
// i % 16, slot i / 16 (EX_TS = 4 slots for top <= 64), sorted descending; a
// new value enters behind every kept value >= it, which is the stable order
// by position since positions arrive ascending.
// ---------------------------------------------------------------------------
constexpr int EX_G = 16, EX_TILE = 256 / EX_G, EX_NS = (kMaxK + 1 + EX_G - 1) / EX_G;
constexpr int EX_TS = 4, EX_JB = 4;
constexpr int kExplainMaxTop = EX_G * EX_TS;
static_assert(EX_G == 16 && EX_TILE == 16, "the group shuffles below are written for 16 lanes");

__device__ __forceinline__ double ex_group_sum(double v) {   // all 16 lanes get the same bits
  v += __shfl_xor(v, 8, EX_G);
  v += __shfl_xor(v, 4, EX_G);
  v += __shfl_xor(v, 2, EX_G);
  v += __shfl_xor(v, 1, EX_G);
  return v;
}

__device__ __forceinline__ int ex_group_sum(int v) {
  v += __shfl_xor(v, 8, EX_G);
  v += __shfl_xor(v, 4, EX_G);
  v += __shfl_xor(v, 2, EX_G);
  v += __shfl_xor(v, 1, EX_G);
  return v;
}

__global__ __launch_bounds__(256) void explain_kernel(
    int e0, int k, int icpt, int implicit, int rows_per_stage, double alpha, double reg,
    int weighted, const int64_t* __restrict__ off, const int* __restrict__ idx,
    const double* __restrict__ r, const double* __restrict__ T, const double* __restrict__ roff,
    const double* __restrict__ S, const int64_t* __restrict__ toff,
    const int* __restrict__ tidx, int top, const int64_t* __restrict__ poff, int64_t phi_base,
    double* __restrict__ X, int* __restrict__ status, double* __restrict__ score,
    double* __restrict__ phi, int* __restrict__ top_pos, double* __restrict__ top_val,
    int* __restrict__ top_cnt) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  __shared__ int s_bad;
  const int K = k + icpt;
  const int W = K + 1;
  const int e = e0 + blockIdx.x, tid = threadIdx.x;
  const int64_t b = off[e];
  const int M = (int)(off[e + 1] - b);
  const int64_t tb = toff[e];
  const int Q = (int)(toff[e + 1] - tb);
  double* G = lds;           // [K][W]
  double* As = lds + K * W;  // [rows_per_stage][K + 2]
  bool solved = false;       // block-uniform
  if (M > 0) {
    const double lam = weighted ? reg * (double)M : reg;
    fi_build(k, icpt, implicit, rows_per_stage, alpha, lam, b, M, idx, r, T, roff, S, G, As);
    solved = !fi_cholesky_solve(K, G, &s_bad);
  }
  for (int i = tid; i < K; i += 256) X[(int64_t)e * K + i] = solved ? G[i * W + K] : 0.0;
  if (tid == 0) status[e] = (M == 0 || solved) ? 1 : 0;
  // 1 / L_pp once per entity, in the row stage the build is done with: the
  // substitutions below multiply where they would divide 2 K times a target
  double* dinv = As;
  if (solved)
    for (int i = tid; i < K; i += 256) dinv[i] = 1.0 / G[i * W + i];
  __syncthreads();

  const int g = tid / EX_G, gl = tid % EX_G;
  double* phie = phi ? phi + (poff[e] - phi_base) : nullptr;
  for (int q0 = 0; q0 < Q; q0 += EX_TILE) {
    const int q = q0 + g;
    if (q >= Q) break;   // the whole group; nothing below crosses groups
    const int64_t tq = tb + q;
    if (!solved) {   // an empty list, or a pivot that was not positive: all zero
      if (gl == 0) {
        score[tq] = 0.0;
        top_cnt[tq] = 0;
      }
      for (int i = gl; i < top; i += EX_G) {
        top_pos[tq * top + i] = -1;
        top_val[tq * top + i] = 0.0;
      }
      if (phie)
        for (int j = gl; j < M; j += EX_G) phie[(int64_t)q * M + j] = 0.0;
      continue;
    }
    const int t = tidx[tq];
    double y[EX_NS];
#pragma unroll
    for (int s = 0; s < EX_NS; ++s) {
      const int i = s * EX_G + gl;
      y[s] = i < k ? T[(int64_t)t * k + i] : (i < K ? 1.0 : 0.0);
    }
    // score = A_t . x in index order
    double sc = 0.0;
#pragma unroll
    for (int s = 0; s < EX_NS; ++s) {
      if (s * EX_G >= K) break;
      const int pend = min(EX_G, K - s * EX_G);
      for (int l = 0; l < pend; ++l)
        sc = fma(__shfl(y[s], l, EX_G), G[(s * EX_G + l) * W + K], sc);
    }
    // L y = A_t
#pragma unroll
    for (int s = 0; s < EX_NS; ++s) {
      if (s * EX_G >= K) break;
      const int pend = min(EX_G, K - s * EX_G);
      for (int l = 0; l < pend; ++l) {
        const int p = s * EX_G + l;
        const double yp = __shfl(y[s], l, EX_G) * dinv[p];
        if (gl == l) y[s] = yp;
#pragma unroll
        for (int s2 = s; s2 < EX_NS; ++s2) {
          if (s2 * EX_G >= K) break;
          const int i = s2 * EX_G + gl;
          if (i > p && i < K) y[s2] -= G[i * W + p] * yp;
        }
      }
    }
    // L^T z = y
#pragma unroll
    for (int s = EX_NS - 1; s >= 0; --s) {
      if (s * EX_G >= K) continue;
      for (int l = min(EX_G, K - s * EX_G) - 1; l >= 0; --l) {
        const int p = s * EX_G + l;
        const double zp = __shfl(y[s], l, EX_G) * dinv[p];
        if (gl == l) y[s] = zp;
#pragma unroll
        for (int s2 = 0; s2 <= s; ++s2) {
          const int i = s2 * EX_G + gl;
          if (i < p) y[s2] -= G[p * W + i] * zp;
        }
      }
    }
    // phi_j = coef_j (z . A_j), and the top list
    int n = 0, tp[EX_TS];
    double tv[EX_TS], thr = 0.0, keep = 0.0;
#pragma unroll
    for (int s = 0; s < EX_TS; ++s) {
      tv[s] = 0.0;
      tp[s] = -1;
    }
    for (int j0 = 0; j0 < M; j0 += EX_JB) {
      int id[EX_JB];
      double d[EX_JB];
#pragma unroll
      for (int u = 0; u < EX_JB; ++u) id[u] = idx[b + min(j0 + u, M - 1)];
#pragma unroll
      for (int u = 0; u < EX_JB; ++u) {
        d[u] = 0.0;
#pragma unroll
        for (int s = 0; s < EX_NS; ++s) {
          if (s * EX_G >= K) break;
          const int i = s * EX_G + gl;
          const double a = i < k ? T[(int64_t)id[u] * k + i] : (i < K ? 1.0 : 0.0);
          d[u] = fma(y[s], a, d[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < EX_JB; ++u) d[u] = ex_group_sum(d[u]);
#pragma unroll
      for (int u = 0; u < EX_JB; ++u) {
        const int j = j0 + u;
        if (j >= M) break;
        const double rj = r[b + j];
        const double coef = implicit ? 1.0 + fi_mul(alpha, rj) : (roff ? rj - roff[id[u]] : rj);
        const double ph = fi_mul(coef, d[u]);
        if (phie) {
          if (gl == (j & (EX_G - 1))) keep = ph;
          if ((j & (EX_G - 1)) == EX_G - 1 || j == M - 1) {
            const int jj = (j & ~(EX_G - 1)) + gl;
            if (jj <= j) phie[(int64_t)q * M + jj] = keep;
          }
        }
        if (top > 0 && (n < top || ph > thr)) {   // group-uniform
          int c = 0;
#pragma unroll
          for (int s = 0; s < EX_TS; ++s)
            if (s * EX_G + gl < n && tv[s] >= ph) ++c;
          const int ins = ex_group_sum(c);   // kept entries that stay ahead of the new one
          double pv[EX_TS];
          int pp[EX_TS];
#pragma unroll
          for (int s = 0; s < EX_TS; ++s) {   // entry i - 1: the lane below, or lane 15 of slot s - 1
            pv[s] = __shfl_up(tv[s], 1, EX_G);
            pp[s] = __shfl_up(tp[s], 1, EX_G);
            if (s > 0) {
              const double wv = __shfl(tv[s - 1], EX_G - 1, EX_G);
              const int wp = __shfl(tp[s - 1], EX_G - 1, EX_G);
              if (gl == 0) {
                pv[s] = wv;
                pp[s] = wp;
              }
            }
          }
#pragma unroll
          for (int s = 0; s < EX_TS; ++s) {
            const int i = s * EX_G + gl;
            if (i > ins && i <= n) {
              tv[s] = pv[s];
              tp[s] = pp[s];
            } else if (i == ins) {
              tv[s] = ph;
              tp[s] = j;
            }
          }
          n = min(n + 1, top);
          if (n == top) {   // the smallest kept value, entry top - 1
            double last = 0.0;
#pragma unroll
            for (int s = 0; s < EX_TS; ++s)
              if (s == (top - 1) / EX_G) last = tv[s];
            thr = __shfl(last, (top - 1) % EX_G, EX_G);
          }
        }
      }
    }
#pragma unroll
    for (int s = 0; s < EX_TS; ++s) {
      const int i = s * EX_G + gl;
      if (i < top) {
        top_pos[tq * top + i] = i < n ? tp[s] : -1;
        top_val[tq * top + i] = i < n ? tv[s] : 0.0;
      }
    }
    if (gl == 0) {
      score[tq] = sc;
      top_cnt[tq] = n;
    }
  }
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
constexpr int64_t kPhiChunk = (int64_t(1) << 28) / 8;   // doubles of one device phi buffer

static int explain(int device, int k, int n_rows, const double* T, const double* row_offset,
                   int mode, int intercept, double alpha, double reg, int reg_mode, int n_ent,
                   const long long* off, const int* idx, const double* r, const long long* toff,
                   const int* tidx, int top, double* x_out, int* status, double* score,
                   const long long* poff, double* phi, int* top_pos, double* top_val,
                   int* top_cnt) {
  if (fi_validate("explain", k, n_rows, T, row_offset, mode, intercept, alpha, reg, reg_mode,
                  n_ent, off, idx, r))
    return -1;
  MR_CHECK(top >= 0 && top <= kExplainMaxTop, "explain: top must be in 0..64");
  MR_CHECK(phi || top_pos || top_val || top_cnt,
           "explain: phi or one of the top outputs must be requested");
  if (n_ent == 0) return 0;
  MR_CHECK(toff, "explain: toff is required");
  MR_CHECK(rk_offsets_ok(toff, n_ent), "explain: target offsets must start at 0 and not decrease");
  const int64_t nt = toff[n_ent];
  MR_CHECK(nt == 0 || tidx, "explain: tidx is required");
  for (int64_t i = 0; i < nt; ++i)
    MR_CHECK(tidx[i] >= 0 && tidx[i] < n_rows, "explain: target id out of range");
  for (int e = 0; e < n_ent; ++e)
    MR_CHECK(toff[e + 1] - toff[e] < 0x7fffffff, "explain: too many targets for one entity");
  if (phi) {
    MR_CHECK(poff, "explain: poff is required with phi");
    MR_CHECK(poff[0] == 0, "explain: poff must be the running sum of Q * M from 0");
    for (int e = 0; e < n_ent; ++e) {
      const int64_t qm = (int64_t)(toff[e + 1] - toff[e]) * (int64_t)(off[e + 1] - off[e]);
      MR_CHECK(qm <= kPhiChunk, "explain: the phi block of one entity exceeds 256 MiB");
      MR_CHECK(poff[e + 1] - poff[e] == qm,
               "explain: poff must be the running sum of Q * M from 0");
    }
  }

  const bool implicit = mode == MR_FOLD_IMPLICIT;
  const int K = k + intercept;
  const int64_t nnz = off[n_ent];
  int rows;
  size_t gbytes, stage;
  fi_solve_lds(K, &rows, &gbytes, &stage);
  MR_CHECK(rows > 0, "explain: k too large");
  const size_t lds = gbytes + stage;
  RkScope sc;
  if (sc.init(device)) return -1;
  hipStream_t s = sc.s;
  const int kk = k * k;
  RkBuf<double> dT, dro, dpart, dS, dr, dX, dscore, dphi, dtv;
  RkBuf<int64_t> doff, dtoff, dpoff;
  RkBuf<int> didx, dtidx, dstat, dtp, dtc;
  if (dT.upload(T, (int64_t)n_rows * k, s) ||
      doff.upload(reinterpret_cast<const int64_t*>(off), (int64_t)n_ent + 1, s) ||
      dtoff.upload(reinterpret_cast<const int64_t*>(toff), (int64_t)n_ent + 1, s) ||
      didx.upload(idx, nnz, s) || dr.upload(r, nnz, s) || dtidx.upload(tidx, nt, s) ||
      dX.alloc((int64_t)n_ent * K) || dstat.alloc(n_ent) || dscore.alloc(nt) ||
      dtp.alloc(nt * top) || dtv.alloc(nt * top) || dtc.alloc(nt))
    return -1;
  if (row_offset && dro.upload(row_offset, n_rows, s)) return -1;
  if (phi && (dpoff.upload(reinterpret_cast<const int64_t*>(poff), (int64_t)n_ent + 1, s) ||
              dphi.alloc(std::min<int64_t>(poff[n_ent], kPhiChunk))))
    return -1;
  if (implicit) {
    const int nblk = (int)std::max<int64_t>(1, std::min<int64_t>(((int64_t)n_rows + 63) / 64, 256));
    if (dpart.alloc((int64_t)nblk * kk) || dS.alloc(kk)) return -1;
    fold_yty_partial_kernel<<<dim3(nblk, (kk + 256 * FY_NQ - 1) / (256 * FY_NQ)), 256, 0, s>>>(
        dT.p, n_rows, k, dpart.p);
    fold_yty_combine_kernel<<<(kk + 255) / 256, 256, 0, s>>>(dpart.p, nblk, kk, dS.p);
    MR_HIP(hipGetLastError());
  }
  const int weighted = reg_mode == MR_REG_WEIGHTED ? 1 : 0;
  if (lds > 64 * 1024)
    MR_HIP(hipFuncSetAttribute((const void*)explain_kernel,
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  // entities per launch: their phi blocks together fit the device buffer
  for (int e0 = 0; e0 < n_ent;) {
    int e1 = n_ent;
    if (phi) {
      e1 = e0 + 1;
      while (e1 < n_ent && poff[e1 + 1] - poff[e0] <= kPhiChunk) ++e1;
    }
    explain_kernel<<<e1 - e0, 256, lds, s>>>(
        e0, k, intercept, implicit ? 1 : 0, rows, alpha, reg, weighted, doff.p, didx.p, dr.p,
        dT.p, dro.p, dS.p, dtoff.p, dtidx.p, top, dpoff.p, phi ? (int64_t)poff[e0] : 0, dX.p,
        dstat.p, dscore.p, phi ? dphi.p : nullptr, dtp.p, dtv.p, dtc.p);
    MR_HIP(hipGetLastError());
    if (phi && poff[e1] > poff[e0])
      MR_D2H(phi + poff[e0], dphi.p, (size_t)(poff[e1] - poff[e0]) * 8, s);
    e0 = e1;
  }
  if (x_out) MR_D2H(x_out, dX.p, (size_t)n_ent * K * 8, s);
  if (status) MR_D2H(status, dstat.p, (size_t)n_ent * 4, s);
  if (score && nt) MR_D2H(score, dscore.p, (size_t)nt * 8, s);
  if (top_pos && nt * top) MR_D2H(top_pos, dtp.p, (size_t)(nt * top) * 4, s);
  if (top_val && nt * top) MR_D2H(top_val, dtv.p, (size_t)(nt * top) * 8, s);
  if (top_cnt && nt) MR_D2H(top_cnt, dtc.p, (size_t)nt * 4, s);
  MR_HIP(hipStreamSynchronize(s));
  return 0;
}

}  // namespace mr

extern "C" {

int mr_explain(int device, int k, int n_rows, const double* T, const double* row_offset, int mode,
               int intercept, double alpha, double reg, int reg_mode, int n_ent,
               const long long* off, const int* idx, const double* r, const long long* toff,
               const int* tidx, int top, double* x_out, int* status, double* score,
               const long long* poff, double* phi, int* top_pos, double* top_val, int* top_cnt) {
  return mr::rk_guard([&]() {
    return mr::explain(device, k, n_rows, T, row_offset, mode, intercept, alpha, reg, reg_mode,
                       n_ent, off, idx, r, toff, tidx, top, x_out, status, score, poff, phi,
                       top_pos, top_val, top_cnt);
  });
}

}  // extern "C"
