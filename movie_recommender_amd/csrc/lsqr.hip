// General sparse LSQR on the GPU (include/mr_lsqr.h): scipy.sparse.linalg.lsqr
// as the reference's SciPy ALS calls it (python/100k_data/ratings_als.py:
// 347-448), as a device-resident context.
//
// Per context: the structure of cgls.hip (SpStructure: A's rows ordered by
// first column, the explicit transpose, the CSR-stream row blocks of both)
// built ONCE on the entry indices, which leaves in place of the values the
// caller's index of every stored entry of A and of A^T; new values are then
// two gathers through these maps (no re-sort).  Per solve: the setup (u = b -
// A x0, v = A^T u, w = v) and three kernels per iteration (lsqr_device.h: KA,
// KT = csr_spmv_kernel<SPG_S, SPO_LSQR>, KX = lsqr_x_kernel here); the
// scalars live in the device LsqrState, every KX publishes (itn, istop, done)
// into a host-mapped seqlock ring, and the host keeps a few iterations
// enqueued ahead (the protocol of CgLs::solve).
//
// LSMR (mr_lsqr_solve_lsmr; lsmr_device.h) runs on the same context: the
// same KA / KT with the LSQR_LSMR bit, its own state, KX = lsmr_x_kernel on
// (h = w, hbar), the same host loop.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/mr_lsqr.h"
#include "engine.h"
#include "lsmr_device.h"
#include "lsqr_device.h"
#include "sp_structure.h"
#include "svds_device.h"

namespace mr {

namespace {

constexpr int kLsqrThreads = 256;

// KX: dk = (1/rho) w, x = x + t1 w, w = v + t2 w with v = vs vh (lsqr.py:
// 467-471), sum dk^2; in the setup w = v (:392-394).  The last workgroup
// applies lsqr_after_x.
__global__ __launch_bounds__(kLsqrThreads) void lsqr_x_kernel(
    LsqrState* st, int64_t n, double* __restrict__ x, double* __restrict__ w,
    const double* __restrict__ vh, double* __restrict__ partials, CgMirror* mirror, int seq) {
#pragma clang fp contract(off)
  if (st->done) return;
  __shared__ double sh[4];
  const bool setup = st->setup != 0;
  const double vs = st->vs, t1 = st->t1, t2 = st->t2, irho = st->irho;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const double v = vs * vh[i];
    if (setup) {
      w[i] = v;
    } else {
      const double wi = w[i];
      const double dk = irho * wi;
      x[i] = x[i] + t1 * wi;
      w[i] = v + t2 * wi;
      acc += dk * dk;
    }
  }
  const double tot = lsqr_block_sum(acc, sh);
  lsqr_last_block(st, partials, tot, sh,
                  [&](double total) { lsqr_after_x(st, total, mirror, seq); });
}

// LSMR's KX: hbar = hbar ch + h, x = x + cx hbar, h = h chh + v with v = vs vh
// (lsmr.py:365-369), sum x^2 on the new x (:413); in the setup h = v, hbar = 0
// (:268-269).  The last workgroup applies lsmr_after_x.
__global__ __launch_bounds__(kLsqrThreads) void lsmr_x_kernel(
    LsmrState* st, int64_t n, double* __restrict__ x, double* __restrict__ h,
    double* __restrict__ hbar, const double* __restrict__ vh, double* __restrict__ partials,
    CgMirror* mirror, int seq) {
#pragma clang fp contract(off)
  if (st->q.done) return;
  __shared__ double sh[4];
  const bool setup = st->q.setup != 0;
  const double vs = st->q.vs, ch = st->ch, cx = st->cx, chh = st->chh;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const double v = vs * vh[i];
    if (setup) {
      h[i] = v;
      hbar[i] = 0.0;
    } else {
      const double hi = h[i];
      const double hb = hbar[i] * ch + hi;
      hbar[i] = hb;
      const double xi = x[i] + cx * hb;
      x[i] = xi;
      h[i] = hi * chh + v;
      acc += xi * xi;
    }
  }
  const double tot = lsqr_block_sum(acc, sh);
  lsqr_last_block(&st->q, partials, tot, sh,
                  [&](double total) { lsmr_after_x(st, total, mirror, seq); });
}

// bnorm = sqrt(sum b_i^2) (lsqr.py:374) when x0 is given.
__global__ __launch_bounds__(kLsqrThreads) void lsqr_bnorm_kernel(
    LsqrState* st, int64_t n, const double* __restrict__ b, double* __restrict__ partials) {
#pragma clang fp contract(off)
  __shared__ double sh[4];
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    acc += b[i] * b[i];
  const double tot = lsqr_block_sum(acc, sh);
  lsqr_last_block(st, partials, tot, sh, [&](double total) { st->bnorm = sqrt(total); });
}

// *out = sum |b_i - t_i| over a fixed grid, the partials in index order.
__global__ __launch_bounds__(kLsqrThreads) void lsqr_l1_kernel(
    LsqrState* st, int64_t n, const double* __restrict__ b, const double* __restrict__ t,
    double* __restrict__ partials, double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double sh[4];
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    acc += fabs(b[i] - t[i]);
  const double tot = lsqr_block_sum(acc, sh);
  lsqr_last_block(st, partials, tot, sh, [&](double total) { *out = total; });
}

// the structure was built on hv[j] = j: the values are the caller's indices
__global__ void lsqr_index_kernel(int64_t n, const double* __restrict__ v,
                                  int32_t* __restrict__ map) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n;
       t += (int64_t)gridDim.x * blockDim.x)
    map[t] = (int32_t)v[t];
}

// dst[t] = tab ? (idx[map[t]] < 0 ? 1.0 : tab[idx[map[t]]]) : src[map[t]]
__global__ void lsqr_values_kernel(int64_t n, const int32_t* __restrict__ map,
                                   const double* __restrict__ src,
                                   const int32_t* __restrict__ idx,
                                   const double* __restrict__ tab, double* __restrict__ dst) {
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n;
       t += (int64_t)gridDim.x * blockDim.x) {
    const int32_t m = map[t];
    if (tab) {
      const int32_t i = idx[m];
      dst[t] = i < 0 ? 1.0 : tab[i];
    } else {
      dst[t] = src[m];
    }
  }
}

unsigned grid_of(int64_t n, int cap) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(cap, (n + kLsqrThreads - 1) / kLsqrThreads));
}

}  // namespace

struct Lsqr : LaunchTimer {
  int device = 0;
  hipStream_t s = nullptr;
  SpStructure sp;
  int64_t rows = 0, cols = 0, nnz = 0;
  std::vector<void*> owned;
  int32_t *map_a = nullptr, *map_t = nullptr;   // the caller's index of A's / A^T's entries
  int32_t* vidx = nullptr;                      // mr_lsqr_set_value_map
  bool have_vidx = false;
  int32_t vidx_max = -1;
  double *vin = nullptr, *tab = nullptr;        // uploaded values / table
  int64_t tab_cap = 0;
  double *b_in = nullptr, *uh = nullptr, *vh = nullptr, *w = nullptr, *x = nullptr,
         *partials = nullptr, *scal = nullptr;
  LsqrState* st = nullptr;
  LsqrState* h_st = nullptr;   // pinned: the initial state up, the final state down
  // LSMR: allocated by the context's first LSMR solve
  double* hbar = nullptr;
  LsmrState *lm = nullptr, *h_lm = nullptr;
  LsqrState* cur = nullptr;    // the running solve's state (st, or lm's head)
  int cur_mode = 0;            // 0, or LSQR_LSMR
  SvdsWork* svds = nullptr;    // the truncated SVD's buffers (svds.hip), by its first call
  CgMirror *h_mirror = nullptr, *d_mirror = nullptr;
  int seq = 0;
  bool ptr_loads = false;
  mr_lsqr_stats stats{};

  ~Lsqr() {
    if (!s) return;
    (void)hipSetDevice(device);
    (void)hipStreamSynchronize(s);
    svds_release(svds);
    for (void* q_ : owned) (void)hipFree(q_);
    if (tab) (void)hipFree(tab);
    if (h_st) (void)hipHostFree(h_st);
    if (h_lm) (void)hipHostFree(h_lm);
    if (h_mirror) (void)hipHostFree(h_mirror);
    destroy_events();
    (void)hipStreamDestroy(s);
  }

  int toc() { return LaunchTimer::toc(s); }

  int init(int dev, int rows_, int cols_, const int* hrp, const int* hci, const double* hv) {
    if (SpStructure::check(rows_, cols_, hrp, hci, hv)) return -1;
    device = dev;
    MR_HIP(hipSetDevice(device));
    MR_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    MR_HIP(hipHostMalloc((void**)&h_st, sizeof(LsqrState), hipHostMallocDefault));
    MR_HIP(hipHostMalloc((void**)&h_mirror, kMirrorSlots * sizeof(CgMirror),
                         hipHostMallocMapped | hipHostMallocCoherent));
    memset(h_mirror, 0, kMirrorSlots * sizeof(CgMirror));
    MR_HIP(hipHostGetDevicePointer((void**)&d_mirror, h_mirror, 0));
    {
      // the structure on the entry indices (exact in fp64: nnz < 2^31)
      std::vector<double> iota((size_t)hrp[rows_]);
      for (size_t j = 0; j < iota.size(); ++j) iota[j] = (double)j;
      if (sp.build(s, rows_, cols_, hrp, hci, iota.data(), owned)) return -1;
    }
    rows = sp.rows;
    cols = sp.cols;
    nnz = sp.nnz;
    if (sp_dmalloc(&map_a, nnz, owned) || sp_dmalloc(&map_t, nnz, owned) ||
        sp_dmalloc(&vidx, nnz, owned) || sp_dmalloc(&vin, nnz, owned) ||
        sp_dmalloc(&b_in, rows, owned) || sp_dmalloc(&uh, rows, owned) ||
        sp_dmalloc(&vh, cols, owned) || sp_dmalloc(&w, cols, owned) ||
        sp_dmalloc(&x, cols, owned) || sp_dmalloc(&partials, kMaxParts, owned) ||
        sp_dmalloc(&scal, 1, owned) || sp_dmalloc(&st, 1, owned))
      return -1;
    MR_HIP(hipMemsetAsync(st, 0, sizeof(LsqrState), s));
    if (nnz) {
      lsqr_index_kernel<<<grid_of(nnz, 4096), kLsqrThreads, 0, s>>>(nnz, sp.v, map_a);
      lsqr_index_kernel<<<grid_of(nnz, 4096), kLsqrThreads, 0, s>>>(nnz, sp.tv, map_t);
      MR_HIP(hipGetLastError());
    }
    // the padding entries of v / tv are read (never used) by the row-block loads
    MR_HIP(hipMemsetAsync(sp.v + nnz, 0, kSpPad * sizeof(double), s));
    MR_HIP(hipMemsetAsync(sp.tv + nnz, 0, kSpPad * sizeof(double), s));
    stats.rows = rows;
    stats.cols = cols;
    stats.nnz = nnz;
    stats.blocks_a = sp.n_blk_a;
    stats.blocks_at = sp.n_blk_t;
    stats.block_max_nnz = kSpTile;
    stats.block_max_rows = kSpMaxRows;
    return set_values(hv);
  }

  int apply(const double* src, const double* table) {
    if (nnz) {
      lsqr_values_kernel<<<grid_of(nnz, 4096), kLsqrThreads, 0, s>>>(nnz, map_a, src, vidx, table,
                                                                    sp.v);
      lsqr_values_kernel<<<grid_of(nnz, 4096), kLsqrThreads, 0, s>>>(nnz, map_t, src, vidx, table,
                                                                    sp.tv);
      MR_HIP(hipGetLastError());
    }
    MR_HIP(hipStreamSynchronize(s));
    return 0;
  }

  int set_values(const double* hv) {
    MR_CHECK(hv || nnz == 0, "null values");
    MR_HIP(hipSetDevice(device));
    if (nnz) MR_H2D(vin, hv, nnz * 8, s);
    return apply(vin, nullptr);
  }

  int set_value_map(const int* index) {
    MR_CHECK(index || nnz == 0, "null value map");
    int32_t mx = -1;
    for (int64_t j = 0; j < nnz; ++j) {
      MR_CHECK(index[j] >= -1, "value map entries are -1 or a table index");
      mx = std::max(mx, index[j]);
    }
    MR_HIP(hipSetDevice(device));
    if (nnz) MR_H2D(vidx, index, nnz * 4, s);
    MR_HIP(hipStreamSynchronize(s));
    vidx_max = mx;
    have_vidx = true;
    return 0;
  }

  int set_values_from_table(const double* table, long long len) {
    MR_CHECK(have_vidx, "no value map set");
    MR_CHECK(len >= 0 && (table || len == 0), "null table");
    MR_CHECK((long long)vidx_max < len, "value map index beyond the table");
    MR_HIP(hipSetDevice(device));
    if (len > tab_cap) {
      MR_HIP(hipStreamSynchronize(s));
      if (tab) (void)hipFree(tab);
      tab = nullptr;
      tab_cap = 0;
      MR_HIP(hipMalloc((void**)&tab, (size_t)len * 8));
      tab_cap = len;
    }
    if (len) MR_H2D(tab, table, len * 8, s);
    // an all -1 map reads no table entry; the kernel still needs a non-null pointer
    return apply(nullptr, tab ? tab : scal);
  }

  // rows == 0 or cols == 0: no product to take (lsqr.py:373-408 by hand)
  int solve_empty(const double* hb, const double* hx0, double* hx, mr_lsqr_result* out) {
    double ss = 0.0;
    for (int64_t i = 0; i < rows; ++i) ss += hb[i] * hb[i];
    for (int64_t j = 0; j < cols; ++j) hx[j] = hx0 ? hx0[j] : 0.0;
    const double beta = std::sqrt(ss);
    *out = mr_lsqr_result{0, 0, beta, beta, 0.0, 0.0, 0.0, 0.0};
    stats.last_iterations = 0;
    return 0;
  }

  int pass(int lmode) {
    const bool kt = (lmode & LSQR_KT) != 0;
    lmode |= cur_mode;
    if (kt)
      return launch_csr_spmv_lsqr(s, cur, lmode, sp.n_blk_t, sp.blk_t, sp.tp, sp.ti, sp.tv, uh, rows,
                                  vh, partials, kMaxParts, ptr_loads);
    return launch_csr_spmv_lsqr(s, cur, lmode, sp.n_blk_a, sp.blk_a, sp.rp, sp.ci, sp.v,
                                (lmode & LSQR_NEG) ? x : vh, cols, uh, partials, kMaxParts,
                                ptr_loads);
  }

  int kx(int sq) {
    if (cur_mode & LSQR_LSMR)
      MR_LAUNCH(lsmr_x_kernel, dim3(grid_of(cols, kUpdParts)), dim3(kLsqrThreads), 0, s, lm, cols,
                x, w, hbar, vh, partials, d_mirror, sq);
    else
      MR_LAUNCH(lsqr_x_kernel, dim3(grid_of(cols, kUpdParts)), dim3(kLsqrThreads), 0, s, st, cols,
                x, w, vh, partials, d_mirror, sq);
    MR_HIP(hipGetLastError());
    return 0;
  }

  int iteration(int it, int sq) {
    if (tic(MR_LSQR_K_A, it) || pass(0) || toc()) return -1;
    if (tic(MR_LSQR_K_AT, it) || pass(LSQR_KT) || toc()) return -1;
    if (tic(MR_LSQR_K_X, it) || kx(sq) || toc()) return -1;
    return 0;
  }

  // rows == 0 or cols == 0 (lsmr.py:237-303 by hand): alpha = 0, so normar == 0
  // returns x0 at once with normA = 0, condA = 1
  int solve_empty_lsmr(const double* hb, const double* hx0, double* hx, mr_lsmr_result* out) {
    double ss = 0.0;
    for (int64_t i = 0; i < rows; ++i) ss += hb[i] * hb[i];
    for (int64_t j = 0; j < cols; ++j) hx[j] = hx0 ? hx0[j] : 0.0;
    *out = mr_lsmr_result{0, 0, std::sqrt(ss), 0.0, 0.0, 1.0, 0.0};
    stats.last_iterations = 0;
    return 0;
  }

  int solve(const double* hb, const double* hx0, double damp, double atol, double btol,
            double conlim, int iter_lim, double* hx, mr_lsqr_result* out) {
    MR_CHECK(out, "null result");
    MR_CHECK((hb || rows == 0) && (hx || cols == 0), "null b or x");
    if (rows == 0 || cols == 0) return solve_empty(hb, hx0, hx, out);
    if (run(0, hb, hx0, damp, atol, btol, conlim, iter_lim, hx)) return -1;
    *out = mr_lsqr_result{h_st->istop, h_st->itn,   h_st->r1norm, h_st->r2norm,
                          h_st->anorm, h_st->acond, h_st->arnorm, h_st->xnorm};
    return 0;
  }

  int solve_lsmr(const double* hb, const double* hx0, double damp, double atol, double btol,
                 double conlim, int maxiter, double* hx, mr_lsmr_result* out) {
    MR_CHECK(out, "null result");
    MR_CHECK((hb || rows == 0) && (hx || cols == 0), "null b or x");
    if (rows == 0 || cols == 0) return solve_empty_lsmr(hb, hx0, hx, out);
    MR_HIP(hipSetDevice(device));
    if (!h_lm) MR_HIP(hipHostMalloc((void**)&h_lm, sizeof(LsmrState), hipHostMallocDefault));
    if ((!hbar && sp_dmalloc(&hbar, cols, owned)) || (!lm && sp_dmalloc(&lm, 1, owned))) return -1;
    if (run(LSQR_LSMR, hb, hx0, damp, atol, btol, conlim, maxiter, hx)) return -1;
    if (h_lm->zero_x) std::fill(hx, hx + cols, 0.0);   // x[()] = 0 (lsmr.py:305-307)
    *out = mr_lsmr_result{h_lm->q.istop, h_lm->q.itn, h_lm->normr, h_lm->normar,
                          h_lm->normA,   h_lm->condA, h_lm->normx};
    return 0;
  }

  // One solve of either kind (mode: 0, or LSQR_LSMR); the final state is left
  // in h_st / h_lm, x in hx.
  int run(int mode, const double* hb, const double* hx0, double damp, double atol, double btol,
          double conlim, int iter_lim, double* hx) {
    const bool lsmr = (mode & LSQR_LSMR) != 0;
    cur_mode = mode;
    cur = lsmr ? &lm->q : st;
    LsqrState* h_cur = lsmr ? &h_lm->q : h_st;
    const size_t st_bytes = lsmr ? sizeof(LsmrState) : sizeof(LsqrState);
    MR_HIP(hipSetDevice(device));
    MR_H2D(b_in, hb, rows * 8, s);
    if (launch_gather_f64(s, rows, sp.perm, b_in, uh)) return -1;   // u = b in the rows' order
    if (hx0) MR_H2D(x, hx0, cols * 8, s);
    else MR_HIP(hipMemsetAsync(x, 0, cols * 8, s));
    MR_HIP(hipMemsetAsync(vh, 0, cols * 8, s));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (timing) {
      if (ev(&e0) || ev(&e1)) return -1;
      MR_HIP(hipEventRecord(e0, s));
    }
    memset((void*)h_cur, 0, st_bytes);
    h_cur->alfa = 1.0;   // the setup's KA: u = 1 * (1 * b) - A x0
    h_cur->us = 1.0;
    h_cur->vs = 1.0;
    h_cur->cs2 = -1.0;
    h_cur->damp = damp;
    h_cur->dampsq = damp * damp;
    h_cur->atol = atol;
    h_cur->btol = btol;
    h_cur->ctol = conlim > 0.0 ? 1.0 / conlim : 0.0;
    h_cur->iter_lim = iter_lim;
    h_cur->setup = 1;
    h_cur->bnorm_is_beta = hx0 ? 0 : 1;
    MR_HIP(hipMemcpyAsync(cur, h_cur, st_bytes, hipMemcpyHostToDevice, s));
    if (tic(MR_LSQR_K_SETUP, -1)) return -1;
    if (hx0) {
      MR_LAUNCH(lsqr_bnorm_kernel, dim3(grid_of(rows, kUpdParts)), dim3(kLsqrThreads), 0, s, cur,
                rows, b_in, partials);
      MR_HIP(hipGetLastError());
    }
    if (pass(LSQR_NEG) || pass(LSQR_KT) || kx(++seq) || toc()) return -1;
    const int seq_init = seq;
    // Enqueue up to kAhead iterations beyond the last known state; an
    // iteration enqueued after the solve stopped exits at once (done flag).
    constexpr int kAhead = 3;
    std::vector<int> seq_of;
    int launched = 0;
    auto enqueue_to = [&](int n) -> int {
      while (launched < std::min(n, iter_lim)) {
        seq_of.push_back(++seq);
        if (iteration(launched, seq_of.back())) return -1;
        ++launched;
      }
      return 0;
    };
    if (enqueue_to(kAhead)) return -1;
    CgMirror ms{};
    if (wait_published(h_mirror, seq_init, s, 300.0, &ms)) return -1;
    int known = -1;   // ms = the state after iteration `known` (-1: the setup)
    while (!ms.done) {
      if (enqueue_to(known + 1 + kAhead)) return -1;
      MR_CHECK(known + 1 < (int)seq_of.size(), "LSQR did not terminate");
      if (wait_published(h_mirror, seq_of[known + 1], s, 300.0, &ms)) return -1;
      ++known;
    }
    if (timing) MR_HIP(hipEventRecord(e1, s));
    MR_HIP(hipMemcpyAsync(h_cur, cur, st_bytes, hipMemcpyDeviceToHost, s));
    MR_D2H(hx, x, cols * 8, s);
    MR_HIP(hipStreamSynchronize(s));
    if (timing) {
      float ms_ = 0.f;
      MR_HIP(hipEventElapsedTime(&ms_, e0, e1));
      stats.solve_ms += ms_;
      pool.push_back(e0);
      pool.push_back(e1);
      for (auto& tm : pend) {
        if (tm.it < h_cur->itn) {   // setup (-1) and the iterations that did work
          MR_HIP(hipEventElapsedTime(&ms_, tm.a, tm.b));
          stats.kernel_ms[tm.cls] += ms_;
          stats.kernel_launches[tm.cls] += 1;
        }
        pool.push_back(tm.a);
        pool.push_back(tm.b);
      }
      pend.clear();
    }
    stats.last_iterations = h_cur->itn;
    stats.iterations_total += h_cur->itn;
    return 0;
  }

  int residual_l1(const double* hb, const double* hx, double* out) {
    MR_CHECK(out && (hb || rows == 0) && (hx || cols == 0), "null argument");
    if (rows == 0) {
      *out = 0.0;
      return 0;
    }
    if (cols == 0) {
      double a = 0.0;
      for (int64_t i = 0; i < rows; ++i) a += std::fabs(hb[i]);
      *out = a;
      return 0;
    }
    MR_HIP(hipSetDevice(device));
    MR_H2D(b_in, hb, rows * 8, s);
    if (launch_gather_f64(s, rows, sp.perm, b_in, uh)) return -1;
    MR_H2D(x, hx, cols * 8, s);
    // b_in = A x (rows in the device's order), then sum |b - A x|
    if (launch_csr_spmv(s, SPG_X, SPO_STORE, nullptr, sp.n_blk_a, sp.blk_a, sp.rp, sp.ci, sp.v, x,
                        nullptr, cols, b_in, nullptr, nullptr, 0, nullptr, kMaxParts, nullptr,
                        ptr_loads))
      return -1;
    lsqr_l1_kernel<<<grid_of(rows, kUpdParts), kLsqrThreads, 0, s>>>(st, rows, uh, b_in, partials,
                                                                   scal);
    MR_HIP(hipGetLastError());
    MR_D2H(out, scal, 8, s);
    return 0;
  }
};

}  // namespace mr

struct mr_lsqr {
  mr::Lsqr c;
};

mr::SvdsHost mr::svds_host_of(mr_lsqr* ctx) {
  mr::Lsqr& c = ctx->c;
  return mr::SvdsHost{c.device, c.s, &c.sp, &c, c.ptr_loads, &c.stats, &c.svds};
}

namespace {
template <typename F>
int lsqr_guarded(F&& f) {
  int rc = -1;
  try {
    rc = f();
  } catch (const std::bad_alloc&) {
    mr::set_error("host out of memory");
  } catch (...) {
    mr::set_error("unexpected C++ exception");
  }
  // a launch helper that failed inside a timed interval left its event pair
  // in this thread's launch-timing slot: drop it
  mr::t_launch = mr::LaunchTiming{};
  return rc;
}
}  // namespace

extern "C" {

mr_lsqr* mr_lsqr_create(int device, int rows, int cols, const int* row_indices,
                        const int* col_indices, const double* values) {
  mr_lsqr* h = nullptr;
  const int rc = lsqr_guarded([&]() -> int {
    h = new mr_lsqr();
    return h->c.init(device, rows, cols, row_indices, col_indices, values);
  });
  if (rc) {
    delete h;
    return nullptr;
  }
  return h;
}

void mr_lsqr_destroy(mr_lsqr* ctx) { delete ctx; }

int mr_lsqr_set_values(mr_lsqr* ctx, const double* values) {
  MR_CHECK(ctx, "null context");
  return lsqr_guarded([&]() { return ctx->c.set_values(values); });
}

int mr_lsqr_set_value_map(mr_lsqr* ctx, const int* index) {
  MR_CHECK(ctx, "null context");
  return lsqr_guarded([&]() { return ctx->c.set_value_map(index); });
}

int mr_lsqr_set_values_from_table(mr_lsqr* ctx, const double* table, long long table_len) {
  MR_CHECK(ctx, "null context");
  return lsqr_guarded([&]() { return ctx->c.set_values_from_table(table, table_len); });
}

int mr_lsqr_solve(mr_lsqr* ctx, const double* b, const double* x0_or_null, double damp,
                  double atol, double btol, double conlim, int iter_lim, double* x_out,
                  mr_lsqr_result* out) {
  MR_CHECK(ctx, "null context");
  return lsqr_guarded([&]() {
    return ctx->c.solve(b, x0_or_null, damp, atol, btol, conlim, iter_lim, x_out, out);
  });
}

int mr_lsqr_solve_lsmr(mr_lsqr* ctx, const double* b, const double* x0_or_null, double damp,
                       double atol, double btol, double conlim, int maxiter, double* x_out,
                       mr_lsmr_result* out) {
  MR_CHECK(ctx, "null context");
  return lsqr_guarded([&]() {
    return ctx->c.solve_lsmr(b, x0_or_null, damp, atol, btol, conlim, maxiter, x_out, out);
  });
}

int mr_lsqr_residual_l1(mr_lsqr* ctx, const double* b, const double* x, double* out) {
  MR_CHECK(ctx, "null context");
  return lsqr_guarded([&]() { return ctx->c.residual_l1(b, x, out); });
}

int mr_lsqr_set_timing(mr_lsqr* ctx, int enable) {
  MR_CHECK(ctx, "null context");
  ctx->c.timing = enable != 0;
  return 0;
}

int mr_lsqr_set_gather_path(mr_lsqr* ctx, int mode) {
  MR_CHECK(ctx, "null context");
  MR_CHECK(mode == 0 || mode == 1, "gather path: 0 (by size) or 1 (pointer loads)");
  ctx->c.ptr_loads = mode == 1;
  return 0;
}

int mr_lsqr_get_stats(mr_lsqr* ctx, mr_lsqr_stats* out) {
  MR_CHECK(ctx && out, "null argument");
  *out = ctx->c.stats;
  return 0;
}

int mr_lsqr_reset_stats(mr_lsqr* ctx) {
  MR_CHECK(ctx, "null context");
  mr_lsqr_stats z{};
  const mr_lsqr_stats& k = ctx->c.stats;
  z.rows = k.rows;
  z.cols = k.cols;
  z.nnz = k.nnz;
  z.blocks_a = k.blocks_a;
  z.blocks_at = k.blocks_at;
  z.block_max_nnz = k.block_max_nnz;
  z.block_max_rows = k.block_max_rows;
  ctx->c.stats = z;
  return 0;
}

}  // extern "C"
