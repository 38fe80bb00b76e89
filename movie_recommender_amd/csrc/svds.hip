// Truncated sparse SVD on a resident LSQR context (include/mr_lsqr.h):
// thick-restart Golub-Kahan-Lanczos with full re-orthogonalisation, fp64.
//
// The right basis P (cols x (ncv + 1)) and the left basis Q (rows x ncv, in
// the structure's row order) are column-major on the device, so a Lanczos
// vector is the operand and the result of the context's CSR-stream SpMV
// (launch_csr_spmv, SPG_X / SPO_STORE) with no copy.  New here is everything
// that touches a basis:
//   basis_dot_kernel     partial sums of h = B^T w, one per column and workgroup
//   basis_hsum_kernel    h_c = its partials in workgroup order
//   basis_update_kernel  w -= B h, with the partial sums of |w|^2
//   basis_scale_kernel   |w|^2 from its partials, w *= 1 / |w|
//   basis_combine_kernel B_new = B Y for a small dense Y (restart, Ritz vectors)
// A workgroup of the dot / update kernels owns rows (pass p, workgroup b,
// thread t) -> ((p G + b) 256 + t) of a fixed grid G <= kBasisBlocks and keeps
// kBasisRows of them per thread in registers while the columns stream by
// (coalesced: a pass of a column is one contiguous run); beyond kBasisRows
// passes it takes a further chunk and adds to its own partials.  Every sum
// has a fixed order (thread, lanes by butterfly, waves in order, workgroups in
// index order), so the same inputs give the same bits.  One CGS pass reads
// (j + 1) n 8 bytes in the dot and as much in the update.
//
// The projected matrix, its Jacobi SVD, the restart rule and the random
// stream are host code (svds_host.h).
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/mr_lsqr.h"
#include "engine.h"
#include "svds_device.h"
#include "svds_host.h"

namespace mr {

namespace {

constexpr int kBasisThreads = 256;
constexpr int kBasisBlocks = 256;   // grid limit of the dot / update kernels
constexpr int kBasisRows = 8;       // rows a thread keeps in registers per chunk
constexpr int kDotCols = 4;         // columns reduced together by the dot kernel
constexpr int kCombTile = 16;       // output columns per thread of the combine
constexpr int kClsOrth = 100, kClsCombine = 101;   // LaunchTimer classes (0 / 1: K_A / K_AT)

unsigned basis_grid(int64_t n) {
  return (unsigned)std::max<int64_t>(
      1, std::min<int64_t>(kBasisBlocks, (n + kBasisThreads - 1) / kBasisThreads));
}

// part[c G + b] (+)= sum over workgroup b's rows of basis[c ld + row] w[row]
__global__ __launch_bounds__(kBasisThreads) void basis_dot_kernel(
    int64_t n, int64_t ld, int j, const double* __restrict__ basis, const double* __restrict__ w,
    double* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ double sh[2][kBasisThreads / 64][kDotCols];
  const int t = threadIdx.x, G = gridDim.x, b = blockIdx.x;
  const int64_t pass_rows = (int64_t)G * kBasisThreads;
  int grp = 0;
  bool first = true;
  for (int64_t r0 = (int64_t)b * kBasisThreads; r0 < n; r0 += kBasisRows * pass_rows) {
    int64_t row[kBasisRows];
    double wr[kBasisRows];
#pragma unroll
    for (int p = 0; p < kBasisRows; ++p) {
      row[p] = r0 + p * pass_rows + t;
      wr[p] = row[p] < n ? w[row[p]] : 0.0;
    }
    for (int c = 0; c < j; c += kDotCols, ++grp) {
      double acc[kDotCols];
#pragma unroll
      for (int u = 0; u < kDotCols; ++u) {
        acc[u] = 0.0;
        if (c + u < j) {
          const double* col = basis + (int64_t)(c + u) * ld;
#pragma unroll
          for (int p = 0; p < kBasisRows; ++p) {
            const double v = row[p] < n ? col[row[p]] : 0.0;
            acc[u] += v * wr[p];
          }
        }
      }
#pragma unroll
      for (int u = 0; u < kDotCols; ++u)
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) acc[u] += __shfl_xor(acc[u], m, 64);
      if ((t & 63) == 0) {
#pragma unroll
        for (int u = 0; u < kDotCols; ++u) sh[grp & 1][t >> 6][u] = acc[u];
      }
      // one barrier per group: sh is double-buffered, and a wave that writes
      // group g + 2 has passed the barrier of g + 1, behind the reads of g
      __syncthreads();
      if (t < kDotCols && c + t < j) {
        const double tot = ((sh[grp & 1][0][t] + sh[grp & 1][1][t]) + sh[grp & 1][2][t]) +
                           sh[grp & 1][3][t];
        double* dst = part + (int64_t)(c + t) * G + b;
        *dst = first ? tot : *dst + tot;
      }
    }
    first = false;
  }
}

// h[c] = sum_b part[c G + b] in workgroup order; hacc[c] = h[c], or += h[c]
__global__ __launch_bounds__(kBasisThreads) void basis_hsum_kernel(
    int j, int G, const double* __restrict__ part, double* __restrict__ h,
    double* __restrict__ hacc, int first) {
#pragma clang fp contract(off)
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= j) return;
  double s = 0.0;
  for (int b = 0; b < G; ++b) s += part[(int64_t)c * G + b];
  h[c] = s;
  hacc[c] = first ? s : hacc[c] + s;
}

// w[row] -= sum_c h[c] basis[c ld + row] (columns in order); npart[b] = the
// workgroup's sum of the new w^2.  j == 0 stores w as it was.
__global__ __launch_bounds__(kBasisThreads) void basis_update_kernel(
    int64_t n, int64_t ld, int j, const double* __restrict__ basis, const double* __restrict__ h,
    double* __restrict__ w, double* __restrict__ npart) {
#pragma clang fp contract(off)
  __shared__ double sh[kBasisThreads / 64];
  const int t = threadIdx.x, G = gridDim.x, b = blockIdx.x;
  const int64_t pass_rows = (int64_t)G * kBasisThreads;
  double ss = 0.0;
  for (int64_t r0 = (int64_t)b * kBasisThreads; r0 < n; r0 += kBasisRows * pass_rows) {
    int64_t row[kBasisRows];
    double wr[kBasisRows];
#pragma unroll
    for (int p = 0; p < kBasisRows; ++p) {
      row[p] = r0 + p * pass_rows + t;
      wr[p] = row[p] < n ? w[row[p]] : 0.0;
    }
#pragma unroll 4
    for (int c = 0; c < j; ++c) {
      const double hc = h[c];
      const double* col = basis + (int64_t)c * ld;
#pragma unroll
      for (int p = 0; p < kBasisRows; ++p) {
        const double v = row[p] < n ? col[row[p]] : 0.0;
        wr[p] = wr[p] - hc * v;
      }
    }
#pragma unroll
    for (int p = 0; p < kBasisRows; ++p)
      if (row[p] < n) {
        w[row[p]] = wr[p];
        ss += wr[p] * wr[p];
      }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) ss += __shfl_xor(ss, m, 64);
  if ((t & 63) == 0) sh[t >> 6] = ss;
  __syncthreads();
  if (t == 0) npart[b] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// tot = sum of npart[0..nparts) (nparts <= kBasisBlocks) in a fixed order,
// the same in every workgroup; scale: w *= 1 / sqrt(tot) (0 when tot == 0).
// Workgroup 0 stores tot.
__global__ __launch_bounds__(kBasisThreads) void basis_scale_kernel(
    int64_t n, int nparts, const double* __restrict__ npart, double* __restrict__ w, int scale,
    double* __restrict__ tot_out) {
#pragma clang fp contract(off)
  __shared__ double sh[kBasisThreads / 64];
  __shared__ double s_tot;
  const int t = threadIdx.x;
  double v = t < nparts ? npart[t] : 0.0;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  if ((t & 63) == 0) sh[t >> 6] = v;
  __syncthreads();
  if (t == 0) s_tot = ((sh[0] + sh[1]) + sh[2]) + sh[3];
  __syncthreads();
  const double tot = s_tot;
  if (blockIdx.x == 0 && t == 0) *tot_out = tot;
  if (!scale) return;
  const double f = tot > 0.0 ? 1.0 / sqrt(tot) : 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + t; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    w[i] = w[i] * f;
}

// out[c ldo + row] = sum_i basis[i ldb + row] Y[i r + c], i in order: a thread
// owns one row and kCombTile output columns; Y's entries are uniform loads.
__global__ __launch_bounds__(kBasisThreads) void basis_combine_kernel(
    int64_t n, int64_t ldb, int m, int r, const double* __restrict__ basis,
    const double* __restrict__ Y, int64_t ldo, double* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t row = (int64_t)blockIdx.x * kBasisThreads + threadIdx.x;
  const int c0 = blockIdx.y * kCombTile;
  const int nc = min(kCombTile, r - c0);
  if (row >= n) return;
  double acc[kCombTile];
#pragma unroll
  for (int u = 0; u < kCombTile; ++u) acc[u] = 0.0;
  if (nc == kCombTile) {
    for (int i = 0; i < m; ++i) {
      const double bv = basis[(int64_t)i * ldb + row];
      const double* y = Y + (int64_t)i * r + c0;
#pragma unroll
      for (int u = 0; u < kCombTile; ++u) acc[u] += bv * y[u];
    }
  } else {
    for (int i = 0; i < m; ++i) {
      const double bv = basis[(int64_t)i * ldb + row];
      const double* y = Y + (int64_t)i * r + c0;
#pragma unroll
      for (int u = 0; u < kCombTile; ++u)
        if (u < nc) acc[u] += bv * y[u];
    }
  }
#pragma unroll
  for (int u = 0; u < kCombTile; ++u)
    if (u < nc) out[(int64_t)(c0 + u) * ldo + row] = acc[u];
}

// Scratch of the orthogonalisation for bases of up to jcap columns.
struct OrthScratch {
  double *part = nullptr, *npart = nullptr, *h = nullptr, *hacc = nullptr, *tot = nullptr;
  int jcap = -1;
  void release() {
    for (double* p : {part, npart, h, hacc, tot})
      if (p) (void)hipFree(p);
    part = npart = h = hacc = tot = nullptr;
    jcap = -1;
  }
  int reserve(int j) {
    if (j <= jcap) return 0;
    release();
    const size_t jc = (size_t)std::max(j, 1);
    MR_HIP(hipMalloc((void**)&part, jc * kBasisBlocks * 8));
    MR_HIP(hipMalloc((void**)&npart, kBasisBlocks * 8));
    MR_HIP(hipMalloc((void**)&h, jc * 8));
    MR_HIP(hipMalloc((void**)&hacc, jc * 8));
    MR_HIP(hipMalloc((void**)&tot, 8));
    jcap = j;
    return 0;
  }
};

// CGS2 of w[n] against basis[:, :j] (column stride ld), then |w|; scale: w is
// normalised too.  hacc holds the sum of both passes' coefficients.
int launch_orth(hipStream_t s, const OrthScratch& sc, int64_t n, int64_t ld, int j,
                const double* basis, double* w, bool scale, double* norm_out) {
  const unsigned G = basis_grid(n);
  for (int pass = 0; pass < (j > 0 ? 2 : 0); ++pass) {
    MR_LAUNCH(basis_dot_kernel, dim3(G), dim3(kBasisThreads), 0, s, n, ld, j, basis,
              (const double*)w, sc.part);
    MR_LAUNCH(basis_hsum_kernel, dim3((j + kBasisThreads - 1) / kBasisThreads),
              dim3(kBasisThreads), 0, s, j, (int)G, (const double*)sc.part, sc.h, sc.hacc,
              pass == 0 ? 1 : 0);
    MR_LAUNCH(basis_update_kernel, dim3(G), dim3(kBasisThreads), 0, s, n, ld, j, basis,
              (const double*)sc.h, w, sc.npart);
  }
  if (j == 0)
    MR_LAUNCH(basis_update_kernel, dim3(G), dim3(kBasisThreads), 0, s, n, ld, 0, basis,
              (const double*)sc.h, w, sc.npart);
  const unsigned gs = scale ? (unsigned)std::max<int64_t>(
                                  1, std::min<int64_t>(1024, (n + kBasisThreads - 1) / kBasisThreads))
                            : 1u;
  MR_LAUNCH(basis_scale_kernel, dim3(gs), dim3(kBasisThreads), 0, s, n, (int)G,
            (const double*)sc.npart, w, scale ? 1 : 0, sc.tot);
  MR_HIP(hipGetLastError());
  double tot = 0.0;
  MR_D2H(&tot, sc.tot, 8, s);
  *norm_out = std::sqrt(tot);
  return 0;
}

int launch_combine(hipStream_t s, int64_t n, int64_t ldb, int m, int r, const double* basis,
                   const double* Yd, int64_t ldo, double* out) {
  if (n <= 0 || r <= 0) return 0;
  const dim3 grid((unsigned)((n + kBasisThreads - 1) / kBasisThreads),
                  (unsigned)((r + kCombTile - 1) / kCombTile));
  MR_LAUNCH(basis_combine_kernel, grid, dim3(kBasisThreads), 0, s, n, ldb, m, r, basis, Yd, ldo,
            out);
  MR_HIP(hipGetLastError());
  return 0;
}

int64_t pad8(int64_t n) { return (std::max<int64_t>(n, 1) + 7) & ~(int64_t)7; }

}  // namespace

struct SvdsWork {
  double *P = nullptr, *P2 = nullptr, *Q = nullptr, *Q2 = nullptr, *Yd = nullptr;
  int cap_ncv = 0;
  int64_t ldp = 0, ldq = 0;
  OrthScratch sc;
  std::vector<int32_t> perm;   // perm[i] = the caller's row of device row i
  std::vector<double> last_resid;
  mr_svds_stats stats{};

  void release_basis() {
    for (double* p : {P, P2, Q, Q2, Yd})
      if (p) (void)hipFree(p);
    P = P2 = Q = Q2 = Yd = nullptr;
    cap_ncv = 0;
  }
  int reserve(int64_t rows, int64_t cols, int ncv) {
    if (ncv <= cap_ncv) return 0;
    release_basis();
    ldp = pad8(cols);
    ldq = pad8(rows);
    const size_t c1 = (size_t)ncv + 1;
    MR_HIP(hipMalloc((void**)&P, (size_t)ldp * c1 * 8));
    MR_HIP(hipMalloc((void**)&P2, (size_t)ldp * c1 * 8));
    MR_HIP(hipMalloc((void**)&Q, (size_t)ldq * c1 * 8));
    MR_HIP(hipMalloc((void**)&Q2, (size_t)ldq * c1 * 8));
    MR_HIP(hipMalloc((void**)&Yd, c1 * c1 * 8));
    if (sc.reserve(ncv + 1)) return -1;
    cap_ncv = ncv;
    return 0;
  }
};

void svds_release(SvdsWork* w) {
  if (!w) return;
  w->release_basis();
  w->sc.release();
  delete w;
}

namespace {

struct Svds {
  SvdsHost H;
  SvdsWork& W;
  int64_t M, N;
  hipStream_t s;
  long long spmv = 0;

  Svds(const SvdsHost& h, SvdsWork& w) : H(h), W(w), M(h.sp->rows), N(h.sp->cols), s(h.s) {}

  double* pcol(int j) { return W.P + (int64_t)j * W.ldp; }
  double* qcol(int j) { return W.Q + (int64_t)j * W.ldq; }
  int tic(int cls) { return H.timer->tic(cls, 0); }
  int toc() { return H.timer->toc(s); }

  // q_j = A p_j, or p_{j+1} = A^T q_j
  int product(bool transposed, int j) {
    const SpStructure& sp = *H.sp;
    ++spmv;
    if (transposed) {
      if (sp.nnz == 0 || sp.n_blk_t <= 0) {
        MR_HIP(hipMemsetAsync(pcol(j + 1), 0, (size_t)N * 8, s));
        return 0;
      }
      if (tic(MR_LSQR_K_AT) ||
          launch_csr_spmv(s, SPG_X, SPO_STORE, nullptr, sp.n_blk_t, sp.blk_t, sp.tp, sp.ti, sp.tv,
                          qcol(j), nullptr, M, pcol(j + 1), nullptr, nullptr, 0, nullptr,
                          kMaxParts, nullptr, H.ptr_loads) ||
          toc())
        return -1;
      return 0;
    }
    if (sp.nnz == 0 || sp.n_blk_a <= 0) {
      MR_HIP(hipMemsetAsync(qcol(j), 0, (size_t)M * 8, s));
      return 0;
    }
    if (tic(MR_LSQR_K_A) ||
        launch_csr_spmv(s, SPG_X, SPO_STORE, nullptr, sp.n_blk_a, sp.blk_a, sp.rp, sp.ci, sp.v,
                        pcol(j), nullptr, N, qcol(j), nullptr, nullptr, 0, nullptr, kMaxParts,
                        nullptr, H.ptr_loads) ||
        toc())
      return -1;
    return 0;
  }

  // CGS2 of column j against columns 0..j-1 of a basis, normalised in place
  int orth(bool right, int j, double* norm) {
    const int64_t n = right ? N : M, ld = right ? W.ldp : W.ldq;
    double* basis = right ? W.P : W.Q;
    if (tic(kClsOrth) ||
        launch_orth(s, W.sc, n, ld, j, basis, basis + (int64_t)j * ld, true, norm) || toc())
      return -1;
    W.stats.orth_bytes += (j > 0 ? 4 : 1) * (long long)(j + 1) * n * 8;
    return 0;
  }

  // a breakdown's replacement for column j: a fresh random vector made
  // orthonormal to the basis; a zero vector when the space is exhausted
  int replace(bool right, int j, SvdsRng& rng, std::vector<double>& tmp) {
    const int64_t n = right ? N : M, ld = right ? W.ldp : W.ldq;
    double* col = (right ? W.P : W.Q) + (int64_t)j * ld;
    if (j >= n) {
      MR_HIP(hipMemsetAsync(col, 0, (size_t)n * 8, s));
      return 0;
    }
    tmp.resize((size_t)n);
    for (int tries = 0; tries < 4; ++tries) {
      rng.fill(tmp.data(), n);
      MR_H2D(col, tmp.data(), n * 8, s);
      double nrm = 0.0;
      if (orth(right, j, &nrm)) return -1;
      if (nrm > 0.0) return 0;
    }
    set_error("svds: no replacement vector after a breakdown");
    return -1;
  }

  // dst[:, :r] = src[:, :m] Y[:, :r] with Y the leading columns of a row-major ncv x ncv matrix
  int combine(bool right, int m, int r, const double* Yfull, int ncv, double* dst,
              std::vector<double>& tmp) {
    const int64_t n = right ? N : M, ld = right ? W.ldp : W.ldq;
    tmp.resize((size_t)m * r);
    for (int i = 0; i < m; ++i)
      for (int c = 0; c < r; ++c) tmp[(size_t)i * r + c] = Yfull[(size_t)i * ncv + c];
    MR_H2D(W.Yd, tmp.data(), (size_t)m * r * 8, s);
    if (tic(kClsCombine) || launch_combine(s, n, ld, m, r, right ? W.P : W.Q, W.Yd, ld, dst) ||
        toc())
      return -1;
    return 0;
  }

  int run(int k, int ncv, double tol, int maxiter, const double* v0, unsigned long long seed,
          int want_vectors, double* s_out, double* U_out, double* Vt_out, mr_svds_result* out) {
    const int mn = (int)std::min(M, N);
    SvdsRng rng(seed);
    std::vector<double> tmp, B((size_t)ncv * ncv, 0.0), X((size_t)ncv * ncv), Y((size_t)ncv * ncv),
        sig(ncv);
    double nrm = 0.0;
    if (v0) {
      MR_H2D(pcol(0), v0, N * 8, s);
    } else {
      tmp.resize((size_t)N);
      rng.fill(tmp.data(), N);
      MR_H2D(pcol(0), tmp.data(), N * 8, s);
    }
    if (orth(true, 0, &nrm)) return -1;
    MR_CHECK(nrm > 0.0 && std::isfinite(nrm), "svds: v0 has no finite, non-zero norm");
    SvdsSweep sw;
    int l = 0, restarts = 0;
    int vrows = ncv;   // rows of Y: P's columns behind the right Ritz vectors
    double bmax = 0.0, beta_last = 0.0;
    for (;;) {
      for (int j = l; j < ncv; ++j) {
        double alpha = 0.0, beta = 0.0;
        if (product(false, j) || orth(false, j, &alpha)) return -1;
        MR_CHECK(std::isfinite(alpha), "svds: a Lanczos vector is not finite");
        if (alpha == 0.0 || alpha <= mn * kSvdsEps * std::max(sw.sigma1, bmax)) {
          alpha = 0.0;
          if (replace(false, j, rng, tmp)) return -1;
        }
        B[(size_t)j * ncv + j] = alpha;
        bmax = std::max(bmax, alpha);
        if (product(true, j) || orth(true, j + 1, &beta)) return -1;
        MR_CHECK(std::isfinite(beta), "svds: a Lanczos vector is not finite");
        // j + 1 == N: p_0 .. p_j span everything, z is rounding alone
        if (j + 1 >= N || beta == 0.0 || beta <= mn * kSvdsEps * std::max(sw.sigma1, bmax)) {
          beta = 0.0;
          if (replace(true, j + 1, rng, tmp)) return -1;
        }
        if (j + 1 < ncv) B[(size_t)j * ncv + j + 1] = beta;
        else beta_last = beta;
        bmax = std::max(bmax, beta);
        W.stats.steps += 1;
      }
      if (ncv == M && M < N && beta_last != 0.0) {
        // Q spans everything: A = Q [B | beta e] P_{ncv+1}^T, whose SVD is A's
        Y.assign((size_t)(ncv + 1) * ncv, 0.0);
        svds_jacobi_augmented(ncv, B.data(), beta_last, X.data(), sig.data(), Y.data());
        svds_judge(ncv, sig.data(), X.data(), 0.0, tol, sw);
        vrows = ncv + 1;
        break;
      }
      svds_jacobi(ncv, B.data(), X.data(), sig.data(), Y.data());
      svds_judge(ncv, sig.data(), X.data(), beta_last, tol, sw);
      // ncv == mn: the sweep above was the whole factorisation
      if (sw.nconv >= k || ncv == mn || restarts >= maxiter) break;
      const int keep = svds_keep(k, ncv, sw.nconv);
      if (combine(true, ncv, keep, Y.data(), ncv, W.P2, tmp)) return -1;
      MR_HIP(hipMemcpyAsync(W.P2 + (int64_t)keep * W.ldp, pcol(ncv), (size_t)N * 8,
                            hipMemcpyDeviceToDevice, s));
      if (combine(false, ncv, keep, X.data(), ncv, W.Q2, tmp)) return -1;
      std::swap(W.P, W.P2);
      std::swap(W.Q, W.Q2);
      svds_restart_b(ncv, keep, sig.data(), X.data(), beta_last, B.data());
      l = keep;
      ++restarts;
    }
    W.last_resid.assign(sw.resid.begin(), sw.resid.begin() + k);
    double max_res = 0.0;
    for (int i = 0; i < k; ++i) {
      s_out[i] = sig[i];
      max_res = std::max(max_res, sw.resid[i]);
    }
    if (want_vectors) {
      if (combine(true, vrows, k, Y.data(), ncv, W.P2, tmp)) return -1;
      for (int c = 0; c < k; ++c)
        MR_D2H(Vt_out + (size_t)c * N, W.P2 + (int64_t)c * W.ldp, N * 8, s);
      if (combine(false, ncv, k, X.data(), ncv, W.Q2, tmp)) return -1;
      tmp.resize((size_t)M);
      for (int c = 0; c < k; ++c) {
        MR_D2H(tmp.data(), W.Q2 + (int64_t)c * W.ldq, M * 8, s);
        for (int64_t i = 0; i < M; ++i) U_out[(size_t)W.perm[i] * k + c] = tmp[i];
      }
    }
    MR_HIP(hipStreamSynchronize(s));
    *out = mr_svds_result{sw.nconv >= k ? 1 : 0, restarts, std::min(sw.nconv, k), spmv, sw.sigma1,
                          max_res};
    return 0;
  }
};

// the timed intervals of one call into the statistics; the events back to the pool
void drain_timer(const SvdsHost& H, SvdsWork* W, bool ok) {
  LaunchTimer& T = *H.timer;
  for (auto& tm : T.pend) {
    float ms = 0.f;
    if (ok && hipEventElapsedTime(&ms, tm.a, tm.b) == hipSuccess) {
      if (tm.cls == kClsOrth || tm.cls == kClsCombine) {
        const int c = tm.cls == kClsOrth ? MR_SVDS_K_ORTH : MR_SVDS_K_COMBINE;
        if (W) {
          W->stats.kernel_ms[c] += ms;
          W->stats.kernel_launches[c] += 1;
        }
      } else if (tm.cls >= 0 && tm.cls < MR_LSQR_K_COUNT) {
        H.lstats->kernel_ms[tm.cls] += ms;
        H.lstats->kernel_launches[tm.cls] += 1;
      }
    }
    T.pool.push_back(tm.a);
    T.pool.push_back(tm.b);
  }
  T.pend.clear();
  t_launch = LaunchTiming{};
}

template <typename F>
int svds_guarded(F&& f) {
  int rc = -1;
  try {
    rc = f();
  } catch (const std::bad_alloc&) {
    set_error("host out of memory");
  } catch (...) {
    set_error("unexpected C++ exception");
  }
  t_launch = LaunchTiming{};
  return rc;
}

int svds_entry(mr_lsqr* ctx, int k, int ncv, double tol, int maxiter, const double* v0,
               unsigned long long seed, int want_vectors, double* s_out, double* U_out,
               double* Vt_out, mr_svds_result* out) {
  MR_CHECK(ctx && out && s_out, "svds: null argument");
  const SvdsHost H = svds_host_of(ctx);
  const int64_t M = H.sp->rows, N = H.sp->cols;
  const int64_t mn = std::min(M, N);
  MR_CHECK(k >= 1 && k <= mn, "svds: k must be in 1..min(rows, cols)");
  if (ncv == 0) ncv = svds_default_ncv(k, (int)mn);
  MR_CHECK((ncv > k && ncv <= mn) || (ncv == k && k == mn),
           "svds: ncv must satisfy k < ncv <= min(rows, cols)");
  MR_CHECK(tol >= 0.0 && std::isfinite(tol), "svds: tol must be finite and >= 0");
  MR_CHECK(maxiter >= 0, "svds: maxiter must be >= 0");
  if (maxiter == 0) maxiter = (int)std::min<int64_t>(10 * mn, 2147483647);
  MR_CHECK(!want_vectors || (U_out && Vt_out), "svds: null U_out or Vt_out");
  if (v0) {
    bool any = false;
    for (int64_t i = 0; i < N; ++i) {
      MR_CHECK(std::isfinite(v0[i]), "svds: v0 must be finite");
      any = any || v0[i] != 0.0;
    }
    MR_CHECK(any, "svds: v0 must not be zero");
  }
  MR_HIP(hipSetDevice(H.device));
  if (!*H.work) *H.work = new SvdsWork();
  SvdsWork& W = **H.work;
  if (W.reserve(M, N, ncv)) return -1;
  if ((int64_t)W.perm.size() != M) {
    W.perm.resize((size_t)M);
    MR_D2H(W.perm.data(), H.sp->perm, M * 4, H.s);
  }
  const auto t0 = std::chrono::steady_clock::now();
  Svds run(H, W);
  const int rc = run.run(k, ncv, tol, maxiter, v0, seed, want_vectors, s_out, U_out, Vt_out, out);
  if (rc) (void)hipStreamSynchronize(H.s);
  drain_timer(H, &W, rc == 0);
  W.stats.solve_ms +=
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return rc;
}

struct DevBuf {
  std::vector<void*> p;
  ~DevBuf() {
    for (void* q : p) (void)hipFree(q);
  }
  int get(double** out, size_t doubles) {
    *out = nullptr;
    MR_HIP(hipMalloc((void**)out, std::max<size_t>(doubles, 1) * 8));
    p.push_back(*out);
    return 0;
  }
};

}  // namespace

}  // namespace mr

extern "C" {

int mr_lsqr_svds(mr_lsqr* ctx, int k, int ncv, double tol, int maxiter,
                 const double* v0_or_null, unsigned long long seed, int want_vectors,
                 double* s_out, double* U_out, double* Vt_out, mr_svds_result* out) {
  return mr::svds_guarded([&]() {
    return mr::svds_entry(ctx, k, ncv, tol, maxiter, v0_or_null, seed, want_vectors, s_out, U_out,
                          Vt_out, out);
  });
}

int mr_lsqr_svds_residuals(mr_lsqr* ctx, int k, double* resid_out) {
  MR_CHECK(ctx && resid_out, "svds: null argument");
  const mr::SvdsHost H = mr::svds_host_of(ctx);
  MR_CHECK(*H.work && (int)(*H.work)->last_resid.size() == k && k > 0,
           "svds: no truncated SVD of this k has run on the context");
  std::copy((*H.work)->last_resid.begin(), (*H.work)->last_resid.end(), resid_out);
  return 0;
}

int mr_svds_get_stats(mr_lsqr* ctx, mr_svds_stats* out) {
  MR_CHECK(ctx && out, "null argument");
  const mr::SvdsHost H = mr::svds_host_of(ctx);
  *out = *H.work ? (*H.work)->stats : mr_svds_stats{};
  return 0;
}

int mr_basis_plan(long long n, long long* blocks_out, long long* rows_per_pass_out) {
  MR_CHECK(n >= 0 && blocks_out && rows_per_pass_out, "basis plan: bad argument");
  *blocks_out = mr::basis_grid(n);
  *rows_per_pass_out = (long long)mr::basis_grid(n) * mr::kBasisThreads;
  return 0;
}

int mr_basis_orth(int device, long long n, int j, const double* basis, double* w_inout,
                  double* h_out, double* norm_out) {
  return mr::svds_guarded([&]() -> int {
    MR_CHECK(n >= 1 && j >= 0, "basis orth: n must be >= 1 and j >= 0");
    MR_CHECK(w_inout && norm_out && (j == 0 || (basis && h_out)), "basis orth: null argument");
    MR_HIP(hipSetDevice(device));
    mr::DevBuf mem;
    mr::OrthScratch sc;
    double *db = nullptr, *dw = nullptr;
    int rc = -1;
    if (!mem.get(&db, (size_t)n * j) && !mem.get(&dw, (size_t)n) && !sc.reserve(j)) {
      rc = [&]() -> int {
        if (j) MR_H2D(db, basis, (size_t)n * j * 8, nullptr);
        MR_H2D(dw, w_inout, (size_t)n * 8, nullptr);
        if (mr::launch_orth(nullptr, sc, n, n, j, db, dw, false, norm_out)) return -1;
        MR_D2H(w_inout, dw, (size_t)n * 8, nullptr);
        if (j) MR_D2H(h_out, sc.hacc, (size_t)j * 8, nullptr);
        MR_HIP(hipStreamSynchronize(nullptr));
        return 0;
      }();
    }
    if (rc) (void)hipDeviceSynchronize();
    sc.release();
    return rc;
  });
}

int mr_basis_combine(int device, long long n, int m, int r, const double* basis,
                     const double* Y, double* out) {
  return mr::svds_guarded([&]() -> int {
    MR_CHECK(n >= 1 && m >= 0 && r >= 1, "basis combine: n and r must be >= 1, m >= 0");
    MR_CHECK(out && (m == 0 || (basis && Y)), "basis combine: null argument");
    MR_HIP(hipSetDevice(device));
    mr::DevBuf mem;
    double *db = nullptr, *dy = nullptr, *dout = nullptr;
    if (mem.get(&db, (size_t)n * m) || mem.get(&dy, (size_t)m * r) ||
        mem.get(&dout, (size_t)n * r))
      return -1;
    if (m) {
      MR_H2D(db, basis, (size_t)n * m * 8, nullptr);
      MR_H2D(dy, Y, (size_t)m * r * 8, nullptr);
    }
    if (mr::launch_combine(nullptr, n, n, m, r, db, dy, n, dout)) return -1;
    MR_D2H(out, dout, (size_t)n * r * 8, nullptr);
    MR_HIP(hipStreamSynchronize(nullptr));
    return 0;
  });
}

}  // extern "C"
