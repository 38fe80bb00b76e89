// Host side of the truncated sparse SVD (svds.hip; include/mr_lsqr.h): the
// pseudo-random stream, the dense SVD of the projected matrix and the
// thick-restart bookkeeping.  Plain C++ with no device call and no library
// beyond the standard one, so a stand-alone program can run it.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace mr {

constexpr double kSvdsEps = 2.220446049250313e-16;

// splitmix64 mapped to (-1, 1): ((z >> 11) + 0.5) 2^-52 - 1.
struct SvdsRng {
  uint64_t s;
  explicit SvdsRng(uint64_t seed) : s(seed) {}
  uint64_t next_u64() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  double next() { return ((double)(next_u64() >> 11) + 0.5) * (1.0 / 4503599627370496.0) - 1.0; }
  void fill(double* v, int64_t n) {
    for (int64_t i = 0; i < n; ++i) v[i] = next();
  }
};

// A = X diag(sig) Y^T for a dense r x n A (row-major, r >= n), by one-sided
// Jacobi (Hestenes) on A's columns: W = A Y is rotated until its columns are
// orthogonal, sig_i = |w_i|, x_i = w_i / sig_i.  sig descending; X (r x n,
// row-major) has orthonormal columns and Y (n x n, row-major) is orthogonal:
// the left vectors of zero singular values (columns of W at rounding level)
// are completed from unit vectors.  Returns the sweeps taken.
inline int svds_jacobi_rect(int r, int n, const double* A, double* X, double* sig, double* Y) {
  std::vector<double> W((size_t)r * n), V((size_t)n * n, 0.0);   // column-major
  for (int i = 0; i < r; ++i)
    for (int j = 0; j < n; ++j) W[(size_t)j * r + i] = A[(size_t)i * n + j];
  for (int j = 0; j < n; ++j) V[(size_t)j * n + j] = 1.0;
  // a column at or below n eps |A|_F is rounding: it is left alone by the
  // rotations (two such columns never settle against each other) and counts
  // as a zero singular value
  double fro = 0.0;
  for (size_t i = 0; i < (size_t)r * n; ++i) fro += A[i] * A[i];
  const double null2 = (n * kSvdsEps) * (n * kSvdsEps) * fro;
  int sweeps = 0;
  for (; sweeps < 60; ++sweeps) {
    bool rotated = false;
    for (int p = 0; p < n - 1; ++p) {
      for (int q = p + 1; q < n; ++q) {
        double* wp = &W[(size_t)p * r];
        double* wq = &W[(size_t)q * r];
        double a = 0.0, b = 0.0, c = 0.0;
        for (int i = 0; i < r; ++i) {
          a += wp[i] * wp[i];
          b += wq[i] * wq[i];
          c += wp[i] * wq[i];
        }
        if (a <= null2 || b <= null2) continue;
        if (c == 0.0 || std::fabs(c) <= kSvdsEps * std::sqrt(a) * std::sqrt(b)) continue;
        rotated = true;
        const double zeta = (b - a) / (2.0 * c);
        const double t =
            (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
        const double cs = 1.0 / std::sqrt(1.0 + t * t), sn = cs * t;
        for (int i = 0; i < r; ++i) {
          const double x = wp[i], y = wq[i];
          wp[i] = cs * x - sn * y;
          wq[i] = sn * x + cs * y;
        }
        double* vp = &V[(size_t)p * n];
        double* vq = &V[(size_t)q * n];
        for (int i = 0; i < n; ++i) {
          const double vx = vp[i], vy = vq[i];
          vp[i] = cs * vx - sn * vy;
          vq[i] = sn * vx + cs * vy;
        }
      }
    }
    if (!rotated) break;
  }
  std::vector<double> nrm(n);
  std::vector<int> ord(n);
  for (int j = 0; j < n; ++j) {
    double a = 0.0;
    for (int i = 0; i < r; ++i) a += W[(size_t)j * r + i] * W[(size_t)j * r + i];
    nrm[j] = a <= null2 ? 0.0 : std::sqrt(a);
    ord[j] = j;
  }
  std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return nrm[a] > nrm[b]; });
  for (int c = 0; c < n; ++c) {
    const int j = ord[c];
    sig[c] = nrm[j];
    for (int i = 0; i < n; ++i) Y[(size_t)i * n + c] = V[(size_t)j * n + i];
    for (int i = 0; i < r; ++i)
      X[(size_t)i * n + c] = nrm[j] > 0.0 ? W[(size_t)j * r + i] / nrm[j] : 0.0;
  }
  // left vectors of the zero singular values: unit vectors, CGS2 against the rest
  // (zero columns sort last, so columns 0..c-1 are in place when c is filled);
  // the unit vector taken is the one farthest from their span: its distance
  // squared is 1 - sum_d X[t, d]^2 >= (r - c) / r
  std::vector<double> u(r);
  for (int c = 0; c < n; ++c) {
    if (sig[c] > 0.0) continue;
    int best = 0;
    double best_in = 2.0;
    for (int t = 0; t < r; ++t) {
      double in = 0.0;
      for (int d = 0; d < c; ++d) in += X[(size_t)t * n + d] * X[(size_t)t * n + d];
      if (in < best_in) {
        best_in = in;
        best = t;
      }
    }
    std::fill(u.begin(), u.end(), 0.0);
    u[best] = 1.0;
    for (int pass = 0; pass < 2; ++pass)
      for (int d = 0; d < c; ++d) {
        double h = 0.0;
        for (int i = 0; i < r; ++i) h += X[(size_t)i * n + d] * u[i];
        for (int i = 0; i < r; ++i) u[i] -= h * X[(size_t)i * n + d];
      }
    double a = 0.0;
    for (int i = 0; i < r; ++i) a += u[i] * u[i];
    const double inv = a > 0.0 ? 1.0 / std::sqrt(a) : 0.0;
    for (int i = 0; i < r; ++i) X[(size_t)i * n + c] = u[i] * inv;
  }
  return sweeps;
}

// The square case: B = X diag(sig) Y^T, all n x n row-major.
inline int svds_jacobi(int n, const double* B, double* X, double* sig, double* Y) {
  return svds_jacobi_rect(n, n, B, X, sig, Y);
}

// The left basis spans everything (ncv == rows < cols): A = Q [B | beta e_ncv]
// P_{ncv+1}^T exactly, so the SVD of the ncv x (ncv + 1) matrix ends the run.
// Taken on its transpose: X (ncv x ncv) is the orthogonal factor, Yaug
// ((ncv + 1) x ncv, row-major) holds the right vectors' coefficients on
// P[:, :ncv + 1].
inline int svds_jacobi_augmented(int ncv, const double* B, double beta_last, double* X,
                                 double* sig, double* Yaug) {
  std::vector<double> T((size_t)(ncv + 1) * ncv, 0.0);   // [B | beta e]^T, row-major
  for (int i = 0; i < ncv; ++i)
    for (int j = 0; j < ncv; ++j) T[(size_t)j * ncv + i] = B[(size_t)i * ncv + j];
  T[(size_t)ncv * ncv + (ncv - 1)] = beta_last;
  return svds_jacobi_rect(ncv + 1, ncv, T.data(), Yaug, sig, X);
}

// The restart decisions on one sweep's Ritz pairs.
struct SvdsSweep {
  int nconv = 0;          // leading converged pairs
  double thr = 0.0;       // the residual limit used
  double sigma1 = 0.0;    // largest Ritz value seen so far (updated)
  std::vector<double> resid;   // |beta_last X[ncv-1, i]|
};

inline double svds_threshold(double tol, int ncv, double sigma1) {
  return tol > 0.0 ? tol * sigma1 : 8.0 * ncv * kSvdsEps * sigma1;
}

// resid, thr and nconv from (sig, X's last row, beta_last); sw.sigma1 carries
// the largest Ritz value over the sweeps.
inline void svds_judge(int ncv, const double* sig, const double* X, double beta_last, double tol,
                       SvdsSweep& sw) {
  sw.sigma1 = std::max(sw.sigma1, ncv ? sig[0] : 0.0);
  sw.thr = svds_threshold(tol, ncv, sw.sigma1);
  sw.resid.assign(ncv, 0.0);
  for (int i = 0; i < ncv; ++i) sw.resid[i] = std::fabs(beta_last * X[(size_t)(ncv - 1) * ncv + i]);
  sw.nconv = 0;
  while (sw.nconv < ncv && sw.resid[sw.nconv] <= sw.thr) ++sw.nconv;
}

inline int svds_keep(int k, int ncv, int nconv) {
  return std::min(ncv - 1, std::max(k + nconv, k + (ncv - k) / 2));
}

// B after a restart that keeps `keep` Ritz pairs: diag(sig[:keep]) with column
// `keep` = beta_last X[ncv-1, :keep] (the couplings of the carried p_ncv).
inline void svds_restart_b(int ncv, int keep, const double* sig, const double* X,
                           double beta_last, double* B) {
  std::fill(B, B + (size_t)ncv * ncv, 0.0);
  for (int i = 0; i < keep; ++i) {
    B[(size_t)i * ncv + i] = sig[i];
    B[(size_t)i * ncv + keep] = beta_last * X[(size_t)(ncv - 1) * ncv + i];
  }
}

inline int svds_default_ncv(int k, int mn) { return std::min(mn, std::max(2 * k + 1, 20)); }

}  // namespace mr
