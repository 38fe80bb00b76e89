// Stand-alone check of the truncated SVD's host code (csrc/svds_host.h): the
// splitmix64 stream, the one-sided Jacobi SVD and the restart bookkeeping.
// No device, no library:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/svds_host_check.cpp -o svds_host_check && ./svds_host_check
// Every matrix is drawn from the stream (seed = its size), so
// tests/svds_cases.Rng rebuilds it in NumPy; the singular values are printed
// one per line ("sigma <case> <index> <value>") for that comparison, and the
// factorisation is checked here: |B - X S Y^T|, |X^T X - I|, |Y^T Y - I|.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../movie_recommender_amd/csrc/svds_host.h"

static int failures = 0;

#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                 \
    }                                                             \
  } while (0)

static void check_svd(const std::string& name, int r, int n, const std::vector<double>& A) {
  std::vector<double> X((size_t)r * n), Y((size_t)n * n), sig(n);
  const int sweeps = mr::svds_jacobi_rect(r, n, A.data(), X.data(), sig.data(), Y.data());
  double amax = 0.0, rec = 0.0, ox = 0.0, oy = 0.0;
  for (double v : A) amax = std::max(amax, std::fabs(v));
  for (int i = 0; i < r; ++i)
    for (int j = 0; j < n; ++j) {
      double s = 0.0;
      for (int c = 0; c < n; ++c) s += X[(size_t)i * n + c] * sig[c] * Y[(size_t)j * n + c];
      rec = std::max(rec, std::fabs(s - A[(size_t)i * n + j]));
    }
  for (int a = 0; a < n; ++a)
    for (int b = 0; b < n; ++b) {
      double sx = 0.0, sy = 0.0;
      for (int i = 0; i < r; ++i) sx += X[(size_t)i * n + a] * X[(size_t)i * n + b];
      for (int i = 0; i < n; ++i) sy += Y[(size_t)i * n + a] * Y[(size_t)i * n + b];
      ox = std::max(ox, std::fabs(sx - (a == b)));
      oy = std::max(oy, std::fabs(sy - (a == b)));
    }
  for (int c = 0; c + 1 < n; ++c) EXPECT(sig[c] >= sig[c + 1]);
  for (int c = 0; c < n; ++c) std::printf("sigma %s %d %.17g\n", name.c_str(), c, sig[c]);
  std::printf("check %s sweeps %d rec %.3g orthX %.3g orthY %.3g\n", name.c_str(), sweeps, rec, ox,
              oy);
  const double lim = 64.0 * n * mr::kSvdsEps;
  EXPECT(sweeps < 60);
  EXPECT(rec <= lim * std::max(amax, 1e-300) * std::max(1.0, std::sqrt((double)n)));
  EXPECT(ox <= lim);
  EXPECT(oy <= lim);
}

static std::vector<double> dense(int n, bool upper) {
  mr::SvdsRng rng((uint64_t)n);
  std::vector<double> B((size_t)n * n);
  rng.fill(B.data(), (int64_t)n * n);
  if (upper)
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < i; ++j) B[(size_t)i * n + j] = 0.0;
  return B;
}

int main() {
  // the stream: splitmix64's published first outputs for seed 0
  mr::SvdsRng g(0);
  EXPECT(g.next_u64() == 0xE220A8397B1DCDAFull);
  EXPECT(g.next_u64() == 0x6E789E6AA1B965F4ull);
  EXPECT(g.next_u64() == 0x06C45D188009454Full);
  mr::SvdsRng g2(12345);
  for (int i = 0; i < 100000; ++i) {
    const double v = g2.next();
    EXPECT(v > -1.0 && v < 1.0);
  }

  // hand cases
  {
    std::vector<double> B{-3.0};
    double X, Y, s;
    mr::svds_jacobi(1, B.data(), &X, &s, &Y);
    EXPECT(s == 3.0 && X * s * Y == -3.0);
    std::vector<double> C{3.0, 0.0, 4.0, 5.0};
    std::vector<double> X2(4), Y2(4), s2(2);
    mr::svds_jacobi(2, C.data(), X2.data(), s2.data(), Y2.data());
    EXPECT(std::fabs(s2[0] - std::sqrt(45.0)) <= 4 * mr::kSvdsEps * 7.0);
    EXPECT(std::fabs(s2[1] - std::sqrt(5.0)) <= 4 * mr::kSvdsEps * 7.0);
  }
  for (int n : {1, 2, 21, 200}) {
    check_svd("upper" + std::to_string(n), n, n, dense(n, true));
    check_svd("dense" + std::to_string(n), n, n, dense(n, false));
  }
  // the arrow a restart leaves: diag(sig) with one full column
  for (int n : {2, 21, 200}) {
    mr::SvdsRng rng(1000 + (uint64_t)n);
    std::vector<double> B((size_t)n * n, 0.0);
    const int keep = n / 2;
    for (int i = 0; i < keep; ++i) {
      B[(size_t)i * n + i] = 2.0 + rng.next();
      B[(size_t)i * n + keep] = 1e-3 * rng.next();
    }
    for (int i = keep; i < n; ++i) {
      B[(size_t)i * n + i] = 1.0 + rng.next();
      if (i + 1 < n) B[(size_t)i * n + i + 1] = rng.next();
    }
    check_svd("arrow" + std::to_string(n), n, n, B);
  }
  // zero rows and columns (breakdowns), and the zero matrix
  for (int n : {1, 2, 21, 200}) {
    std::vector<double> B = dense(n, true);
    for (int j = 0; j < n; ++j) {
      B[(size_t)(n / 2) * n + j] = 0.0;
      B[(size_t)(n - 1) * n + j] = 0.0;
      B[(size_t)j * n + n / 3] = 0.0;
    }
    check_svd("zerorows" + std::to_string(n), n, n, B);
    check_svd("zero" + std::to_string(n), n, n, std::vector<double>((size_t)n * n, 0.0));
  }
  // the augmented factorisation of a wide matrix's last sweep
  for (int n : {1, 2, 21}) {
    std::vector<double> B = dense(n, true), X((size_t)n * n), sig(n), Ya((size_t)(n + 1) * n);
    mr::svds_jacobi_augmented(n, B.data(), 0.75, X.data(), sig.data(), Ya.data());
    double rec = 0.0;
    for (int i = 0; i < n; ++i)
      for (int j = 0; j <= n; ++j) {
        double s = 0.0;
        for (int c = 0; c < n; ++c) s += X[(size_t)i * n + c] * sig[c] * Ya[(size_t)j * n + c];
        const double want = j < n ? B[(size_t)i * n + j] : (i == n - 1 ? 0.75 : 0.0);
        rec = std::max(rec, std::fabs(s - want));
      }
    std::printf("check augmented%d rec %.3g\n", n, rec);
    EXPECT(rec <= 64.0 * (n + 1) * mr::kSvdsEps);
  }

  // restart bookkeeping
  EXPECT(mr::svds_default_ncv(6, 1000) == 20 && mr::svds_default_ncv(29, 1000) == 59 &&
         mr::svds_default_ncv(3, 5) == 5);
  EXPECT(mr::svds_keep(5, 6, 0) == 5 && mr::svds_keep(5, 11, 0) == 8 &&
         mr::svds_keep(5, 11, 4) == 9 && mr::svds_keep(5, 11, 9) == 10);
  EXPECT(mr::svds_threshold(1e-6, 20, 3.0) == 3e-6);
  EXPECT(mr::svds_threshold(0.0, 20, 3.0) == 8.0 * 20 * mr::kSvdsEps * 3.0);
  {
    const int n = 4;
    std::vector<double> sig{4.0, 3.0, 2.0, 1.0}, X((size_t)n * n, 0.0), B((size_t)n * n, 7.0);
    for (int i = 0; i < n; ++i) X[(size_t)(n - 1) * n + i] = 0.1 * (i + 1) * (i % 2 ? -1 : 1);
    mr::SvdsSweep sw;
    mr::svds_judge(n, sig.data(), X.data(), 1e-3, 1e-3, sw);   // thr = 4e-3
    EXPECT(sw.sigma1 == 4.0 && sw.nconv == 4 && sw.resid[1] == std::fabs(1e-3 * -0.2));
    mr::svds_judge(n, sig.data(), X.data(), 2e-3, 1.25e-4, sw);   // thr 5e-4; resid 2e-4, 4e-4, 6e-4
    EXPECT(sw.nconv == 2);
    mr::svds_restart_b(n, 2, sig.data(), X.data(), 2e-3, B.data());
    const double want[16] = {4.0, 0, 2e-3 * 0.1, 0, 0, 3.0, 2e-3 * -0.2, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 16; ++i) EXPECT(B[i] == want[i]);
  }
  std::printf(failures ? "FAILED (%d)\n" : "ok (%d failures)\n", failures);
  return failures ? 1 : 0;
}
