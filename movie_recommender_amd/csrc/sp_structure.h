// The device structure behind the CSR-stream SpMV of a general sparse matrix
// (cgls.hip, lsqr.hip): A with its rows ordered by first column, its explicit
// transpose, and the row blocks of both.  Built once per context
// (SpStructure::build, cgls.hip).
#pragma once
#include <vector>

#include "mr_internal.h"

namespace mr {

template <typename T>
int sp_dmalloc(T** p, int64_t n, std::vector<void*>& owned) {
  *p = nullptr;
  MR_HIP(hipMalloc((void**)p, (size_t)std::max<int64_t>(n, 1) * sizeof(T)));
  owned.push_back(*p);
  return 0;
}

// Per-kernel-class timing of a solver's launches with HIP events: a timed
// launch takes an event pair through the launch-timing slot (MR_LAUNCH).
struct LaunchTimer {
  bool timing = false;
  struct Timed {
    int cls, it;
    hipEvent_t a, b;
  };
  std::vector<Timed> pend;
  std::vector<hipEvent_t> pool;

  int ev(hipEvent_t* e) {
    if (!pool.empty()) {
      *e = pool.back();
      pool.pop_back();
      return 0;
    }
    MR_HIP(hipEventCreate(e));
    return 0;
  }
  int tic(int cls, int it) {
    if (!timing) return 0;
    Timed tm{cls, it, nullptr, nullptr};
    if (ev(&tm.a) || ev(&tm.b)) return -1;
    t_launch.start = tm.a;
    t_launch.stop = tm.b;
    pend.push_back(tm);
    return 0;
  }
  int toc(hipStream_t s) {
    if (!timing) return 0;
    if (t_launch.start) {   // nothing was launched: an empty interval
      MR_HIP(hipEventRecord(pend.back().a, s));
      MR_HIP(hipEventRecord(pend.back().b, s));
    }
    t_launch = LaunchTiming{};
    return 0;
  }
  void destroy_events() {
    for (auto& e : pool) (void)hipEventDestroy(e);
    for (auto& e : pend) {
      (void)hipEventDestroy(e.a);
      (void)hipEventDestroy(e.b);
    }
    pool.clear();
    pend.clear();
  }
};

struct SpStructure {
  int64_t rows = 0, cols = 0, nnz = 0;
  int64_t *rp = nullptr, *tp = nullptr;         // row offsets of A and of A^T
  int64_t *blk_a = nullptr, *blk_t = nullptr;   // (first row, its first non-zero) pairs
  int64_t n_blk_a = 0, n_blk_t = 0;
  int32_t *ci = nullptr, *ti = nullptr;         // ids, padded by kSpPad entries
  int32_t* perm = nullptr;                      // perm[i] = the caller's row of row i
  double *v = nullptr, *tv = nullptr;           // values, padded by kSpPad entries

  // The caller's CSR arrays checked on the host (no device call).
  static int check(int rows_, int cols_, const int* hrp, const int* hci, const double* hv);
  // Uploads the (checked) CSR arrays on s, sorts the rows, transposes and
  // cuts the row blocks; every array is added to `owned`.  The values travel
  // with their entries, so a caller that passes hv[j] = j finds in v / tv
  // the caller's index of every stored entry.
  int build(hipStream_t s, int rows_, int cols_, const int* hrp, const int* hci, const double* hv,
            std::vector<void*>& owned);
};

}  // namespace mr
