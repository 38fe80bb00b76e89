"""LSQR against CG on the matrix of bench_cg.py (27e6 x 2.8e6, 10 per row):
ms per LSQR iteration and per kernel class (HIP events), beside ``mr_cg``'s ms
per CG iteration from the same process, and each kernel's algorithmic-byte
fraction of HBM.

    python tools/lsqr_bench.py [--rows 27e6] [--cols 2.8e6] [--per-row 10]
                               [--iterations 50]

Algorithmic bytes per LSQR iteration (nnz non-zeros):
  ka   uh = A v - alfa u    nnz 12 + rows (8 u read + 8 u write)
  kt   vh = A^T u - beta v  nnz 12 + cols (8 vh read + 8 vh write)
  kx   dk, x, w             cols (8 vh + 8 w read + 8 w write + 8 x read + 8 x write)
and per CG iteration as bench_cg.py counts them, less the gathered vectors
and row offsets so that both are counted by one rule:
  spmv_a  nnz 12 + rows 8 (t write)      spmv_at  nnz 12 + cols 8 (q write)
Prints ONE JSON line.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0


def frac(nbytes, avg_ms):
    return round(nbytes / (avg_ms / 1e3) / 1e9 / HBM_PEAK_GBS, 4) if avg_ms > 0 else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=27e6)
    ap.add_argument("--cols", type=float, default=2.8e6)
    ap.add_argument("--per-row", type=int, default=10)
    ap.add_argument("--iterations", type=int, default=50)
    args = ap.parse_args()
    rows, cols, per = int(args.rows), int(args.cols), args.per_row
    from bench_cg import alg_bytes, bench_matrix
    from movie_recommender_amd import _lib
    from movie_recommender_amd.lsqr import LsqrContext
    rp, ci, v, b = bench_matrix(rows, cols, per)
    nnz = len(v)
    out = {"rows": rows, "cols": cols, "nnz": nnz, "iterations": args.iterations}

    with LsqrContext((rp, ci, v, cols)) as ctx:
        ctx.solve(b, iter_lim=2, atol=0.0, btol=0.0, conlim=0.0)   # warm-up
        ctx.set_timing(True)
        ctx.reset_stats()
        _, r = ctx.solve(b, iter_lim=args.iterations, atol=0.0, btol=0.0, conlim=0.0)
        s = ctx.stats()
    by = {"ka": nnz * 12 + rows * 16, "kt": nnz * 12 + cols * 16, "kx": cols * 40}
    kern = {}
    for c in ("ka", "kt", "kx"):
        n = s["kernel_launches"][c]
        avg = s["kernel_ms"][c] / max(n, 1)
        kern[c] = {"launches": n, "avg_us": round(avg * 1e3, 2), "alg_bytes": by[c],
                   "hbm_frac": frac(by[c], avg)}
    iters_timed = max(s["kernel_launches"]["ka"], 1)
    lsqr_ms = sum(s["kernel_ms"][c] for c in ("ka", "kt", "kx")) / iters_timed
    out["lsqr"] = {"istop": r["istop"], "itn": r["itn"], "ms_per_iteration": round(lsqr_ms, 4),
                   "solve_ms": round(s["solve_ms"], 3),
                   "setup_ms": round(s["kernel_ms"]["setup"], 3), "kernels": kern}

    L = _lib.lib()
    h = L.mr_cg_create(0, rows, cols, rp.ctypes.data_as(_lib.IP), ci.ctypes.data_as(_lib.IP),
                       v.ctypes.data_as(_lib.DP))
    if not h:
        raise RuntimeError(_lib.last_error())
    try:
        x = np.zeros(cols)
        rr = ctypes.c_double(0)
        _lib.check(L.mr_cg_solve(h, b.ctypes.data_as(_lib.DP), x.ctypes.data_as(_lib.DP), 0.01, 2,
                                 ctypes.byref(rr)), "mr_cg_solve")
        _lib.check(L.mr_cg_set_timing(h, 1), "mr_cg_set_timing")
        _lib.check(L.mr_cg_reset_stats(h), "mr_cg_reset_stats")
        x = np.zeros(cols)
        it = _lib.check(L.mr_cg_solve(h, b.ctypes.data_as(_lib.DP), x.ctypes.data_as(_lib.DP),
                                      0.01, args.iterations, ctypes.byref(rr)), "mr_cg_solve")
        st = _lib.MrCgStats()
        _lib.check(L.mr_cg_get_stats(h, ctypes.byref(st)), "mr_cg_get_stats")
        c = st.as_dict()
    finally:
        L.mr_cg_destroy(h)
    cby = {"spmv_a": nnz * 12 + rows * 8, "spmv_at": nnz * 12 + cols * 8, "update": cols * 48}
    ck = {}
    for name in ("spmv_a", "spmv_at", "update"):
        n = c["kernel_launches"][name]
        avg = c["kernel_ms"][name] / max(n, 1)
        ck[name] = {"launches": n, "avg_us": round(avg * 1e3, 2), "alg_bytes": cby[name],
                    "hbm_frac": frac(cby[name], avg),
                    # by bench_cg.py's count (gathered vectors and offsets included)
                    "hbm_frac_bench_cg": frac(alg_bytes(name, rows, cols, nnz), avg)}
    cg_ms = sum(c["kernel_ms"][n] for n in ("spmv_a", "spmv_at", "update")) / \
        max(c["kernel_launches"]["spmv_a"], 1)
    out["cg"] = {"iterations": it, "ms_per_iteration": round(cg_ms, 4), "kernels": ck}
    out["lsqr_over_cg"] = round(lsqr_ms / cg_ms, 4) if cg_ms > 0 else None
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
