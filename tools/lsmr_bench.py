"""LSMR against LSQR on the matrix of bench_cg.py (27e6 x 2.8e6, 10 per row),
both on one resident context in one process: ms per iteration and per kernel
class (HIP events), each kernel's algorithmic-byte fraction of HBM, and the
(istop, itn) both solvers reach at SciPy's default tolerances -- the count
the reference's lsmr / lsqr comparison (python/basics/lsmr.py) is about.

    python tools/lsmr_bench.py [--rows 27e6] [--cols 2.8e6] [--per-row 10]
                               [--iterations 50] [--default-cap 2000]

Algorithmic bytes per iteration (nnz non-zeros); KA and KT are one kernel for
both solvers:
  ka        uh = A v - alfa u    nnz 12 + rows (8 u read + 8 u write)
  kt        vh = A^T u - beta v  nnz 12 + cols (8 vh read + 8 vh write)
  kx lsqr   dk, x, w             cols 40 (vh, w, x read; w, x write)
  kx lsmr   hbar, x, h           cols 56 (vh, h, hbar, x read; h, hbar, x write)
Prints ONE JSON line.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0
ZERO = dict(atol=0.0, btol=0.0, conlim=0.0)


def frac(nbytes, avg_ms):
    return round(nbytes / (avg_ms / 1e3) / 1e9 / HBM_PEAK_GBS, 4) if avg_ms > 0 else None


def timed(ctx, solve, by):
    """One timed solve's per-kernel-class table and ms per iteration."""
    ctx.set_timing(True)
    ctx.reset_stats()
    _, r = solve()
    s = ctx.stats()
    ctx.set_timing(False)
    kern = {}
    for c in ("ka", "kt", "kx"):
        n = s["kernel_launches"][c]
        avg = s["kernel_ms"][c] / max(n, 1)
        kern[c] = {"launches": n, "avg_us": round(avg * 1e3, 2), "alg_bytes": by[c],
                   "hbm_frac": frac(by[c], avg)}
    ms = sum(s["kernel_ms"][c] for c in ("ka", "kt", "kx")) / max(s["kernel_launches"]["ka"], 1)
    return {"istop": r["istop"], "itn": r["itn"], "ms_per_iteration": round(ms, 4),
            "solve_ms": round(s["solve_ms"], 3), "setup_ms": round(s["kernel_ms"]["setup"], 3),
            "kernels": kern}, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=27e6)
    ap.add_argument("--cols", type=float, default=2.8e6)
    ap.add_argument("--per-row", type=int, default=10)
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--default-cap", type=int, default=2000,
                    help="iteration limit of the runs at SciPy's default tolerances")
    args = ap.parse_args()
    rows, cols, per = int(args.rows), int(args.cols), args.per_row
    from bench_cg import bench_matrix
    from movie_recommender_amd.lsqr import LsqrContext
    rp, ci, v, b = bench_matrix(rows, cols, per)
    nnz = len(v)
    n = args.iterations
    out = {"rows": rows, "cols": cols, "nnz": nnz, "iterations": n}
    by = {"ka": nnz * 12 + rows * 16, "kt": nnz * 12 + cols * 16}

    with LsqrContext((rp, ci, v, cols)) as ctx:
        ctx.solve(b, iter_lim=2, **ZERO)          # warm-up of both
        ctx.solve_lsmr(b, maxiter=2, **ZERO)
        out["lsqr"], lsqr_ms = timed(ctx, lambda: ctx.solve(b, iter_lim=n, **ZERO),
                                     dict(by, kx=cols * 40))
        out["lsmr"], lsmr_ms = timed(ctx, lambda: ctx.solve_lsmr(b, maxiter=n, **ZERO),
                                     dict(by, kx=cols * 56))
        out["lsmr_over_lsqr"] = round(lsmr_ms / lsqr_ms, 4) if lsqr_ms > 0 else None
        # SciPy's default tolerances (1e-6, 1e-6, 1e8); SciPy's own limits are
        # 2 cols (lsqr) and min(rows, cols) (lsmr), capped here
        ctx.set_timing(True)
        for name, solve in (("lsqr", lambda: ctx.solve(b, iter_lim=min(2 * cols, args.default_cap))),
                            ("lsmr", lambda: ctx.solve_lsmr(b, maxiter=min(rows, cols,
                                                                          args.default_cap)))):
            ctx.reset_stats()
            _, r = solve()
            out[name + "_default_tolerances"] = {
                "istop": r["istop"], "itn": r["itn"],
                "solve_ms": round(ctx.stats()["solve_ms"], 3)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
