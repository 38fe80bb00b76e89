"""Truncated SVD (PureSVD's factorisation) on synth's ML-full-shape rating
matrix: k = 64, the default ncv, on one resident context.

    python tools/svds_bench.py [--scale 1.0] [--k 64] [--tol 0] [--maxiter 200]
                               [--timed-restarts 8] [--cpu-scale 0.05]
                               [--out profiles/svds/svds_bench.json]

Reports the untimed run (wall ms, restarts, SpMV count, converged or not
within --maxiter restarts), then a run of --timed-restarts restarts with HIP
events per kernel class: ms per Lanczos step for A, A^T, the orthogonalisation
and the restart combine, and the orthogonalisation kernels' fraction of their
byte floor -- the dot and the update of one CGS pass each read (j + 1) n 8
bytes of basis and vector, CGS2 runs two passes (``mr_svds_stats.orth_bytes``
counts exactly these) -- against 8 TB/s.  Beside them SciPy's ``svds`` on the
CPU on a --cpu-scale slice of the same generator (threads as the environment
sets them).  Prints ONE JSON line and writes it to --out.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0


def rating_csr(scale):
    from movie_recommender_amd import synth
    nu, ni, nd = synth.SHAPES["ml-full"]
    nu, ni, nd = max(1, int(nu * scale)), max(1, int(ni * scale)), max(1, int(nd * scale))
    u, i, r = synth.raw_pairs(nu, ni, nd)          # sorted by (user, item), de-duplicated
    rp = np.zeros(nu + 1, np.int64)
    np.cumsum(np.bincount(u, minlength=nu), out=rp[1:])
    return rp, i.astype(np.int64), r.astype(np.float64), nu, ni


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--tol", type=float, default=0.0)
    ap.add_argument("--maxiter", type=int, default=200)
    ap.add_argument("--timed-restarts", type=int, default=8)
    ap.add_argument("--cpu-scale", type=float, default=0.05)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svds", "svds_bench.json"))
    args = ap.parse_args()
    from movie_recommender_amd.lsqr import LsqrContext
    from movie_recommender_amd.svds import SvdsNoConvergence, default_ncv

    rp, ci, v, rows, cols = rating_csr(args.scale)
    k = args.k
    ncv = default_ncv(k, min(rows, cols))
    out = {"rows": rows, "cols": cols, "nnz": len(v), "k": k, "ncv": ncv, "tol": args.tol}

    def run(ctx, maxiter):
        t0 = time.perf_counter()
        try:
            s = ctx.svds(k=k, tol=args.tol, maxiter=maxiter, return_singular_vectors=False)
            top = float(s[-1])
        except SvdsNoConvergence:
            top = None
        wall = (time.perf_counter() - t0) * 1e3
        r = ctx.last_svds
        return {"wall_ms": round(wall, 2), "converged": r["converged"], "nconv": r["nconv"],
                "restarts": r["restarts"], "spmv": r["spmv"], "sigma_1": r["anorm"],
                "max_residual": r["max_residual"], "largest_returned": top}

    with LsqrContext((rp, ci, v, cols)) as ctx:
        run(ctx, 1)                                   # warm-up: allocation, first launches
        out["run"] = run(ctx, args.maxiter)
        ctx.set_timing(True)
        ctx.reset_stats()
        s0 = ctx.svds_stats()
        out["timed_run"] = run(ctx, args.timed_restarts)
        ls, s1 = ctx.stats(), ctx.svds_stats()
        ctx.set_timing(False)
    steps = s1["steps"] - s0["steps"]
    orth_ms = s1["kernel_ms"]["orth"] - s0["kernel_ms"]["orth"]
    comb_ms = s1["kernel_ms"]["combine"] - s0["kernel_ms"]["combine"]
    orth_bytes = s1["orth_bytes"] - s0["orth_bytes"]
    out["timed"] = {
        "steps": steps,
        "ms_per_step": {"a": round(ls["kernel_ms"]["ka"] / max(steps, 1), 4),
                        "at": round(ls["kernel_ms"]["kt"] / max(steps, 1), 4),
                        "orth": round(orth_ms / max(steps, 1), 4),
                        "combine": round(comb_ms / max(steps, 1), 4)},
        "orth_ms": round(orth_ms, 3), "orth_bytes": orth_bytes,
        "orth_fraction_of_byte_floor": (round(orth_bytes / (orth_ms / 1e3) / 1e9 / HBM_PEAK_GBS, 4)
                                        if orth_ms > 0 else None),
        "combine_ms_per_restart": round(comb_ms / max(out["timed_run"]["restarts"], 1), 3)}

    if args.cpu_scale > 0:
        import scipy.sparse as sp
        import scipy.sparse.linalg as spl
        rp, ci, v, rows, cols = rating_csr(args.scale * args.cpu_scale)
        A = sp.csr_matrix((v, ci, rp), shape=(rows, cols))
        kc = min(k, min(rows, cols) - 1)
        t0 = time.perf_counter()
        s = spl.svds(A, k=kc, tol=args.tol, return_singular_vectors=False)
        out["scipy_cpu_slice"] = {"rows": rows, "cols": cols, "nnz": A.nnz, "k": kc,
                                  "wall_ms": round((time.perf_counter() - t0) * 1e3, 2),
                                  "sigma_1": float(np.max(s)),
                                  "threads": os.environ.get("OMP_NUM_THREADS")}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
