"""Measurements of the regularised-ALS additions on the bench workload
(DESIGN.md "Regularised ALS").  HIP-event kernel / phase times come from the
engine's own timing (mr_stats); step and objective() times are host clocks
around work that ends in a device synchronise.

  python tools/reg_bench.py --mode step [--k 64]     wall time of an ALS step
      at lambda = 0 (no stats are read, so MR_LIB_PATH may point at an older
      library: run it alternately on both for an A/B)
  python tools/reg_bench.py --mode reg  [--k 64]     the ridge pass per side
      against its byte floor, the unfused start's cost at fixed CG counts,
      objective() and sse() against the users Gram
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from movie_recommender_amd import synth
from movie_recommender_amd.engine import AlsContext

HBM_MEASURED = 6.29e12   # bytes/s, float4 copy on MI355X


def load(shape, k):
    cache = f"/tmp/mr_bench_{shape}_k{k}_{synth.DATA_SEED}.npz"
    if os.path.exists(cache):
        d = np.load(cache)
        return synth.RatingSet(d["u"], d["i"], d["r"], int(d["nu"]), int(d["ni"]), k)
    rs = synth.movielens_like(shape, k)
    np.savez(cache, u=rs.user_ids, i=rs.item_ids, r=rs.ratings, nu=rs.num_users, ni=rs.num_items)
    return rs


def diag_lines(k):
    """64-byte lines of one entity's tri16 block that hold a diagonal entry
    (csrc/mr_internal.h packed_offset(i, i, nb)); blocks start line-aligned."""
    nb = (k + 15) // 16
    n_off = nb * (nb - 1) // 2
    n_tiles = n_off + nb // 2 + (nb & 1)
    lines = set()
    for i in range(k):
        b, r = i % nb, i // nb
        if (nb & 1) and b == nb - 1:
            o = (n_off + nb // 2) * 256 + r * 17
        elif b % 2 == 0:
            o = (n_off + b // 2) * 256 + r * 17
        else:
            o = n_tiles * 256 + (b // 2) * 16 + r
        lines.add(o * 4 // 64)
    return len(lines)


def mode_step(a, rs, U0, V0):
    k = a.k
    with AlsContext(rs.user_ids, rs.item_ids, rs.ratings, k, rs.num_users, rs.num_items) as ctx:
        ctx.set_factors(U0, V0)
        ctx.iterate(a.warmup)
        ctx.sync()
        ms = []
        for _ in range(a.reps):
            t = time.perf_counter()
            ctx.iterate(a.steps)
            ctx.sync()
            ms.append((time.perf_counter() - t) * 1e3 / a.steps)
    return {"mode": "step", "lib": os.environ.get("MR_LIB_PATH", "tree"), "k": k,
            "step_ms": [round(x, 3) for x in ms], "median_ms": round(float(np.median(ms)), 3)}


def mode_reg(a, rs, U0, V0):
    k, lam = a.k, 0.05
    out = {"mode": "reg", "k": k, "N": int(rs.n), "users": rs.num_users, "items": rs.num_items}
    cnt = {"users": np.bincount(rs.user_ids, minlength=rs.num_users),
           "items": np.bincount(rs.item_ids, minlength=rs.num_items)}
    with AlsContext(rs.user_ids, rs.item_ids, rs.ratings, k, rs.num_users, rs.num_items,
                    timing=True) as ctx:
        ctx.set_factors(U0, V0)
        # -- the ridge pass per side, against its byte floor
        ctx.set_regularization(lam, "weighted")
        for side in ("users", "items"):
            ctx.build_normal_equations(side)            # warm-up
            ctx.reset_stats()
            for _ in range(a.reps):
                ctx.build_normal_equations(side)
            st = ctx.stats()
            ms = st["kernel_ms"]["regularize"] / st["kernel_launches"]["regularize"]
            gram = st["kernel_ms"]["gram_" + side] / st["kernel_launches"]["gram_" + side]
            floor_bytes = 2 * 64 * diag_lines(k) * int((cnt[side] > 0).sum())
            out["ridge_" + side] = {
                "ms": round(ms, 4), "gram_ms": round(gram, 4), "floor_MB": round(floor_bytes / 1e6, 1),
                "floor_ms_at_6.29TBs": round(floor_bytes / HBM_MEASURED * 1e3, 4),
                "fraction_of_floor_rate": round(floor_bytes / HBM_MEASURED * 1e3 / ms, 3)}
        # -- the start: fused (lambda = 0), unfused (lambda = 0), unfused + pass
        # (lambda > 0), the same factors and a fixed CG count per half-step
        for name, lam_, fuse in (("fused_lam0", 0.0, 1), ("unfused_lam0", 0.0, 0),
                                 ("lam>0", lam, 1)):
            ctx.set_regularization(lam_, "weighted")
            ctx.set_option("fuse_start", fuse)
            rec = {}
            for rep in range(a.reps + 1):
                ctx.set_factors(U0, V0)
                if rep == 1:
                    ctx.reset_stats()                   # rep 0 is the warm-up
                its = [ctx.half_step(s, 0.0, a.cg)[0] for s in ("users", "items")]
            st = ctx.stats()
            rec["cg_its"] = its
            for ph in ("gram_users", "solve_users", "gram_items", "solve_items"):
                rec[ph + "_ms"] = round(st["phase_ms"][ph] / a.reps, 4)
            rec["half_steps_ms"] = round(sum(st["phase_ms"].values()) / a.reps, 4)
            out[name] = rec
        ctx.set_option("fuse_start", 1)
        # -- objective() and sse(): host wall per call (allocations, the D2H
        # of the result and the synchronise included)
        ctx.set_regularization(lam, "weighted")
        ctx.set_factors(U0, V0)
        o = ctx.objective()
        t = time.perf_counter()
        for _ in range(a.reps):
            o2 = ctx.objective()
        out["objective_wall_ms"] = round((time.perf_counter() - t) * 1e3 / a.reps, 4)
        out["objective_bitwise_repeat"] = o == o2
        out["objective"] = o
        n = min(rs.n, 1_000_000)
        t = time.perf_counter()
        for _ in range(a.reps):
            s = ctx.sse(rs.user_ids[:n], rs.item_ids[:n], rs.ratings[:n])
        out["sse_1M_wall_ms"] = round((time.perf_counter() - t) * 1e3 / a.reps, 4)
        out["sse_1M"] = s
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["step", "reg"], required=True)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--shape", default="ml-full")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3, help="ALS iterations per timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cg", type=int, default=6, help="CG iterations per half-step (mode reg)")
    a = ap.parse_args()
    rs = load(a.shape, a.k)
    rng = np.random.RandomState(0)
    U0 = rng.uniform(-1, 1, rs.num_users * (a.k + 1))
    V0 = rng.uniform(-1, 1, rs.num_items * a.k)
    res = (mode_step if a.mode == "step" else mode_reg)(a, rs, U0, V0)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
