"""The blocked exact solve (csrc/cholesky.hip, MR_OPT_SOLVE_BLOCKED = 1)
beside the LDS kernel (solve_kernel, the default) on the bench workload
(DESIGN.md "Blocked exact solve"): MR_K_SOLVE per half-step, HIP-event times
from the engine's own timing (mr_stats), same context, same factors, same
normal equations; ML-full-shape synthetic, lambda = 0.05 weighted.

  python tools/solve_bench.py [--k 64 128 256 512] [--reps 3]

k <= 128: both kernels, their ratio and the largest difference between the
factors they return.  k > 128 (the LDS kernel refuses): the blocked kernel
alone, with the solve phase of a CG half-step (the reference's stop rule) of
the same context beside it for scale; the ratings are the k = 128 shrunk set
(the generator's degree pruning at k + 1 ratings per user leaves nothing at
k = 256), so most blocks have fewer ratings than unknowns and are positive
definite through lambda alone.  "fp64_fraction" is E K^3 / 3 FMAs
(2 flop each) over the time, against 78.6 TFLOP/s.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from movie_recommender_amd.engine import AlsContext
from reg_bench import load

SIDES = ("users", "items")
FP64_PEAK = 78.6e12


def solve_ms(ctx, U, V, reps):
    """Median MR_K_SOLVE time of the users and the items half-step of one
    iteration from (U, V), the first repetition dropped as a warm-up; the
    factors after the last repetition."""
    ms = {s: [] for s in SIDES}
    for rep in range(reps + 1):
        ctx.set_factors(U, V)
        for side in SIDES:
            ctx.reset_stats()
            ctx.half_step(side)
            st = ctx.stats()
            assert st["kernel_launches"]["solve"] == 1
            if rep:
                ms[side].append(st["kernel_ms"]["solve"])
    return {s: round(float(np.median(v)), 4) for s, v in ms.items()}, ctx.get_factors()


def cg_phase_ms(ctx, U, V, reps):
    ms = {s: [] for s in SIDES}
    its = {}
    for rep in range(reps + 1):
        ctx.set_factors(U, V)
        for side in SIDES:
            ctx.reset_stats()
            its[side] = ctx.half_step(side)[0]
            if rep:
                ms[side].append(ctx.stats()["phase_ms"]["solve_" + side])
    return {s: round(float(np.median(v)), 4) for s, v in ms.items()}, its


def fraction(ms, E, K):
    return round(2.0 * E * K ** 3 / 3.0 / (ms * 1e-3) / FP64_PEAK, 4)


def run(a, k):
    rs = load(a.shape, min(k, 128))
    rng = np.random.RandomState(0)
    U0 = rng.uniform(-1, 1, rs.num_users * (k + 1))
    V0 = rng.uniform(-1, 1, rs.num_items * k)
    E = {"users": (rs.num_users, k + 1), "items": (rs.num_items, k)}
    out = {"k": k, "ratings_of_k": min(k, 128), "N": int(rs.n), "users": rs.num_users,
           "items": rs.num_items, "lambda": a.reg, "reg_mode": "weighted", "note": "ms per solve launch (MR_K_SOLVE)"}
    with AlsContext(rs.user_ids, rs.item_ids, rs.ratings, k, rs.num_users, rs.num_items,
                    solver="cholesky", reg=a.reg, reg_mode="weighted", timing=True) as ctx:
        if k <= 128:
            out["lds_ms"], (Ul, Vl) = solve_ms(ctx, U0, V0, a.reps)
            out["lds_fp64_fraction"] = {s: fraction(out["lds_ms"][s], *E[s]) for s in SIDES}
        ctx.set_option("solve_blocked", 1)
        out["blocked_ms"], (Ub, Vb) = solve_ms(ctx, U0, V0, a.reps)
        out["blocked_fp64_fraction"] = {s: fraction(out["blocked_ms"][s], *E[s]) for s in SIDES}
        out["nonpd"] = [ctx.stats()["nonpd_users"], ctx.stats()["nonpd_items"]]
        if k <= 128:
            out["blocked/lds"] = {s: round(out["blocked_ms"][s] / out["lds_ms"][s], 3)
                                  for s in SIDES}
            out["max_abs_difference"] = [float(np.max(np.abs(Ub - Ul))),
                                         float(np.max(np.abs(Vb - Vl)))]
        else:
            ctx.set_solver("cg")
            out["cg_solve_phase_ms"], out["cg_iterations"] = cg_phase_ms(ctx, U0, V0, a.reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, nargs="+", default=[64, 128, 256, 512])
    ap.add_argument("--shape", default="ml-full")
    ap.add_argument("--reg", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    for k in a.k:
        print(json.dumps(run(a, k)), flush=True)


if __name__ == "__main__":
    main()
