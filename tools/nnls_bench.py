"""The non-negative solver beside the Cholesky solver on the bench workload
(DESIGN.md "Non-negative factors"): MR_K_SOLVE per half-step, HIP-event times
from the engine's own timing (mr_stats), same context, same factors, same
normal equations; lambda = 0.05 weighted, explicit ratings.

  python tools/nnls_bench.py [--k 64 128] [--reps 3]

Two points: iteration 1 (uniform(-1, 1) factors: about half of every warm
start set is wrong) and iteration 10 (after nine NNLS iterations: the warm
start is the previous iteration's support).  Per point and side: the Cholesky
solve, the NNLS solve, the NNLS solve cut at one round per entity
(set_nnls(max_rounds=1): what a perfect start would cost), and the histogram
of rounds per entity from nnls_rounds (index = rounds; index 0 = entities that
are not positive definite, here the ones without ratings).
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


def solve_ms(ctx, U, V, reps):
    """Median MR_K_SOLVE time of the users and the items half-step of one
    iteration from (U, V), the first repetition dropped as a warm-up."""
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
    return {s: round(float(np.median(v)), 4) for s, v in ms.items()}


def point(ctx, U, V, reps):
    out = {}
    ctx.set_solver("cholesky")
    out["cholesky_ms"] = solve_ms(ctx, U, V, reps)
    ctx.set_solver("nnls")
    ctx.set_nnls(0, True)
    out["nnls_ms"] = solve_ms(ctx, U, V, reps)
    ctx.set_factors(U, V)
    for side in SIDES:          # the same iteration once more, for its rounds
        ctx.half_step(side)
        r = ctx.nnls_rounds(side)
        st = ctx.nnls_stats(side)
        out["rounds_" + side] = {
            "histogram": np.bincount(np.abs(r)).tolist(), "unconverged": st["unconverged"],
            "mean": round(st["rounds_total"] / max(1, int(np.sum(r != 0))), 3),
            "max": st["rounds_max"]}
    ctx.set_nnls(1, True)
    out["nnls_one_round_ms"] = solve_ms(ctx, U, V, reps)
    ctx.set_nnls(0, True)
    for side in SIDES:
        c = out["cholesky_ms"][side]
        out["ratio_" + side] = {"nnls/cholesky": round(out["nnls_ms"][side] / c, 2),
                                "one_round/cholesky": round(out["nnls_one_round_ms"][side] / c, 2)}
    return out


def run(a, k):
    rs = load(a.shape, k)
    rng = np.random.RandomState(0)
    U0 = rng.uniform(-1, 1, rs.num_users * (k + 1))
    V0 = rng.uniform(-1, 1, rs.num_items * k)
    out = {"k": k, "N": int(rs.n), "users": rs.num_users, "items": rs.num_items,
           "lambda": a.reg, "reg_mode": "weighted", "note": "ms per solve launch (MR_K_SOLVE)"}
    with AlsContext(rs.user_ids, rs.item_ids, rs.ratings, k, rs.num_users, rs.num_items,
                    solver="nnls", reg=a.reg, reg_mode="weighted", timing=True) as ctx:
        out["iteration_1"] = point(ctx, U0, V0, a.reps)
        ctx.set_solver("nnls")
        ctx.set_factors(U0, V0)
        history = []
        for _ in range(9):
            ctx.iterate(1)
            history.append(round(ctx.objective()["J"], 1))
        U9, V9 = ctx.get_factors()
        out["J_after_iterations_1_to_9"] = history
        out["zero_share_users_items"] = [
            round(float(np.mean(U9.reshape(-1, k + 1)[:, :k] == 0.0)), 3),
            round(float(np.mean(V9 == 0.0)), 3)]
        out["iteration_10"] = point(ctx, U9, V9, a.reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--shape", default="ml-full")
    ap.add_argument("--reg", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    for k in a.k:
        print(json.dumps(run(a, k)), flush=True)


if __name__ == "__main__":
    main()
