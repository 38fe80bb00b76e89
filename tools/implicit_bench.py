"""Per-class kernel times of one implicit-feedback ALS iteration beside one
explicit iteration (DESIGN.md "Implicit feedback"): the ML-full-shape
synthetic with its ratings shifted back to the half-star set {0.5 .. 5} (so
they are >= 0), the same lambda and solver, the same process and context.
HIP-event times from the engine's own timing (mr_stats).

  python tools/implicit_bench.py [--k 64 128] [--alpha 1.0] [--reps 3]

The implicit mode adds no timing class: its weighted kernel is booked as the
side's Gram, the global Gram S and the add pass as one "regularize" entry per
half-step (then the ridge pass as another).  `rocprofv3 --kernel-trace --stats`
over this script separates them by kernel name (wnormal_kernel,
yty_partial_kernel + yty_combine_kernel, add_s_kernel).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from movie_recommender_amd import synth
from movie_recommender_amd.engine import AlsContext
from reg_bench import HBM_MEASURED


def load(shape, k):
    """(user ids, item ids, half-star ratings, users, items): the bench
    workload with the per-movie median added back."""
    cache = f"/tmp/mr_implicit_bench_{shape}_k{k}_{synth.DATA_SEED}.npz"
    if os.path.exists(cache):
        d = np.load(cache)
        return d["u"], d["i"], d["r"], int(d["nu"]), int(d["ni"])
    rs = synth.movielens_like(shape, k)
    stars = np.round(2.0 * (rs.ratings + rs.medians[rs.item_ids])) / 2.0
    np.savez(cache, u=rs.user_ids, i=rs.item_ids, r=stars, nu=rs.num_users, ni=rs.num_items)
    return rs.user_ids, rs.item_ids, stars, rs.num_users, rs.num_items


def gsize_of(k):
    nb = (k + 15) // 16
    return (nb * (nb - 1) // 2 + nb // 2 + (nb & 1)) * 256 + (nb // 2) * 16


def per_launch(st):
    return {name: round(st["kernel_ms"][name] / n, 4)
            for name, n in st["kernel_launches"].items() if n}


def run(a, k):
    uid, iid, stars, nu, ni = load(a.shape, k)
    assert stars.min() >= 0.5 and stars.max() <= 5.0
    rng = np.random.RandomState(0)
    U0 = rng.uniform(-1, 1, nu * (k + 1))
    V0 = rng.uniform(-1, 1, ni * k)
    out = {"k": k, "N": len(stars), "users": nu, "items": ni,
           "lambda": a.reg, "reg_mode": a.reg_mode, "solver": a.solver, "alpha": a.alpha,
           "note": "ms per launch; 'regularize' under implicit averages the (S + add pass) "
                   "entry and the ridge entry of a half-step"}
    with AlsContext(uid, iid, stars, k, nu, ni,
                    solver=a.solver, reg=a.reg, reg_mode=a.reg_mode, timing=True) as ctx:
        for name, alpha in (("explicit", 0.0), ("implicit", a.alpha)):
            ctx.set_implicit(alpha)
            ctx.set_factors(U0, V0)
            ctx.iterate(1)                      # warm-up
            ctx.set_factors(U0, V0)
            ctx.reset_stats()
            ctx.iterate(a.reps)
            st = ctx.stats()
            rec = {"ms_per_launch": per_launch(st),
                   "launches_per_iteration": {n: v / a.reps
                                              for n, v in st["kernel_launches"].items() if v},
                   "phase_ms_per_iteration": {p: round(v / a.reps, 4)
                                              for p, v in st["phase_ms"].items()},
                   "cg_per_iteration": [st["cg_users_total"] / a.reps,
                                        st["cg_items_total"] / a.reps]}
            out[name] = rec
        # S + add pass alone: normal equations without the ridge
        ctx.set_regularization(0.0, a.reg_mode)
        for side, E in (("users", nu), ("items", ni)):
            ctx.build_normal_equations(side)    # warm-up
            ctx.reset_stats()
            for _ in range(a.reps):
                ctx.build_normal_equations(side)
            st = ctx.stats()
            floor = 2 * E * gsize_of(k) * 4
            out["s_plus_add_" + side] = {
                "ms": round(st["kernel_ms"]["regularize"] / st["kernel_launches"]["regularize"], 4),
                "wnormal_ms": round(st["kernel_ms"]["gram_" + side] /
                                    st["kernel_launches"]["gram_" + side], 4),
                "add_floor_MB": round(floor / 1e6, 1),
                "add_floor_ms_at_6.29TBs": round(floor / HBM_MEASURED * 1e3, 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--shape", default="ml-full")
    ap.add_argument("--alpha", type=float, default=1.0)
    ap.add_argument("--reg", type=float, default=0.05)
    ap.add_argument("--reg-mode", default="weighted")
    ap.add_argument("--solver", default="cg")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    for k in a.k:
        print(json.dumps(run(a, k)), flush=True)


if __name__ == "__main__":
    main()
