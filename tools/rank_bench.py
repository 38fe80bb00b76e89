"""Kernel times of the ranking evaluation and the implicit fold-in (DESIGN.md
"Ranking evaluation and implicit fold-in"): the ML-full-shape synthetic at
k = 64 with a 20 % held-out split, HIP-event time per kernel class from
mr_rank_counts' kernel_ms.

  python tools/rank_bench.py [--k 64] [--users 65536] [--reps 3]

* the tile-count kernel for the first B users beside
  MovieTable.kernel_ms()["scores"] (the K-S1 score kernel of top_n, which
  forms the same B x I fp64 scores and stores them) in the same process;
* fold-in users per second at list lengths 20 and 200 (wall clock around
  the call: upload, Y^T Y, the per-user solve and the read-back).

The factors are seeded uniform(-1, 1): the times do not depend on the values.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from movie_recommender_amd import _lib, implicit, ranking, synth
from movie_recommender_amd.serving import MovieTable


def load(shape, k):
    """(user ids, item ids, users, items) of the bench workload, cached."""
    cache = f"/tmp/mr_rank_bench_{shape}_k{k}_{synth.DATA_SEED}.npz"
    if os.path.exists(cache):
        d = np.load(cache)
        return d["u"], d["i"], int(d["nu"]), int(d["ni"])
    rs = synth.movielens_like(shape, k)
    np.savez(cache, u=rs.user_ids, i=rs.item_ids, nu=rs.num_users, ni=rs.num_items)
    return rs.user_ids, rs.item_ids, rs.num_users, rs.num_items


def best(reps, fn):
    out = [fn() for _ in range(reps)]
    return out[int(np.argmin([o[0] for o in out]))]


def run_counts(a):
    uid, iid, nu, ni = load(a.shape, a.k)
    B = min(a.users, nu)
    sel = uid < B
    u, i = uid[sel].astype(np.int64), iid[sel].astype(np.int64)
    held = np.random.default_rng(1).random(len(u)) < 0.2
    test, excl = (u[held], i[held]), (u[~held], i[~held])
    rng = np.random.default_rng(0)
    X, Y = rng.uniform(-1, 1, (B, a.k)), rng.uniform(-1, 1, (ni, a.k))
    out = {"k": a.k, "users": B, "items": ni, "test_pairs": int(held.sum()),
           "excluded_pairs": int((~held).sum()),
           "pairs_per_tile": round(float(held.sum()) / ((B + 31) // 32), 1)}

    def counts():
        c = ranking.rank_counts(X, Y, test, excl)
        return c["kernel_ms"]["tile_counts"], c
    counts()                                             # warm-up
    t0 = time.perf_counter()
    ms, c = best(a.reps, counts)
    out["rank_counts_kernel_ms"] = {n: round(v, 3) for n, v in c["kernel_ms"].items()}
    out["rank_counts_wall_s_per_call"] = round((time.perf_counter() - t0) / a.reps, 3)
    out["mpr_of_random_factors"] = round(
        ranking.metrics_from_counts(c, test[0])["mpr"], 4)
    for name, tuning in (("one_block_per_item_tile", (0, 65535, 0)),
                         ("one_item_group", (0, 1, 0)),
                         ("compare_path_only", (0, 0, -1))):
        _lib.check(_lib.lib().mr_rank_set_tuning(*tuning), "tuning")
        try:
            counts()
            ms_v, c_v = best(a.reps, counts)
        finally:
            _lib.check(_lib.lib().mr_rank_set_tuning(0, 0, 0), "tuning")
        assert all(np.array_equal(c_v[n], c[n]) for n in ("above", "tied", "tied_before"))
        out["tile_counts_ms_" + name] = round(ms_v, 3)
    # one held-out pair per 32-user tile: the count kernel's score part alone
    order = np.argsort(test[0], kind="stable")
    first = np.flatnonzero(np.diff(np.concatenate([[-1], test[0][order] // 32])) != 0)
    sparse = (test[0][order][first], test[1][order][first])

    def score_part():
        return ranking.rank_counts(X, Y, sparse, excl)["kernel_ms"]["tile_counts"], None
    score_part()
    out["tile_counts_ms_one_pair_per_tile"] = round(best(a.reps, score_part)[0], 3)
    out["pairs_in_that_run"] = int(len(first))
    # the yardstick: the score kernel of top_n on the same B x I (it also
    # stores the keys; mr_rec_scores would add 8 B x I bytes of host copy)
    if a.k <= 128:
        ids = {m: m for m in range(ni)}
        with MovieTable(a.k, Y.reshape(-1), ids, dict.fromkeys(ids, 0.0)) as table:
            Xb = np.concatenate([X, np.zeros((B, 1))], axis=1)

            def scores():
                table.top_n_arrays(Xb, None, 10)
                return table.kernel_ms()["scores"], table.kernel_ms()
            scores()
            ms_s, all_ms = best(a.reps, scores)
        out["score_kernel_ms"] = round(ms_s, 3)
        out["top_n_kernel_ms"] = {n: round(v, 3) for n, v in all_ms.items() if v}
        out["tile_counts_over_scores"] = round(ms / ms_s, 3)
    flop = 2.0 * B * ni * a.k
    out["tile_counts_fp64_tflops"] = round(flop / (ms * 1e-3) / 1e12, 2)
    return out


def run_fold_in(a):
    uid, iid, nu, ni = load(a.shape, a.k)
    rng = np.random.default_rng(2)
    Y = rng.uniform(-1, 1, (ni, a.k))
    out = {"k": a.k, "items": ni, "fold_in_users": a.fold_users}
    for M in (20, 200):
        off = np.arange(a.fold_users + 1, dtype=np.int64) * M
        items = rng.integers(0, ni, a.fold_users * M)
        r = rng.integers(1, 11, a.fold_users * M) * 0.5

        def fold():
            t0 = time.perf_counter()
            _, status = implicit.fold_in(Y, (off, items, r), alpha=8.0, reg=0.5)
            assert np.all(status == 1)
            return time.perf_counter() - t0, None
        fold()
        s, _ = best(a.reps, fold)
        out[f"fold_in_M{M}_users_per_s"] = round(a.fold_users / s)
        out[f"fold_in_M{M}_wall_s"] = round(s, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--shape", default="ml-full")
    ap.add_argument("--users", type=int, default=65536)
    ap.add_argument("--fold-users", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    print(json.dumps(run_counts(a)), flush=True)
    print(json.dumps(run_fold_in(a)), flush=True)


if __name__ == "__main__":
    main()
