"""Fold-in rates (DESIGN.md "Fold-in"): entities per second of mr_fold_in at
k = 64 and k = 128, 16,384 new entities with lists of M = 20 and M = 200
entries against a 20,000-row table, for the Cholesky and the non-negative
solve (with the histogram of its rounds), and mr_implicit_fold_in on the same
input beside them.

  python tools/foldin_bench.py [--ks 64 128] [--entities 16384] [--reps 3]

Wall clock around the call (upload, T^T T, the per-entity build and solve, the
read-back), best of --reps after a warm-up.  The table is |uniform(-1, 1)|, r
in {0.5, ..., 5}; the times of the Cholesky solve do not depend on the values,
the rounds of the non-negative solve do.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from movie_recommender_amd import foldin, implicit

ALPHA, REG = 8.0, 0.5


def best(reps, fn):
    fn()                                                   # warm-up
    out = [fn() for _ in range(reps)]
    return out[int(np.argmin([o[0] for o in out]))]


def run(k, M, a):
    rng = np.random.default_rng(k + M)
    T = np.abs(rng.uniform(-1, 1, (a.rows, k)))
    offs = rng.integers(1, 11, a.rows) * 0.25
    E = a.entities
    lists = (np.arange(E + 1, dtype=np.int64) * M, rng.integers(0, a.rows, E * M),
             rng.integers(1, 11, E * M) * 0.5)
    out = {"k": k, "M": M, "entities": E, "rows": a.rows}

    def timed(name, fn):
        def once():
            t0 = time.perf_counter()
            res = fn()
            return time.perf_counter() - t0, res
        s, res = best(a.reps, once)
        out[name + "_per_s"] = round(E / s)
        out[name + "_wall_s"] = round(s, 4)
        return res

    _, status = timed("implicit_old_entry", lambda: implicit.fold_in(T, lists, ALPHA, REG))
    assert np.all(status == 1)
    forms = {"implicit": dict(mode="implicit", alpha=ALPHA),
             "explicit_intercept": dict(mode="explicit", intercept=True, row_offset=offs)}
    for form, kw in forms.items():
        for nonneg in (False, True):
            name = form + ("_nnls" if nonneg else "_cholesky")
            _, status, rounds = timed(name, lambda: foldin.fold_in(
                T, lists, reg=REG, nonneg=nonneg, **kw))
            assert np.all(status == 1), name
            if nonneg:
                out[name + "_rounds_histogram"] = {
                    int(v): int(n) for v, n in zip(*np.unique(rounds, return_counts=True))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--entities", type=int, default=16384)
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    for k in a.ks:
        for M in (20, 200):
            print(json.dumps(run(k, M, a)), flush=True)


if __name__ == "__main__":
    main()
