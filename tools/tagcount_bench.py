"""Tag-count model rates (DESIGN.md "Content model: tag counting"): fits per
second of TagCountTable.fit and top-N users per second of
TagCountTable.top_n_arrays at an ML-full-like table -- 53,889 movies with a
median, 19 genres, 14,529 distinct tags, tags on 45 % of the movies, 1 to 29
Zipf-popular draws each (the synthetic table of tools/tagls_bench.py) -- on
rating lists with the lengths of ``synth.movielens_like("ml-full")``; beside
them the wall time of the tests' NumPy restatement on a sample of the same
lists.

  python tools/tagcount_bench.py [--users 65536] [--top-users 2048] [--cpu-lists 64]
                                 [--cpu-top 4] [--scale 1.0] [--reps 2] [--out FILE]

Wall clock around each call (upload, kernels, read-back), best of --reps after
a warm-up; the kernel classes' own milliseconds beside it.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
from movie_recommender_amd import synth  # noqa: E402
from movie_recommender_amd.tagcount import TagCountFit, TagCountTable  # noqa: E402
from tagls_bench import N_GENRES, N_MOVIES, N_TAGS, best, movie_data  # noqa: E402


def sub_fit(table, fit, n):
    """The first n models of a fit."""
    e = fit.tp_off[n]
    return TagCountFit(table, fit.genre_dense[:n], fit.tp_off[:n + 1], fit.tp_idx[:e],
                       fit.tp_val[:e], fit.x0[:n], fit.x1[:n], fit.has0[:n], fit.has1[:n])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=65536)
    ap.add_argument("--top-users", type=int, default=2048)
    ap.add_argument("--cpu-lists", type=int, default=64)
    ap.add_argument("--cpu-top", type=int, default=4)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    rng = np.random.default_rng(14)
    rs = synth.movielens_like("ml-full", scale=a.scale)
    order = np.argsort(rs.user_ids, kind="stable")
    deg = np.bincount(rs.user_ids, minlength=rs.num_users)
    start = np.concatenate([[0], np.cumsum(deg)])
    users = np.nonzero(deg >= 1)[0][:a.users]
    off = np.concatenate([[0], np.cumsum(deg[users])]).astype(np.int64)
    pos = np.concatenate([order[start[u]:start[u + 1]] for u in users])
    mids = rs.item_ids[pos].astype(np.int64) % N_MOVIES + 1
    ratings = rng.integers(1, 11, len(mids)) / 2.0
    genres, tags, counts, med = movie_data(rng)
    genre_counts = {}
    for gs in genres.values():
        for g in gs:
            genre_counts[g] = genre_counts.get(g, 0) + 1
    print("lists and movie data ready", file=sys.stderr, flush=True)
    out = {"users": len(users), "ratings": int(off[-1]), "movies": N_MOVIES, "tags": N_TAGS,
           "genres": N_GENRES, "tag_entries": sum(len(d) for d in tags.values()),
           "list_len_mean": float(deg[users].mean()), "list_len_max": int(deg[users].max())}
    with TagCountTable(genres, tags, counts, genre_counts, med) as t:
        s, fit = best(a.reps, lambda: t.fit((off, mids, ratings)))
        out.update(fit_wall_s=round(s, 4), fits_per_s=round(len(users) / s),
                   fit_kernel_ms={k: round(v, 3) for k, v in t.kernel_ms().items()
                                  if k in ("profile", "fit", "compact")},
                   profile_entries=int(fit.tp_off[-1]), with_x0=int(fit.has0.sum()),
                   with_x1=int(fit.has1.sum()),
                   rank_histogram={f"{r0}/{r1}": int(n) for (r0, r1), n in zip(
                       *np.unique(np.stack([fit.rank0, fit.rank1], 1), axis=0,
                                  return_counts=True))})
        print("fit done", file=sys.stderr, flush=True)
        nt = min(a.top_users, len(users))
        sub = sub_fit(t, fit, nt)
        rated = (off[:nt + 1].copy(), mids[:off[nt]])
        s, _ = best(a.reps, lambda: t.top_n_arrays(sub, rated, 400))
        out.update(top_n_users=nt, top_n_wall_s=round(s, 4), top_n_users_per_s=round(nt / s),
                   top_n_kernel_ms={k: round(v, 3) for k, v in t.kernel_ms().items()
                                    if k in ("scatter", "scores", "exclude", "select")})
        few = sub_fit(t, fit, min(a.cpu_top, nt))
        gpu_scores = t.scores(few)
    print("top-N done", file=sys.stderr, flush=True)
    # the tests' NumPy restatement on a sample of the same lists
    import tagcount_cases as T
    d = dict(movie_genres=genres, movie_tags=tags, tag_counts=counts, genre_counts=genre_counts,
             med=med, med_keys=np.array(list(med)))
    nc = min(a.cpu_lists, len(users))
    lists = [list(zip(mids[off[u]:off[u + 1]].tolist(), ratings[off[u]:off[u + 1]].tolist()))
             for u in range(nc)]
    t0 = time.perf_counter()
    cpu = [T.CpuModel(l, d) for l in lists]
    s = time.perf_counter() - t0
    out.update(numpy_lists=nc, numpy_wall_s=round(s, 4), numpy_fits_per_s=round(nc / s, 1))
    t0 = time.perf_counter()
    same = True
    for u in range(len(few)):       # scores of the GPU's own models, restated
        sc = T.exact_scores((few.tag_profile(u), few.genre_profile(u), few.x_factors0(u),
                             few.x_factors1(u)), d)[0]
        same = same and bool(np.array_equal(sc, gpu_scores[u]))
    s = time.perf_counter() - t0
    out.update(numpy_score_users=len(few), numpy_score_wall_s=round(s, 4),
               numpy_score_users_per_s=round(len(few) / s, 2) if len(few) else None,
               scores_equal_restatement=same,
               profiles_equal_restatement=all(
                   fit.tag_profile(u) == {k: v for k, v in m.tag_profile.items() if v != 0}
                   and fit.n0[u] == m.n0 for u, m in enumerate(cpu)))
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
