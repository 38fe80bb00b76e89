"""Content-model rates (DESIGN.md "Content model"): fits per second of
TagTable.fit and top-N users per second of TagTable.top_n at the reference's
shape -- 53,889 movies with a median, 14,529 tags, 19 genres -- on rating
lists with the lengths of ``synth.movielens_like("ml-full")``; beside them the
wall time of the tests' NumPy restatement on a sample of the same lists.

  python tools/tagls_bench.py [--users 65536] [--top-users 2048] [--cpu-lists 64]
                              [--scale 1.0] [--reps 2] [--out FILE]

Wall clock around each call (upload, kernels, read-back), best of --reps after
a warm-up; the kernel classes' own milliseconds beside it.  Movie features are
synthetic: 1-4 genres per movie, tags on 45 % of the movies with Zipf
popularity; tag ids spread up to 66,814.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
from movie_recommender_amd import synth  # noqa: E402
from movie_recommender_amd.content import TagFit, TagTable  # noqa: E402

N_MOVIES, N_TAGS, N_GENRES = 53_889, 14_529, 19


def movie_data(rng):
    tids = np.sort(rng.choice(np.arange(1, 66_814), N_TAGS - 1, replace=False)).tolist() + [66_814]
    zipf = 1.0 / np.arange(1, N_TAGS + 1)
    zipf /= zipf.sum()
    genres, raw = {}, {}
    has_tags = rng.random(N_MOVIES) < 0.45
    n_tags = rng.integers(1, 30, N_MOVIES)
    draws = rng.choice(N_TAGS, int(n_tags[has_tags].sum()), p=zipf)
    pos = 0
    for m in range(1, N_MOVIES + 1):
        genres[m] = set(rng.choice(N_GENRES, rng.integers(1, 5), replace=False).tolist())
        if has_tags[m - 1]:
            ts = np.unique(draws[pos:pos + n_tags[m - 1]])
            pos += n_tags[m - 1]
            raw[m] = {tids[t]: int(c) for t, c in zip(ts, rng.integers(1, 40, len(ts)))}
    counts = {}
    for d in raw.values():
        for t, c in d.items():
            counts[t] = counts.get(t, 0) + c
    tags = {m: {t: float(np.log(c) + 1) for t, c in d.items()} for m, d in raw.items()}
    med = {m: float(v) for m, v in zip(range(1, N_MOVIES + 1), rng.integers(1, 11, N_MOVIES) / 2)}
    return genres, tags, counts, med


def best(reps, fn):
    fn()                                                   # warm-up
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = fn()
        out.append((time.perf_counter() - t0, res))
    return min(out, key=lambda o: o[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=65536)
    ap.add_argument("--top-users", type=int, default=2048)
    ap.add_argument("--cpu-lists", type=int, default=64)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    rng = np.random.default_rng(14)
    rs = synth.movielens_like("ml-full", scale=a.scale)
    order = np.argsort(rs.user_ids, kind="stable")
    deg = np.bincount(rs.user_ids, minlength=rs.num_users)
    start = np.concatenate([[0], np.cumsum(deg)])
    users = np.nonzero(deg >= 2)[0][:a.users]
    off = np.concatenate([[0], np.cumsum(deg[users])]).astype(np.int64)
    pos = np.concatenate([order[start[u]:start[u + 1]] for u in users])
    mids = rs.item_ids[pos].astype(np.int64) % N_MOVIES + 1
    ratings = rng.integers(1, 11, len(mids)) / 2.0
    genres, tags, counts, med = movie_data(rng)
    out = {"users": len(users), "ratings": int(off[-1]), "movies": N_MOVIES, "tags": N_TAGS,
           "list_len_mean": float(deg[users].mean()), "list_len_max": int(deg[users].max())}
    with TagTable(genres, tags, counts, med) as t:
        s, fit = best(a.reps, lambda: t.fit((off, mids, ratings)))
        out.update(fit_wall_s=round(s, 4), fits_per_s=round(len(users) / s),
                   fit_kernel_ms={k: round(v, 3) for k, v in t.kernel_ms().items()
                                  if k in ("profile", "fit")},
                   itn_mean=float(fit.itn.mean()), itn_max=int(fit.itn.max()),
                   istop_histogram={int(v): int(n) for v, n in
                                    zip(*np.unique(fit.istop, return_counts=True))})
        nt = min(a.top_users, len(users))
        sub = TagFit(fit.p[:nt], fit.profile[:nt], fit.x[:nt])
        rated = (off[:nt + 1].copy(), mids[:off[nt]])
        s, _ = best(a.reps, lambda: t.top_n_arrays(sub, rated, 400))
        out.update(top_n_users=nt, top_n_wall_s=round(s, 4), top_n_users_per_s=round(nt / s),
                   top_n_kernel_ms={k: round(v, 3) for k, v in t.kernel_ms().items()
                                    if k in ("scores", "exclude", "select")})
    # the tests' NumPy restatement on a sample of the same lists (fit only)
    import content_cases as C
    d = dict(movie_genres=genres, movie_tags=tags, tag_counts=counts, med=med)
    nc = min(a.cpu_lists, len(users))
    lists = [list(zip(mids[off[u]:off[u + 1]].tolist(), ratings[off[u]:off[u + 1]].tolist()))
             for u in range(nc)]
    t0 = time.perf_counter()
    for l in lists:
        C.CpuModel(l, d)
    s = time.perf_counter() - t0
    out.update(numpy_lists=nc, numpy_wall_s=round(s, 4), numpy_fits_per_s=round(nc / s, 1))
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
