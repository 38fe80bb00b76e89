"""Golden fixture for the tag-count model, generated from the REFERENCE's own
Python code.

Run in the build container (needs /root/reference; writes nothing there):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_tagcount.py

Imported from the reference (plain NumPy/SciPy modules, no data files read):
  * ``python/app_local/models.py``  -- ``TagCount_UserProfile``: profiles, the
    two ``numpy.linalg.lstsq`` solves and ``predict``.  The module's
    ``numpy.linalg.lstsq`` is wrapped to capture (A, b) and the full return of
    every solve;
  * ``python/full_data/my_util.py`` -- ``compute_ranking_agreement``.

The movie data is content_small.npz's (tests/content_cases.py) plus
genre_counts = movies per genre (gc_*).

Fixture  tagcount_small.npz
  lists         CSR (l_off, l_mid, l_r) with a name each (l_name)
  per list      the reference's tag_profile (tp_*: tag id, value, keys in
                  insertion order, zero members included) and genre_profile
                  (gp_*); row_td / row_gd: the dot products of every rating's
                  movie; n0, has0, has1, x0_ref, x1_ref, rank0, rank1
                s_u0 / s_u1: largest |x_perm - x_ref|_inf / max(1, |x_ref|_inf)
                  over 16 row permutations of (A, b) through lstsq
                rank_stable0 / 1: all 16 permutations report the reference's
                  rank and the singular values on either side of the cut are
                  at least 2^10 away from it
                scores of every candidate, the top-60 list (rec_*), and for
                  the lists of PARAM_LISTS get_param_list (par_*)
  test lists    (t_off, t_mid, t_r) with the reference agreement (nan = None)
                and pair counts; a test list with a counted pair whose order
                could flip inside the score rounding bound is redrawn
The generator asserts that the NumPy restatement of tests/tagcount_cases.py
meets every rule on this fixture, and prints the measured spread.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = "/root/reference/python"
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(REF, "app_local"))
import models as ref_models  # noqa: E402  (reference: app_local/models.py)
sys.path.pop(0)
sys.path.insert(0, os.path.join(REF, "full_data"))
import my_util as ref_util  # noqa: E402  (reference: full_data/my_util.py)
sys.path.pop(0)

import content_cases as C  # noqa: E402
import tagcount_cases as T  # noqa: E402

SEED = 24
HALF = np.arange(1, 11) / 2.0
SIZES = [0, 1, 2, 3, 4, 63, 64, 65, 129, 600]
N_VAR = 16
TOP = 60
PARAM_LISTS = ("len65_0", "all_three", "len1_0")

captured = []
_lstsq = np.linalg.lstsq


class _Spy:
    """Stands in for the ``numpy.linalg`` the reference module sees."""

    @staticmethod
    def lstsq(A, b, rcond=None):
        r = _lstsq(A, b, rcond=rcond)
        captured.append((np.array(A, np.float64), np.array(b, np.float64).reshape(-1), r))
        return r


class _NumpySpy:
    linalg = _Spy

    def __getattr__(self, name):
        return getattr(np, name)


ref_models.numpy = _NumpySpy()


def ref_model(d, lst):
    captured.clear()
    return ref_models.TagCount_UserProfile(d["movie_genres"], lst, d["movie_tags"],
                                           d["tag_counts"], d["genre_counts"], d["med"],
                                           d["genre_names"], d["tag_names"])


def draw_until(rs, d, make, accept, what):
    for _ in range(4000):
        lst = make()
        if accept(ref_model(d, lst), lst):
            return lst
    raise RuntimeError("no list found for " + what)


def ref_rows(model, lst, d):
    return [(model._dot_product_with_movie_tag_scores(d["movie_tags"][m])
             if m in d["movie_tags"] else 0,
             model._dot_product_with_movie_genre_ids(d["movie_genres"][m])
             if m in d["movie_genres"] else 0) for m, _ in lst]


def rating_lists(rs, d):
    med, tags, genres = d["med"], d["movie_tags"], d["movie_genres"]
    pool = np.array(list(med))
    tagged = np.array([m for m in med if m in tags])
    untagged = np.array([m for m in med if m not in tags])
    genreless = np.array([m for m in med if m not in genres])
    rate = lambda ms: [(int(m), float(rs.choice(HALF))) for m in ms]   # noqa: E731
    n0_of = lambda mod, lst: sum(td > 0.1 for td, _ in ref_rows(mod, lst, d))   # noqa: E731
    lists, names = [], []
    for rep in range(2):
        for n in SIZES:
            lists.append(rate(rs.choice(pool, n, replace=False)))
            names.append(f"len{n}_{rep}")
    lists.append([(int(m), 3.0) for m in rs.choice(pool, 12, replace=False)])
    names.append("all_three")
    lists.append(rate(rs.choice(untagged, 10, replace=False)))
    names.append("untagged_only")
    lists.append(rate(rs.choice(genreless, 10, replace=False)))
    names.append("genreless_only")
    mixed = lambda: rate(list(rs.choice(untagged, 5, replace=False))       # noqa: E731
                         + list(rs.choice(tagged, 4, replace=False)))
    lists.append(draw_until(rs, d, mixed, lambda mod, l: n0_of(mod, l) == 2, "A0 of 2 rows"))
    names.append("a0_two_rows")
    lists.append(draw_until(rs, d, mixed, lambda mod, l: n0_of(mod, l) == 3, "A0 of 3 rows"))
    names.append("a0_three_rows")

    def threshold_ok(mod, l):
        tds = [td for td, _ in ref_rows(mod, l, d)]
        return (any(td < -0.1 for td in tds) and any(1e-6 < td <= 0.1 for td in tds)
                and mod.x_factors0 is not None)
    lists.append(draw_until(rs, d, lambda: rate(rs.choice(pool, 30, replace=False)), threshold_ok,
                            "fit threshold"))
    names.append("fit_threshold")

    def cancelling():
        x = int(rs.choice(tagged))
        rest = [m for m in rs.choice(pool, 8, replace=False) if m != x]
        return [(x, 5.0)] + rate(rest) + [(x, 1.0)]
    lists.append(draw_until(rs, d, cancelling,
                            lambda mod, l: any(v == 0 for v in mod.tag_profile.values()),
                            "cancelling offsets"))
    names.append("cancelling")
    base = list(rs.choice(tagged, 9, replace=False))
    lists.append(rate(base[:5]) + [(int(base[0]), 4.5)] + rate(base[5:]) + [(int(base[0]), 2.0)])
    names.append("repeated_movie")
    # every movie has the same genre set and no tags: a constant, nonzero genre product
    sets = {}
    for m in med:
        if m in genres and m not in tags:
            sets.setdefault(frozenset(genres[m]), []).append(m)
    same = max(sets.values(), key=len)
    assert len(same) >= 4
    lists.append([(int(m), r) for m, r in zip(same[:4], (5.0, 4.0, 1.5, 4.5))])
    names.append("const_genre")
    return lists, names


def spread_and_stability(rs, A, b, res):
    """(s_u, rank_stable) of one captured solve."""
    x_ref, rank, s = res[0].reshape(-1), int(res[2]), res[3]
    cut = T.EPS * max(A.shape) * s[0]
    stable = all(v > cut * 2.0 ** 10 for v in s[:rank]) and all(v * 2.0 ** 10 <= cut
                                                                for v in s[rank:])
    spread = 0.0
    for _ in range(N_VAR):
        pm = rs.permutation(len(b))
        r = _lstsq(A[pm], b[pm], rcond=None)
        spread = max(spread, C.rel_inf(r[0], x_ref))
        stable = stable and int(r[2]) == rank
    return spread, stable


def main():
    rs = np.random.RandomState(SEED)
    d = T.movie_data()
    d["genre_names"] = {f"genre{g}": g for g in d["genre_counts"]}
    d["tag_names"] = {f"tag{t}": t for t in d["tag_counts"]}
    lists, names = rating_lists(rs, d)
    med_keys = d["med_keys"]
    all_mids = np.array(sorted(set(d["movie_genres"]) | set(d["movie_tags"]) | set(d["med"])))
    B = len(lists)
    x0_ref, x1_ref = np.zeros((B, 3)), np.zeros((B, 2))
    ints = {k: np.zeros(B, np.int32) for k in ("n0", "has0", "has1", "rank0", "rank1",
                                                "rank_stable0", "rank_stable1")}
    s_u0, s_u1 = np.zeros(B), np.zeros(B)
    scores = np.zeros((B, len(med_keys)))
    tp_off, tp_tid, tp_val, gp_off, gp_gid, gp_val = [0], [], [], [0], [], []
    row_td, row_gd = [], []
    rec_off, rec_mid, rec_score = [0], [], []
    par_off, par_name, par_val = [0], [], []
    t_lists, agreement, n_agree, n_dis = [], [], [], []
    models = []
    for u, lst in enumerate(lists):
        model = ref_model(d, lst)
        solves = list(captured)
        rows = ref_rows(model, lst, d)
        row_td += [float(td) for td, _ in rows]
        row_gd += [float(gd) for _, gd in rows]
        ints["n0"][u] = sum(td > 0.1 for td, _ in rows)
        assert (model.x_factors0 is not None) == (ints["n0"][u] >= 3)
        assert (model.x_factors1 is not None) == (len(lst) >= 2)
        assert len(solves) == int(ints["n0"][u] >= 3) + int(len(lst) >= 2)
        if model.x_factors0 is not None:
            A, b, res = solves[0]
            x0_ref[u], ints["has0"][u], ints["rank0"][u] = res[0].reshape(-1), 1, res[2]
            s_u0[u], ints["rank_stable0"][u] = spread_and_stability(rs, A, b, res)
        if model.x_factors1 is not None:
            A, b, res = solves[-1]
            x1_ref[u], ints["has1"][u], ints["rank1"][u] = res[0].reshape(-1), 1, res[2]
            s_u1[u], ints["rank_stable1"][u] = spread_and_stability(rs, A, b, res)
        tp_tid += list(model.tag_profile)
        tp_val += [float(v) for v in model.tag_profile.values()]
        tp_off.append(len(tp_tid))
        gp_gid += list(model.genre_profile)
        gp_val += [float(v) for v in model.genre_profile.values()]
        gp_off.append(len(gp_gid))
        sc = np.array([model.predict(int(m)) for m in med_keys], np.float64)
        scores[u] = sc
        rated = dict(lst)
        top = sorted(((float(s), int(m)) for s, m in zip(sc, med_keys) if int(m) not in rated),
                     reverse=True)[:TOP]
        rec_mid += [m for _, m in top]
        rec_score += [s for s, _ in top]
        rec_off.append(len(rec_mid))
        if names[u] in PARAM_LISTS:
            for n, v in model.get_param_list():
                par_name.append(f"{n}:{v}" if n == "__comment" else n)
                par_val.append(np.nan if n == "__comment" else float(v))
        par_off.append(len(par_name))
        mdl = (model.tag_profile, model.genre_profile, model.x_factors0, model.x_factors1)
        models.append(mdl)
        # held-out list: some movies without a median; no counted pair inside the rounding
        # bound (equal keys tie in any implementation, and so do two exact medians)
        _, bnd, keys = T.exact_scores(mdl, d)
        bound = dict(zip(med_keys.tolist(), bnd.tolist()))
        same = dict(zip(med_keys.tolist(), keys))
        for _ in range(40):
            tl = [(int(m), float(rs.choice(HALF))) for m in rs.choice(all_mids, 25, replace=False)]
            kept = [(m, a) for m, a in tl if model.predict(m) is not None]
            pred = [(m, float(model.predict(m))) for m, _ in kept]
            safe = all(ai == aj or same[mi] == same[mj] or abs(pi - pj) > bound[mi] + bound[mj]
                       or bound[mi] == bound[mj] == 0.0
                       for (mi, ai), (_, pi) in zip(kept, pred)
                       for (mj, aj), (_, pj) in zip(kept, pred))
            if safe:
                break
        else:
            raise RuntimeError("no safe test list for " + names[u])
        val = ref_util.compute_ranking_agreement(kept, pred) if len(pred) > 1 else None
        _, ag, dg = C.agreement_counts([a for _, a in kept], np.array([q for _, q in pred]))
        assert val is None or val == ag / (ag + dg)
        t_lists.append(tl)
        agreement.append(np.nan if val is None else val)
        n_agree.append(ag if val is not None else 0)
        n_dis.append(dg if val is not None else 0)

    # the lists the kernels can go wrong on are what they claim to be
    at = names.index
    assert ints["n0"][at("a0_two_rows")] == 2 and not ints["has0"][at("a0_two_rows")]
    assert ints["n0"][at("a0_three_rows")] == 3 and ints["has0"][at("a0_three_rows")]
    u = at("all_three")
    assert not models[u][0] and not models[u][1] and not ints["has0"][u] and ints["rank1"][u] == 1
    assert not models[at("untagged_only")][0] and not models[at("genreless_only")][1]
    assert any(v == 0 for v in models[at("cancelling")][0].values())
    u = at("const_genre")
    assert len({gd for gd in row_gd[sum(map(len, lists[:u])):][:4]}) == 1 and row_gd[
        sum(map(len, lists[:u]))] != 0

    # the restatement must meet every rule on this fixture
    e0, e1 = [], []
    for u, lst in enumerate(lists):
        m = T.CpuModel(lst, d)
        tp, gp = models[u][0], models[u][1]
        assert list(m.tag_profile.items()) == list(tp.items()), names[u]
        assert list(m.genre_profile.items()) == list(gp.items()), names[u]
        a = sum(map(len, lists[:u]))
        assert [float(td) for td, _ in m.rows] == row_td[a:a + len(lst)], names[u]
        assert [float(gd) for _, gd in m.rows] == row_gd[a:a + len(lst)], names[u]
        assert m.n0 == ints["n0"][u] and (m.x0 is not None) == bool(ints["has0"][u])
        assert (m.x1 is not None) == bool(ints["has1"][u])
        if m.x0 is not None:
            e0.append(C.rel_inf(m.x0, x0_ref[u]))
            assert not ints["rank_stable0"][u] or m.rank0 == ints["rank0"][u], names[u]
        if m.x1 is not None:
            e1.append(C.rel_inf(m.x1, x1_ref[u]))
            assert not ints["rank_stable1"][u] or m.rank1 == ints["rank1"][u], names[u]
        s, bnd, _ = T.exact_scores(models[u], d)
        assert np.all(np.abs(s - scores[u]) <= bnd), names[u]
    r0 = T.spread_report(e0, s_u0[ints["has0"] == 1])
    r1 = T.spread_report(e1, s_u1[ints["has1"] == 1])
    print(f"lists {B}; x0 on {len(e0)} (rank stable {int(ints['rank_stable0'].sum())}), "
          f"x1 on {len(e1)} (rank stable {int(ints['rank_stable1'].sum())}); "
          f"max s_u {max(s_u0.max(), s_u1.max()):.3e}; restatement worst e_u / max(s_u, 2^-40): "
          f"x0 {r0['worst_ratio']:.3g} (over their own bound {r0['over']}), "
          f"x1 {r1['worst_ratio']:.3g} (over {r1['over']})")

    l_off = np.zeros(B + 1, np.int64)
    l_off[1:] = np.cumsum([len(l) for l in lists])
    t_off = np.zeros(B + 1, np.int64)
    t_off[1:] = np.cumsum([len(l) for l in t_lists])
    out = dict(
        gc_gid=np.array(list(d["genre_counts"]), np.int64),
        gc_cnt=np.array(list(d["genre_counts"].values()), np.int64), l_off=l_off,
        l_mid=np.array([m for l in lists for m, _ in l], np.int64),
        l_r=np.array([r for l in lists for _, r in l], np.float64), l_name=np.array(names),
        tp_off=np.array(tp_off, np.int64), tp_tid=np.array(tp_tid, np.int64),
        tp_val=np.array(tp_val, np.float64), gp_off=np.array(gp_off, np.int64),
        gp_gid=np.array(gp_gid, np.int64), gp_val=np.array(gp_val, np.float64),
        row_td=np.array(row_td, np.float64), row_gd=np.array(row_gd, np.float64),
        x0_ref=x0_ref, x1_ref=x1_ref, s_u0=s_u0, s_u1=s_u1, scores=scores,
        rec_off=np.array(rec_off, np.int64), rec_mid=np.array(rec_mid, np.int64),
        rec_score=np.array(rec_score, np.float64), par_off=np.array(par_off, np.int64),
        par_name=np.array(par_name), par_val=np.array(par_val, np.float64), t_off=t_off,
        t_mid=np.array([m for l in t_lists for m, _ in l], np.int64),
        t_r=np.array([r for l in t_lists for _, r in l], np.float64),
        agreement=np.array(agreement), n_agree=np.array(n_agree, np.int64),
        n_disagree=np.array(n_dis, np.int64), seed=SEED, numpy=np.__version__, **ints)
    path = os.path.join(HERE, "tagcount_small.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
