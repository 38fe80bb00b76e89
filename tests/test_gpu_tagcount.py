"""GPU: the tag-count model against the reference's recorded results by the
rules of tests/tagcount_cases.py -- bit-equal profiles, row counts and model
flags, both coefficient vectors inside the reference's own rounding spread
with the reference's rank, and exact scores / top-N / agreement given the
reference's models -- plus batch independence and the paths that depend on
sizes."""
import numpy as np
import pytest

import content_cases as C
import tagcount_cases as T
from movie_recommender_amd.tagcount import (TagCount_UserProfile, TagCountFit, TagCountTable,
                                            median_eval, tag_count_eval)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return T.fixture()


def _table(d):
    return TagCountTable(d["movie_genres"], d["movie_tags"], d["tag_counts"], d["genre_counts"],
                         d["med"])


@pytest.fixture(scope="module")
def table(gpu, fx):
    with _table(fx) as t:
        yield t


@pytest.fixture(scope="module")
def fit_gpu(table, fx):
    return table.fit(fx["lists"])


@pytest.fixture(scope="module")
def fit_ref(table, fx):
    """The reference's models as the GPU takes them."""
    return TagCountFit.from_models(table, fx["ref_models"])


@pytest.fixture(scope="module")
def cpu_scores(fx):
    return [T.exact_scores(m, fx)[:2] for m in fx["ref_models"]]


def _nonzero(profile):
    return {k: v for k, v in profile.items() if v != 0}


def test_profiles_rows_and_flags_exact(fit_gpu, fx):
    for u, name in enumerate(fx["names"]):
        assert fit_gpu.tag_profile(u) == _nonzero(fx["tag_profiles"][u]), name
        assert fit_gpu.genre_profile(u) == _nonzero(fx["genre_profiles"][u]), name
        a, b = fit_gpu.tp_off[u], fit_gpu.tp_off[u + 1]
        assert np.all(np.diff(fit_gpu.tp_idx[a:b]) > 0), name
    assert np.array_equal(fit_gpu.n0, fx["n0"])
    assert np.array_equal(fit_gpu.has0, fx["has0"])
    assert np.array_equal(fit_gpu.has1, fx["has1"])
    u = fx["names"].index("all_three")
    assert fit_gpu.tp_off[u] == fit_gpu.tp_off[u + 1] and not fit_gpu.genre_dense[u].any()
    assert (fit_gpu.has0[u], fit_gpu.has1[u], fit_gpu.rank1[u]) == (0, 1, 1)
    u = fx["names"].index("cancelling")
    assert 0.0 in fx["tag_profiles"][u].values()       # the key is there, the value is exactly 0
    for u in np.nonzero(fx["has0"] == 0)[0]:
        assert not fit_gpu.x0[u].any() and fit_gpu.rank0[u] == 0
    for u in np.nonzero(fx["has1"] == 0)[0]:
        assert not fit_gpu.x1[u].any() and fit_gpu.rank1[u] == 0


def test_coefficients_inside_reference_spread(fit_gpu, fx):
    for x, ref, has, s_u, rank, rank_ref, stable in (
            (fit_gpu.x0, fx["x0_ref"], fx["has0"], fx["s_u0"], fit_gpu.rank0, fx["rank0"],
             fx["rank_stable0"]),
            (fit_gpu.x1, fx["x1_ref"], fx["has1"], fx["s_u1"], fit_gpu.rank1, fx["rank1"],
             fx["rank_stable1"])):
        on = np.nonzero(has)[0]
        errs = [C.rel_inf(x[u], ref[u]) for u in on]
        print(f"x{3 - x.shape[1]}: worst e_u / max(s_u, 2^-40) =",
              max(e / max(s, C.FLOOR) for e, s in zip(errs, s_u[on])), "max e_u", max(errs))
        C.check_fixed_iteration(errs, s_u[on])
        st = stable.astype(bool)
        assert np.array_equal(rank[st], rank_ref[st])
        assert st.sum() >= 14


def test_scores_from_reference_models(table, fit_ref, cpu_scores, fx):
    S = table.scores(fit_ref)
    for u, (s, bound) in enumerate(cpu_scores):
        assert np.array_equal(S[u], s), fx["names"][u]
        assert np.all(np.abs(S[u] - fx["scores"][u]) <= bound), fx["names"][u]
    # the fit threshold is not the predict threshold: products in (1e-6, 0.1] go to model 0
    u = fx["names"].index("fit_threshold")
    tp, gp, x0, x1 = fx["ref_models"][u]
    td = np.array([T.dots_of(int(m), tp, gp, fx)[0] for m in fx["med_keys"]])
    between = (td > 1e-6) & (td <= 0.1)
    assert between.any() and (td < -0.1).any()
    c = int(np.nonzero(between)[0][0])
    gd = T.dots_of(int(fx["med_keys"][c]), tp, gp, fx)[1]
    assert S[u, c] == ((0.0 + td[c] * x0[0]) + gd * x0[1] + x0[2]) + fx["med_vals"][c]


@pytest.mark.parametrize("N", [1, 7, 60, 1024])
@pytest.mark.parametrize("with_rated", [False, True])
def test_top_n_from_reference_models(table, fit_ref, cpu_scores, fx, N, with_rated):
    rated = [dict(l) for l in fx["lists"]] if with_rated else None
    got = table.top_n(fit_ref, rated, N)
    for u, (s, _) in enumerate(cpu_scores):
        want = C.exact_top_n(s, fx["med_keys"], rated[u] if with_rated else {}, N)
        assert got[u] == want, fx["names"][u]


def test_top_n_rated_as_csr(table, fit_ref, fx):
    lists = fx["lists"]
    off = np.zeros(len(lists) + 1, np.int64)
    off[1:] = np.cumsum([len(l) + 1 for l in lists])
    ids = np.concatenate([[m for m, _ in l] + [10 ** 6] for l in lists])   # one unknown id each
    a = table.top_n_arrays(fit_ref, (off, ids), 60)
    b = table.top_n_arrays(fit_ref, [dict(l) for l in lists], 60)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_agreement_from_reference_models(table, fit_ref, fx):
    res = table.evaluate_fit(fit_ref, fx["t_lists"])
    assert np.array_equal(np.isnan(res["agreement"]), np.isnan(fx["agreement"]))
    ok = ~np.isnan(fx["agreement"])
    assert ok.sum() >= 25
    assert np.array_equal(res["agreement"][ok], fx["agreement"][ok])
    assert np.array_equal(res["n_agree"][ok], fx["n_agree"][ok])
    assert np.array_equal(res["n_disagree"][ok], fx["n_disagree"][ok])


def _same(a, u, b, v):
    pa, pb = slice(a.tp_off[u], a.tp_off[u + 1]), slice(b.tp_off[v], b.tp_off[v + 1])
    return (np.array_equal(a.tp_idx[pa], b.tp_idx[pb])
            and np.array_equal(a.tp_val[pa], b.tp_val[pb])
            and np.array_equal(a.genre_dense[u], b.genre_dense[v])
            and np.array_equal(a.x0[u], b.x0[v]) and np.array_equal(a.x1[u], b.x1[v])
            and all(getattr(a, n)[u] == getattr(b, n)[v]
                    for n in ("has0", "has1", "n0", "rank0", "rank1")))


def test_batch_independence(table, fit_gpu, fx):
    again = table.fit(fx["lists"])
    for u in range(len(again)):
        assert _same(again, u, fit_gpu, u)
    names = fx["names"]
    for n in ("len0_0", "len1_1", "len2_0", "len600_1", "len65_0", "len129_0", "cancelling",
              "all_three", "a0_three_rows"):
        u = names.index(n)
        assert _same(table.fit([fx["lists"][u]]), 0, fit_gpu, u), n      # a batch of one
    a, b, c = names.index("len2_1"), names.index("len600_0"), names.index("len0_1")
    mixed = table.fit([fx["lists"][i] for i in (a, b, c, a)])
    assert _same(mixed, 0, fit_gpu, a) and _same(mixed, 1, fit_gpu, b)
    assert _same(mixed, 2, fit_gpu, c) and _same(mixed, 3, fit_gpu, a)


def test_fit_split_over_launches(gpu):
    """A fit launch holds the dense tag rows of its users in 1 GiB: on a table
    of 9,000 tags (72,000 bytes a row) 15,000 copies of a short list take two
    launches, and every copy gives the bits of the list fitted alone."""
    rs = np.random.RandomState(7)
    n_movies, n_tags = 400, 9000
    movies = list(range(1, n_movies + 1))
    genres = {m: {int(g) for g in rs.choice(19, 2, replace=False)} for m in movies}
    # 23 tags of a block that walks over all 9,000, and 30 random ones
    tags = {m: {int(t): float(np.log(rs.randint(1, 30)) + 1)
                for t in [(m * 23 + j) % n_tags for j in range(23)]
                + list(rs.choice(n_tags, 30, replace=False))} for m in movies}
    tag_counts = {}
    for dct in tags.values():
        for t in dct:
            tag_counts[t] = tag_counts.get(t, 0) + int(rs.randint(1, 30))
    genre_counts = {g: 40 + g for g in range(19)}
    med = {m: float(rs.choice(np.arange(1, 11) / 2)) for m in movies}
    lst = [(int(m), float(r)) for m, r in zip(rs.choice(movies, 7, replace=False),
                                               (5.0, 4.5, 1.0, 3.0, 4.0, 5.0, 2.5))]
    copies = 15000
    with TagCountTable(genres, tags, tag_counts, genre_counts, med) as t:
        assert t.num_tags * 8 * copies > 1 << 30 > t.num_tags * 8 * (copies // 2)
        one = t.fit([lst])
        off = np.arange(copies + 1, dtype=np.int64) * len(lst)
        f = t.fit((off, np.tile([m for m, _ in lst], copies), np.tile([r for _, r in lst], copies)))
    d = dict(movie_genres=genres, movie_tags=tags, tag_counts=tag_counts,
             genre_counts=genre_counts, med=med)
    m = T.CpuModel(lst, d)
    assert one.tag_profile(0) == _nonzero(m.tag_profile) and one.n0[0] == m.n0 >= 3
    assert C.rel_inf(one.x0[0], m.x0) <= 1e-9 and C.rel_inf(one.x1[0], m.x1) <= 1e-9
    k = one.tp_off[1]
    assert np.array_equal(f.tp_off, np.arange(copies + 1) * k)
    assert np.all(f.tp_idx.reshape(copies, k) == one.tp_idx[None, :])
    assert np.all(f.tp_val.reshape(copies, k) == one.tp_val[None, :])
    assert np.all(f.genre_dense == one.genre_dense[0][None, :])
    assert np.all(f.x0 == one.x0[0][None, :]) and np.all(f.x1 == one.x1[0][None, :])
    for n in ("has0", "has1", "n0", "rank0", "rank1"):
        assert np.all(getattr(f, n) == getattr(one, n)[0]), n


def test_scores_and_top_n_over_user_chunks(gpu):
    """A scores / top-N launch takes at most 65,535 users (the score grid's y
    extent): 65,535 + 9 models on a ten-movie table take two, and every user
    on either side of the boundary gets what its model gets in a small batch
    -- models, CSR profile offsets, exclusion lists and output rows all follow
    the chunk."""
    rs = np.random.RandomState(3)
    movies = list(range(11, 21))
    genres = {m: {int(g) for g in rs.choice(6, 2, replace=False)} for m in movies}
    tags = {m: {int(t): float(rs.randint(1, 5)) for t in rs.choice(8, 2, replace=False)}
            for m in movies[:7]}
    tag_counts = {t: 1 + sum(int(dd.get(t, 0)) for dd in tags.values()) for t in range(8)}
    genre_counts = {g: 3 + g for g in range(6)}
    med = {m: float(rs.choice(np.arange(1, 11) / 2)) for m in movies}
    d = dict(movie_genres=genres, movie_tags=tags, tag_counts=tag_counts,
             genre_counts=genre_counts, med=med, med_keys=np.array(movies),
             med_vals=np.array([med[m] for m in movies]))
    models = [({}, {}, None, None), ({}, {1: 0.5}, None, [0.5, -1.0]),
              ({0: 0.25, 3: 1.5}, {0: 1.0, 2: -0.5}, [40.0, 1.5, 0.0], [2.0, 0.125]),
              ({1: -2.0, 2: 0.75, 7: 9.0}, {}, [-2.0, 0.75, 9.0], None),
              ({5: 1e-7}, {4: 2.0, 5: 0.25}, [1.0, 1.0, 1.0], [3.0, -7.0]),
              ({t: 0.5 + t for t in range(8)}, {g: 1.0 - g for g in range(6)},
               [0.125, -0.5, 3.0], [1.0, -3.0]),
              ({4: 3.0, 6: -1.0}, {3: 0.5}, [1.0, -1.0, 2.0], [-2.0, 3.0])]
    base_rated = [[], [11], [12, 13, 999], [20], list(range(11, 19)), [15, 16], [14, 17, 19]]
    n = 65535 + 9
    idx = np.arange(n) % len(models)
    lens = np.array([len(r) for r in base_rated])
    off = np.concatenate([[0], np.cumsum(lens[idx])]).astype(np.int64)
    ids = np.concatenate([np.asarray(base_rated[b], np.int64) for b in idx])
    with TagCountTable(genres, tags, tag_counts, genre_counts, med) as t:
        base = TagCountFit.from_models(t, models)
        plen = np.diff(base.tp_off)
        big = TagCountFit(
            t, base.genre_dense[idx], np.concatenate([[0], np.cumsum(plen[idx])]),
            np.concatenate([base.tp_idx[base.tp_off[b]:base.tp_off[b + 1]] for b in idx]),
            np.concatenate([base.tp_val[base.tp_off[b]:base.tp_off[b + 1]] for b in idx]),
            base.x0[idx], base.x1[idx], base.has0[idx], base.has1[idx])
        s_small = t.scores(base)
        m_small, sc_small, c_small = t.top_n_arrays(base, base_rated, 4)
        s_big = t.scores(big)
        m_big, sc_big, c_big = t.top_n_arrays(big, (off, ids), 4)
    for b, mdl in enumerate(models):        # the small batch itself is the restatement's answer
        s = T.exact_scores(mdl, d)[0]
        assert np.array_equal(s_small[b], s), b
        want = C.exact_top_n(s, d["med_keys"], set(base_rated[b]), 4)
        assert list(zip(sc_small[b, :c_small[b]], m_small[b, :c_small[b]])) == want
    assert c_small.tolist() == [4, 4, 4, 4, 2, 4, 4]
    assert np.array_equal(s_big, s_small[idx])
    assert np.array_equal(c_big, c_small[idx])
    valid = np.arange(4)[None, :] < c_big[:, None]          # a row is defined up to its count
    assert np.array_equal(np.where(valid, m_big, 0), np.where(valid, m_small[idx], 0))
    assert np.array_equal(np.where(valid, sc_big, 0.0), np.where(valid, sc_small[idx], 0.0))


def _param_list(fx, name):
    u = fx["names"].index(name)
    a, b = fx["par_off"][u], fx["par_off"][u + 1]
    return [str(s) for s in fx["par_name"][a:b]], fx["par_val"][a:b]


def test_model_and_recommendations_end_to_end(table, fx):
    from movie_recommender_amd.serving import get_recommendations
    names = fx["names"]
    no_median = next(k for k in fx["movie_genres"] if k not in fx["med"])
    for n in ("len65_0", "len600_0", "fit_threshold", "cancelling", "all_three", "len1_0",
              "len0_1"):
        u = names.index(n)
        lst = fx["lists"][u]
        m = TagCount_UserProfile(fx["movie_genres"], lst, fx["movie_tags"], fx["tag_counts"],
                                 fx["genre_counts"], fx["med"], fx["genre_names"],
                                 fx["tag_names"], table=table)
        assert m.is_valid()
        assert list(m.tag_profile.items()) == list(fx["tag_profiles"][u].items()), n
        assert list(m.genre_profile.items()) == list(fx["genre_profiles"][u].items()), n
        assert (m.x_factors0 is not None) == bool(fx["has0"][u])
        assert (m.x_factors1 is not None) == bool(fx["has1"][u])
        if m.x_factors0 is not None:
            assert m.x_factors0.shape == (3, 1)
        if m.x_factors1 is not None:
            assert m.x_factors1.shape == (2, 1)
        s = T.exact_scores((m.tag_profile, m.genre_profile, m.x_factors0, m.x_factors1), fx)[0]
        for c in (0, 5, 100, len(s) - 1):
            assert m.predict(int(fx["med_keys"][c])) == s[c]
        assert m.predict(no_median) is None
        rot, full = get_recommendations(m, dict(lst), 60, rotation=1)
        want = [mid for _, mid in C.exact_top_n(s, fx["med_keys"], dict(lst), 60)]
        assert full == want and rot == want[1::4]
        if n in ("len65_0", "all_three", "len1_0"):
            ref_names, ref_vals = _param_list(fx, n)
            got = m.get_param_list()
            assert [f"{k}:{v}" if k == "__comment" else k for k, v in got] == ref_names
            x_rows = {i for i, k in enumerate(ref_names) if k in ("tag importance",
                                                                  "genre importance", "user bias")}
            for i, (k, v) in enumerate(got):
                if k == "__comment":
                    continue
                if i in x_rows:      # coefficients: inside the spread rule's floor here
                    assert abs(v - ref_vals[i]) <= 8 * C.FLOOR * max(1.0, abs(ref_vals[i]))
                else:                # profile values: exact
                    assert v == ref_vals[i]
    assert m.get_param_list() == []                       # len0_1: nothing to list
    with pytest.raises(KeyError):
        TagCount_UserProfile(fx["movie_genres"], [(int(fx["med_keys"][0]), 3.0), (10 ** 7, 1.0)],
                             fx["movie_tags"], fx["tag_counts"], fx["genre_counts"], fx["med"],
                             table=table)


def test_evals_equal_per_user_path_and_restatement(table, fx):
    idx = [fx["names"].index(n) for n in ("len0_0", "len1_1", "len4_0", "len65_1", "len129_0",
                                          "fit_threshold", "all_three", "const_genre")]
    train = [(1000 + u, fx["lists"][u]) for u in idx]
    test = [(1000 + u, fx["t_lists"][u]) for u in idx]
    got = tag_count_eval(train, test, fx["movie_genres"], fx["movie_tags"], fx["tag_counts"],
                         fx["genre_counts"], fx["med"])
    assert got == tag_count_eval(train, test, None, None, None, None, None, table=table)
    want = []
    for (uid, tr), (_, te) in zip(train, test):
        m = TagCount_UserProfile(fx["movie_genres"], tr, fx["movie_tags"], fx["tag_counts"],
                                 fx["genre_counts"], fx["med"], table=table)
        pred = np.array([np.nan if m.predict(mid) is None else m.predict(mid) for mid, _ in te])
        val, _, _ = C.agreement_counts([a for _, a in te], pred)
        if val is not None:
            want.append((uid, val))
    assert got == want and len(want) >= 6
    # the median predictor; the last user has no test movie with a median, the one before a
    # single one: neither has an agreement
    no_median = [k for k in fx["movie_genres"] if k not in fx["med"]]
    test = test + [(7, [(int(fx["med_keys"][3]), 4.0), (no_median[0], 2.0)]),
                   (8, [(no_median[1], 1.0), (no_median[2], 5.0)])]
    got, stats = median_eval(test, fx["med"], return_stats=True)
    want = []
    for uid, te in test:
        pred = np.array([fx["med"].get(mid, np.nan) for mid, _ in te])
        val, _, _ = C.agreement_counts([a for _, a in te], pred)
        if val is not None:
            want.append((uid, val))
    assert got == want and len(want) == len(idx)
    assert np.array_equal(stats["pred"][~np.isnan(stats["pred"])],
                          np.array([fx["med"][m] for _, te in test for m, _ in te
                                    if m in fx["med"]]))
    assert got == median_eval(test, None, table=table)
