"""GPU: the content model (tag least squares) against the reference's recorded
results by the rules of tests/content_cases.py -- exact profiles, LSQR inside
the reference's own rounding spread at a fixed iteration count, the stopping
rule, and exact scores / top-N / agreement given x -- plus batch independence
and the paths that depend on sizes."""
import numpy as np
import pytest

import content_cases as C
from movie_recommender_amd.content import (TagFit, TagLS_UserProfile, TagTable, tag_ls_eval)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return C.fixture()


@pytest.fixture(scope="module")
def table(gpu, fx):
    with TagTable(fx["movie_genres"], fx["movie_tags"], fx["tag_counts"], fx["med"]) as t:
        yield t


@pytest.fixture(scope="module")
def fit_default(table, fx):
    return table.fit(fx["lists"])


@pytest.fixture(scope="module")
def fit_ref(fx):
    """The reference's models (profile, x_ref) as the GPU takes them."""
    return TagFit(fx["p"], fx["profile"], fx["x_ref"])


@pytest.fixture(scope="module")
def cpu_scores(fx):
    out = []
    for u in range(len(fx["lists"])):
        attr = C.attr_matrix(fx["profiles"][u], fx)
        out.append((C.exact_scores(fx["profiles"][u], fx["x_ref"][u], fx, attr),
                    C.score_bound(fx["profiles"][u], fx["x_ref"][u], fx, attr)))
    return out


def test_profiles_exact(fit_default, fx):
    assert np.array_equal(fit_default.p, fx["p"])
    assert np.array_equal(fit_default.profile, fx["profile"])


def test_b_zero_and_iteration_limit(table, fit_default, fx):
    u = fx["names"].index("b_zero")
    assert fit_default.itn[u] == 0 and fit_default.istop[u] == 0
    assert not fit_default.x[u].any()
    f = table.fit([fx["lists"][fx["names"].index("len100_0")]], iter_lim=3)
    assert (f.itn[0], f.istop[0]) == (3, 7)


def test_fixed_iteration_rule(table, fx):
    f = table.fit(fx["lists"], atol=0, btol=0, conlim=0, iter_lim=fx["itn_ref"])
    assert np.array_equal(f.itn, fx["itn_ref"])
    errs = [C.rel_inf(f.x[u], fx["x_ref"][u]) for u in range(len(f))]
    print("fixed iteration: worst e_u / max(s_u, 2^-40) =",
          max(e / max(s, C.FLOOR) for e, s in zip(errs, fx["s_u"])), "max e_u", max(errs))
    C.check_fixed_iteration(errs, fx["s_u"])


def test_stop_rule(table, fit_default, fx):
    itn, istop = fit_default.itn, fit_default.istop
    print("stop iterations", itn.tolist(), "reference", fx["itn_ref"].tolist())
    C.check_stop(itn, istop, fx)
    # the stops change no arithmetic: the same bits as the fixed-iteration run at that itn
    f = table.fit(fx["lists"], atol=0, btol=0, conlim=0, iter_lim=itn)
    assert np.array_equal(f.x, fit_default.x)
    errs = [C.rel_inf(fit_default.x[u], fx["traj"][u][itn[u] - 1] if itn[u] else np.zeros(C.ROW))
            for u in range(len(itn))]
    C.check_fixed_iteration(errs, fx["s_u"])


def test_scores_from_x_ref(table, fit_ref, cpu_scores, fx):
    S = table.scores(fit_ref)
    for u, (s, bound) in enumerate(cpu_scores):
        assert np.array_equal(S[u], s), fx["names"][u]
        assert np.all(np.abs(S[u] - fx["scores"][u]) <= bound), fx["names"][u]


@pytest.mark.parametrize("N", [1, 7, 60, 1024])
@pytest.mark.parametrize("with_rated", [False, True])
def test_top_n_from_x_ref(table, fit_ref, cpu_scores, fx, N, with_rated):
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


def test_agreement_from_x_ref(table, fit_ref, fx):
    res = table.evaluate_fit(fit_ref, fx["t_lists"])
    assert np.array_equal(np.isnan(res["agreement"]), np.isnan(fx["agreement"]))
    ok = ~np.isnan(fx["agreement"])
    assert np.array_equal(res["agreement"][ok], fx["agreement"][ok])
    assert np.array_equal(res["n_agree"][ok], fx["n_agree"][ok])
    assert np.array_equal(res["n_disagree"][ok], fx["n_disagree"][ok])


def _same(a, u, b, v):
    return (a.p[u] == b.p[v] and np.array_equal(a.profile[u], b.profile[v])
            and np.array_equal(a.x[u], b.x[v]) and a.itn[u] == b.itn[v]
            and a.istop[u] == b.istop[v])


def test_batch_independence(table, fit_default, fx):
    again = table.fit(fx["lists"])
    for u in range(len(again)):
        assert _same(again, u, fit_default, u)
    names = fx["names"]
    for n in ("len2_0", "len600_1", "len151_0", "len71_1", "cooccur", "featureless", "b_zero"):
        u = names.index(n)
        assert _same(table.fit([fx["lists"][u]]), 0, fit_default, u), n      # a batch of one
    a, b = names.index("len2_1"), names.index("len600_0")
    mixed = table.fit([fx["lists"][a], fx["lists"][b], fx["lists"][a]])
    assert _same(mixed, 0, fit_default, a) and _same(mixed, 1, fit_default, b)
    assert _same(mixed, 2, fit_default, a)


def test_fit_split_over_launches(table, fit_default, fx):
    """A fit launch holds lists up to 48 Mi entries of A scratch (length x
    allowed factors each): 3400 copies of a 600-rating list take two launches,
    and every copy gives the bits of the list fitted alone."""
    u = fx["names"].index("len600_0")
    lst = fx["lists"][u]
    copies = 3400
    assert copies * 600 * 25 > 48 << 20 > (copies // 2) * 600 * 25
    off = np.arange(copies + 1, dtype=np.int64) * len(lst)
    f = table.fit((off, np.tile([m for m, _ in lst], copies), np.tile([r for _, r in lst], copies)))
    assert np.all(f.p == fit_default.p[u]) and np.all(f.itn == fit_default.itn[u])
    assert np.all(f.istop == fit_default.istop[u])
    assert np.all(f.profile == fit_default.profile[u][None, :])
    assert np.all(f.x == fit_default.x[u][None, :])


def test_scores_and_top_n_over_user_chunks(gpu):
    """A scores / top-N launch takes at most 65,535 users (the score grid's y
    extent) or 1 GiB of keys: 65,535 + 9 models on a ten-movie table take two,
    and every user on either side of the boundary gets what its model gets in
    a small batch -- models, exclusion lists and output rows all follow the
    chunk."""
    rs = np.random.RandomState(3)
    movies = list(range(11, 21))
    genres = {m: {int(g) for g in rs.choice(6, 2, replace=False)} for m in movies}
    tags = {m: {int(t): float(rs.randint(1, 5)) for t in rs.choice(8, 2, replace=False)}
            for m in movies[:7]}
    counts = {t: 1 + sum(int(d.get(t, 0)) for d in tags.values()) for t in range(8)}
    med = {m: float(rs.choice(np.arange(1, 11) / 2)) for m in movies}
    base = TagFit.from_models([([], [0.25]), ([3], [0.5, -1.0]), ([1002, 0], [40.0, 1.5, 0.0]),
                               ([5, 1, 1007], [-2.0, 0.75, 9.0, 0.5]), ([2, 4], [1.0, 1.0, 1.0]),
                               ([1000, 1001, 1003, 1], [3.0, -7.0, 11.0, 0.125, -0.5]),
                               ([0, 1, 2, 3, 4, 5], [1.0, -1.0, 2.0, -2.0, 3.0, -3.0, 0.0])])
    base_rated = [[], [11], [12, 13, 999], [20], list(range(11, 19)), [15, 16], [14, 17, 19]]
    n = 65535 + 9
    idx = np.arange(n) % len(base)
    big = TagFit(base.p[idx], base.profile[idx], base.x[idx])
    lens = np.array([len(r) for r in base_rated])
    off = np.concatenate([[0], np.cumsum(lens[idx])]).astype(np.int64)
    ids = np.concatenate([np.asarray(base_rated[b], np.int64) for b in idx])
    with TagTable(genres, tags, counts, med) as t:
        s_small = t.scores(base)
        m_small, sc_small, c_small = t.top_n_arrays(base, base_rated, 4)
        s_big = t.scores(big)
        m_big, sc_big, c_big = t.top_n_arrays(big, (off, ids), 4)
    d = dict(movie_genres=genres, movie_tags=tags, tag_counts=counts, med=med,
             med_keys=np.array(movies), med_vals=np.array([med[m] for m in movies]))
    for b in range(len(base)):        # the small batch itself is the restatement's answer
        s = C.exact_scores(base.profile_list(b), base.x[b, :base.p[b] + 1], d)
        assert np.array_equal(s_small[b], s)
        want = C.exact_top_n(s, d["med_keys"], set(base_rated[b]), 4)
        assert list(zip(sc_small[b, :c_small[b]], m_small[b, :c_small[b]])) == want
    assert c_small.tolist() == [4, 4, 4, 4, 2, 4, 4]
    assert np.array_equal(s_big, s_small[idx])
    assert np.array_equal(c_big, c_small[idx])
    valid = np.arange(4)[None, :] < c_big[:, None]          # a row is defined up to its count
    assert np.array_equal(np.where(valid, m_big, 0), np.where(valid, m_small[idx], 0))
    assert np.array_equal(np.where(valid, sc_big, 0.0), np.where(valid, sc_small[idx], 0.0))


def test_profile_over_several_counter_passes(gpu):
    """The profile kernel counts 4096 distinct feature ids per pass: a table
    with 9000 tags takes three, and the kept ids come from all of them."""
    rs = np.random.RandomState(5)
    n_movies, n_tags = 400, 9000
    tids = np.sort(rs.choice(np.arange(1, 131072), n_tags, replace=False))   # ids up to 2^17
    genres = {m: {int(g) for g in rs.choice(19, 2, replace=False)} for m in range(1, n_movies + 1)}
    tags = {m: {int(t): float(rs.randint(1, 9)) for t in rs.choice(tids, 40, replace=False)}
            for m in range(1, n_movies + 1)}
    # three tags, one per pass, on every fifth movie: certain profile entries
    hot = [int(tids[10]), int(tids[5000]), int(tids[8999])]
    for m in range(1, n_movies + 1, 5):
        for t in hot:
            tags[m][t] = 2.0
    counts = {}
    for d in tags.values():
        for t, v in d.items():
            counts[t] = counts.get(t, 0) + int(v)
    med = {m: float(rs.choice(np.arange(1, 11) / 2)) for m in range(1, n_movies + 1)}
    d = dict(movie_genres=genres, movie_tags=tags, tag_counts=counts, med=med)
    lists = [[(int(m), float(rs.choice(np.arange(1, 11) / 2)))
              for m in rs.choice(np.arange(1, n_movies + 1), n, replace=False)]
             for n in (12, 80, 400)]
    with TagTable(genres, tags, counts, med) as t:
        f = t.fit(lists, atol=0, btol=0, conlim=0, iter_lim=3)
    for u, l in enumerate(lists):
        m = C.CpuModel(l, d, atol=0, btol=0, conlim=0, iter_lim=3)
        assert f.profile_list(u) == m.profile
        # three steps from the same start: rounding only (fp64, <= 26 columns, values O(1))
        assert C.rel_inf(f.x[u, :len(m.x)], m.x) <= 1e-9
    assert set(hot) <= {i - 1000 for i in f.profile_list(2)}


def test_model_and_recommendations_end_to_end(table, fx):
    from movie_recommender_amd.serving import get_recommendations
    names = fx["names"]
    for n in ("len30_0", "len311_0", "cooccur", "featureless"):
        u = names.index(n)
        lst = fx["lists"][u]
        m = TagLS_UserProfile(fx["movie_genres"], lst, fx["movie_tags"], fx["tag_counts"],
                              fx["med"], table=table)
        assert m.is_valid() and m.profile == fx["profiles"][u]
        assert m.x_factors.shape == (len(m.profile) + 1, 1)
        s = C.exact_scores(m.profile, m.x_factors, fx)
        for c in (0, 5, 100, len(s) - 1):
            assert m.predict(int(fx["med_keys"][c])) == s[c]
        assert m.predict(next(k for k in fx["movie_genres"] if k not in fx["med"])) is None
        rot, full = get_recommendations(m, dict(lst), 60, rotation=1)
        want = [mid for _, mid in C.exact_top_n(s, fx["med_keys"], dict(lst), 60)]
        assert full == want and rot == want[1::4]
    with pytest.raises(KeyError):
        TagLS_UserProfile(fx["movie_genres"],
                          [(int(fx["med_keys"][0]), 3.0), (10 ** 7, 1.0)], fx["movie_tags"],
                          fx["tag_counts"], fx["med"], table=table)


def test_tag_ls_eval_equals_per_user_path(table, fx):
    idx = [fx["names"].index(n) for n in ("len5_0", "len20_1", "len70_0", "len200_0", "b_zero",
                                          "few_ids", "len2_0")]
    train = [(1000 + u, fx["lists"][u]) for u in idx]
    test = [(1000 + u, fx["t_lists"][u]) for u in idx]
    got = tag_ls_eval(train, test, fx["movie_genres"], fx["movie_tags"], fx["tag_counts"],
                      fx["med"])
    want = []
    for (uid, tr), (_, te) in zip(train, test):
        m = TagLS_UserProfile(fx["movie_genres"], tr, fx["movie_tags"], fx["tag_counts"],
                              fx["med"], table=table)
        pred = np.array([np.nan if m.predict(mid) is None else m.predict(mid) for mid, _ in te])
        val, _, _ = C.agreement_counts([a for _, a in te], pred)
        if val is not None:
            want.append((uid, val))
    assert got == want and len(want) >= 5
