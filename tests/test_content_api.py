"""CPU: the content model's NumPy restatement (tests/content_cases.py) against
the reference's recorded results (tests/golden/content_small.npz) by the
acceptance rules the GPU is held to as well, and the Python-level argument
checks of movie_recommender_amd.content (they need no device)."""
import numpy as np
import pytest

import content_cases as C
from movie_recommender_amd import content
from movie_recommender_amd.content import TagFit, TagLS_UserProfile, TagTable


@pytest.fixture(scope="module")
def fx():
    return C.fixture()


@pytest.fixture(scope="module")
def cpu_default(fx):
    return [C.CpuModel(l, fx) for l in fx["lists"]]


def test_fixture_covers_the_cases(fx):
    names = fx["names"]
    for n in ("featureless", "few_ids", "tie_by_id", "listed_twice", "b_zero", "cooccur"):
        assert n in names
    lens = sorted({len(l) for l in fx["lists"]})
    for n in (2, 3, 10, 11, 30, 31, 70, 71, 150, 151, 310, 311, 600):
        assert n in lens
    assert fx["p"][names.index("featureless")] == 0
    u = names.index("few_ids")
    assert fx["p"][u] < C.decide_num_factors(len(fx["lists"][u]))
    assert fx["profiles"][names.index("tie_by_id")] == [5, 2]
    assert fx["itn_ref"][names.index("b_zero")] == 0
    assert fx["profile"].max() >= 66000 + 1000 and fx["p"].max() == 25
    assert 8 <= fx["stable"].sum() < len(names)
    assert len(fx["med_keys"]) < len(set(fx["mg_mid"]) | set(fx["mt_mid"]) | set(fx["med_keys"]))


def test_profiles_exact(fx, cpu_default):
    for u, m in enumerate(cpu_default):
        assert m.profile == fx["profiles"][u], fx["names"][u]


def test_b_zero_and_iteration_limit(fx):
    u = fx["names"].index("b_zero")
    m = C.CpuModel(fx["lists"][u], fx)
    assert (m.itn, m.istop) == (0, 0) and not m.x.any()
    u = fx["names"].index("len100_0")
    m = C.CpuModel(fx["lists"][u], fx, iter_lim=3)
    assert (m.itn, m.istop) == (3, 7)


def test_fixed_iteration_rule(fx):
    errs = []
    for u, l in enumerate(fx["lists"]):
        m = C.CpuModel(l, fx, atol=0, btol=0, conlim=0, iter_lim=int(fx["itn_ref"][u]))
        assert m.itn == fx["itn_ref"][u]
        errs.append(C.rel_inf(C.x_row(m.x), fx["x_ref"][u]))
    C.check_fixed_iteration(errs, fx["s_u"])


def test_stop_rule(fx, cpu_default):
    C.check_stop([m.itn for m in cpu_default], [m.istop for m in cpu_default], fx)
    errs = []
    for u, m in enumerate(cpu_default):
        # the stops change no arithmetic: the same bits as the fixed-iteration run
        f = C.CpuModel(fx["lists"][u], fx, atol=0, btol=0, conlim=0, iter_lim=m.itn)
        assert np.array_equal(f.x, m.x), fx["names"][u]
        ref = fx["traj"][u][m.itn - 1] if m.itn else np.zeros(C.ROW)
        errs.append(C.rel_inf(C.x_row(m.x), ref))
    C.check_fixed_iteration(errs, fx["s_u"])


def test_scores_top_n_and_agreement_from_x_ref(fx):
    mids = fx["med_keys"]
    for u, l in enumerate(fx["lists"]):
        prof, x = fx["profiles"][u], fx["x_ref"][u]
        attr = C.attr_matrix(prof, fx)
        s = C.exact_scores(prof, x, fx, attr)
        bound = C.score_bound(prof, x, fx, attr)
        assert np.all(np.abs(s - fx["scores"][u]) <= bound), fx["names"][u]
        # the reference's top-60: the same movies wherever no two scores lie inside the bound
        top = C.exact_top_n(s, mids, dict(l), 60)
        ref = fx["recs"][u]
        assert len(top) == len(ref)
        b = dict(zip(mids.tolist(), bound.tolist()))
        for (s1, m1), (s2, m2) in zip(top, ref):
            assert m1 == m2 or abs(s1 - s2) <= b[m1] + b[m2]
        # agreement on the held-out list
        tl = fx["t_lists"][u]
        idx = {int(m): c for c, m in enumerate(mids)}
        pred = np.array([s[idx[m]] if m in idx else np.nan for m, _ in tl])
        val, ag, dg = C.agreement_counts([a for _, a in tl], pred)
        if np.isnan(fx["agreement"][u]):
            assert val is None
        else:
            assert val == fx["agreement"][u]
            assert (ag, dg) == (fx["n_agree"][u], fx["n_disagree"][u])


@pytest.mark.parametrize("n,want", [
    (0, 0), (1, 0), (2, 1), (9, 4), (10, 5), (11, 5), (13, 5), (14, 6), (29, 9), (30, 10),
    (31, 10), (37, 10), (38, 11), (69, 14), (70, 15), (71, 15), (85, 15), (86, 16), (149, 19),
    (150, 20), (151, 20), (181, 20), (182, 21), (309, 24), (310, 25), (311, 25), (100000, 25)])
def test_decide_num_factors(n, want):
    assert content.decide_num_factors(n) == want
    assert C.decide_num_factors(n) == want


def _table(fx):
    return TagTable(fx["movie_genres"], fx["movie_tags"], fx["tag_counts"], fx["med"])


def test_table_layout(fx):
    t = _table(fx)
    assert t.cand_mid.tolist() == fx["med_keys"].tolist()
    for c in (0, 17, len(t.cand_mid) - 1):
        f = C.movie_features(int(t.cand_mid[c]), fx["movie_genres"], fx["movie_tags"],
                             fx["tag_counts"])
        a, b = t.feat_off[c], t.feat_off[c + 1]
        assert t.feat_id[a:b].tolist() == sorted(f)
        assert t.feat_val[a:b].tolist() == [f[i] for i in sorted(f)]


def test_argument_checks(fx):
    t = _table(fx)
    m0, m1 = int(fx["med_keys"][0]), int(fx["med_keys"][1])
    with pytest.raises(ValueError):
        t.fit([[(m0, 3.0)]])                                   # the reference raises too
    no_median = next(m for m in fx["movie_genres"] if m not in fx["med"])
    with pytest.raises(KeyError):
        t.fit([[(m0, 3.0), (no_median, 2.0)]])
    with pytest.raises(KeyError):
        t.fit([[(m0, 3.0), (10 ** 7, 2.0)]])
    with pytest.raises(ValueError):
        t.fit([[(m0, 3.0), (m1, 2.0)]], iter_lim=[5, 5])
    with pytest.raises(ValueError):                             # offsets do not end at len(ids)
        t.fit((np.array([0, 3]), np.array([m0, m1]), np.array([3.0, 2.0])))
    with pytest.raises(ValueError):                             # decreasing offsets
        t.fit((np.array([0, 2, 1, 2]), np.array([m0, m1]), np.array([3.0, 2.0])))
    fit = TagFit.from_models([([3], [0.5, 0.1])])
    for n in (0, 1025, -1):
        with pytest.raises(ValueError):
            t.top_n_arrays(fit, None, n)
    with pytest.raises(ValueError):
        t.top_n_arrays(fit, (np.array([0, 5]), np.array([m0])), 10)
    with pytest.raises(ValueError):
        t.top_n_arrays(fit, [[m0], [m1]], 10)
    with pytest.raises(ValueError):
        TagFit.from_models([([3, 4], [0.5, 0.1])])
    with pytest.raises(ValueError):
        TagFit.from_models([([3, 3], [0.5, 0.1, 0.2])])
    with pytest.raises(ValueError):
        t.evaluate_fit(fit, [[(m0, 3.0)], [(m1, 2.0)]])


def test_table_cache_keeps_its_keys_alive(fx):
    """tag_table_for caches on the identity of all four dictionaries, holds
    them while cached, and keeps at most MAX_CACHED_TABLES tables."""
    content._TABLES.clear()
    args = [fx["movie_genres"], fx["movie_tags"], fx["tag_counts"], fx["med"]]
    t = content.tag_table_for(*args)
    assert content.tag_table_for(*args) is t
    for i in range(4):                       # a new object in any place is a new table
        other = list(args)
        other[i] = dict(args[i])
        t2 = content.tag_table_for(*other)
        assert t2 is not t
        entry = next(e for e in content._TABLES.values() if e[0] is t2)
        assert all(a is b for a, b in zip(entry[1], other))
    assert len(content._TABLES) == content.MAX_CACHED_TABLES
    assert not any(e[0] is t for e in content._TABLES.values())     # least recently used left
    content._TABLES.clear()


def test_get_param_list_format():
    m = object.__new__(TagLS_UserProfile)
    m.profile = [1007, 3, 1002, 5]
    m.x_factors = np.array([[0.5], [-1.0], [2.0], [4.0], [0.25]])
    m._genre_ids, m._tag_ids = {"Drama": 3, "Noir": 5}, {"dark": 7, "slow": 2}
    assert m.get_param_list() == [("__comment", "Genre Parameters"), ("Noir", 4.0),
                                  ("Drama", -1.0), ("__comment", "Tag Parameters"),
                                  ("slow", 2.0), ("dark", 0.5)]
    m._tag_ids = None
    assert m.get_param_list() == []
    m._genre_ids, m._tag_ids = {"Drama": 3, "Noir": 5}, {"dark": 7, "slow": 2}
    m.profile, m.x_factors = [1007], np.array([[0.5], [0.25]])
    assert m.get_param_list() == [("__comment", "Tag Parameters"), ("dark", 0.5)]


def test_get_recommendations_rejects_foreign_objects():
    from movie_recommender_amd.serving import get_recommendations

    class Invalid:
        def is_valid(self):
            return False

    with pytest.raises(ValueError):
        get_recommendations(Invalid(), {})
    with pytest.raises((AttributeError, TypeError)):
        get_recommendations(object(), {})
    with pytest.raises((AttributeError, TypeError)):
        get_recommendations({"profile": [3]}, {})
