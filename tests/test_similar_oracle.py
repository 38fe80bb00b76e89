"""CPU: the similar-movies oracle (oracle/similar_oracle.py) reproduces the
fixtures made with the reference's SimilarMovieFinder, and the fixtures
exercise the num_results*20 cut and exact score ties."""
import numpy as np
import pytest

from oracle import similar_oracle as O
from similar_cases import (ExactSimilar, cut_ranges, exact_similar, expected, fixture,
                           fixture_arrays, synthetic_similar, to_dicts)


@pytest.mark.parametrize("nres", [20, 5, 40])
def test_find_similar_matches_reference(nres):
    d = fixture("main")
    exp = expected(d, nres)
    for q, e in zip(d["queries"].tolist()[:25], exp):
        ids, scores = O.find_similar_movie(d["genres"], d["movie_ratings"], q,
                                           float(d["buff_limit"]), int(d["buff_point"]), nres)
        assert (tuple(ids), tuple(scores)) == e or (ids == [] and e == ((), ()))


def test_fixture_exercises_cut_and_ties():
    d = fixture("main")
    mr, g = d["movie_ratings"], d["genres"]
    big = 0
    for q in d["queries"].tolist()[:12]:
        n = 0
        for j in range(len(mr)):
            if j != q and O.genres_similar(g, mr[q][0], mr[j][0]):
                s, _, _ = O.scaled_dot_product(mr, q, j, 0.05, 100)
                n += s > 0.3
        big += n > 20 * 20
    assert big >= 3
    scores = d["n20_scores"].tolist()
    assert len(scores) != len(set(scores))       # bit-equal scores (twin movies)


# ---------------------------------------------------------------------------
# the vectorised restatement (similar_cases.ExactSimilar) that the large GPU
# cases of test_gpu_similar_ranges.py are compared with
# ---------------------------------------------------------------------------
def _bits(x):
    return np.asarray(x, np.float64).view(np.int64)


@pytest.mark.parametrize("nres", [20, 5, 40])
def test_exact_restatement_matches_reference_fixture(nres):
    """All 60 queries of the reference-made fixture, ids and score bits."""
    d = fixture("main")
    queries = d["queries"].tolist()
    got = exact_similar(fixture_arrays(d), queries, float(d["buff_limit"]),
                        int(d["buff_point"]), nres)
    assert len(queries) == 60
    for q, (ids, scores, total), (eids, escores) in zip(queries, got, expected(d, nres)):
        assert np.array_equal(ids, np.asarray(eids, np.int64)), q
        assert np.array_equal(_bits(scores), _bits(escores)), q
        assert total >= len(eids)


def test_exact_restatement_matches_dict_oracle_across_ranges():
    """Just above one accumulation range (M = 4200): a core movie, both twins
    of the pair across the range boundary and of the core pair, a movie
    without raters, one without genres, the last movie."""
    M, core = 4200, 24
    arrays = synthetic_similar(5, M, 1500, core, 40)
    _, off, uid, _, U, _, has = arrays
    assert U > int(uid.max()) + 1 and 0 not in uid            # users without ratings
    genres, mr = to_dicts(arrays)
    assert sorted(m for m, _ in mr) != [m for m, _ in mr]     # ids not monotone
    no_genres = int(np.flatnonzero((has == 0) & (np.diff(off) >= 3))[0])
    queries = [0, 2, core - 3, 4095, 4096, 4097, no_genres, 1000, M - 1, 40]
    assert len(mr[4097][1]) == 0
    ex = ExactSimilar(arrays, 0.05, 100)
    totals = []
    for nres in (20, 3):
        for q in queries:
            ids, scores, total, _ = ex.find(q, nres)
            eids, escores = O.find_similar_movie(genres, mr, q, 0.05, 100, nres)
            assert np.array_equal(ids, np.asarray(eids, np.int64)), (q, nres)
            assert np.array_equal(_bits(scores), _bits(escores)), (q, nres)
            totals.append(total)
    assert max(totals) > 400 and min(totals) == 0             # both orderings were compared
    ids, _, _, _ = ex.find(4095, 20)
    assert mr[4096][0] in ids.tolist()                        # the twin across the boundary


def test_cut_rule_on_hand_made_lists():
    """similar_cases.cut_ranges (the kernel's list-cut rule, used by the GPU
    tests to assert that their inputs reach the mid-stream cut)."""
    M = 8300
    full = np.arange(2048)                                    # 1024 + 1024, then cut at chunk 2
    assert cut_ranges(full, M, 20) == ([0], True, 2048)
    assert cut_ranges(np.arange(1025), M, 51) == ([0], True, 1025)
    assert cut_ranges(np.arange(1024), M, 51) == ([], True, 0)
    assert cut_ranges(np.arange(1020), M, 51) == ([], False, 0)
    both = np.concatenate([np.arange(1100), 4096 + np.arange(1100)])
    assert cut_ranges(both, M, 20)[0] == [0, 1]
