"""GPU: the similar-movies search (csrc/similar.hip through
SimilarMovieFinder.from_arrays) beyond one accumulation range and at the
edges of its candidate list, its packed 32-bit sums, its num_results range
and its refusals.

Expected values come from similar_cases.ExactSimilar, which
tests/test_similar_oracle.py pins bit for bit to the reference-made fixture
and to the dict oracle; the small constructed cases are compared with the
dict oracle (oracle/similar_oracle.py) as well.  Every comparison is exact:
ids, counts and the scores' bit patterns.
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import similar_oracle as O
from similar_cases import (SM_CAP, ExactSimilar, cut_ranges, synthetic_similar, to_dicts,
                           twin_pairs)

pytestmark = pytest.mark.gpu

M, U, CORE, PER_USER, SEED = 8300, 3000, 24, 40, 11   # 3 ranges, the last holds 108 movies
UBP = ctypes.POINTER(ctypes.c_ubyte)
ULLP = ctypes.POINTER(ctypes.c_ulonglong)


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def _finder(arrays, **kw):
    from movie_recommender_amd.similar import SimilarMovieFinder
    return SimilarMovieFinder.from_arrays(*arrays, **kw)


def _check_row(ex, f, q, nres, oj, os_, oc, what=""):
    """One query's output row against the restatement."""
    ids, scores, _, idx = ex.find(q, nres)
    c = int(oc)
    assert c == len(ids), (what, q, nres, c, len(ids))
    assert np.array_equal(oj[:c], idx.astype(np.int32)), (what, q, nres)
    assert np.array_equal(f._ids[oj[:c]], ids), (what, q, nres)
    assert np.array_equal(_bits(os_[:c]), _bits(scores)), (what, q, nres)


def _check_dict_oracle(dicts, f, q, nres, oj, os_, oc):
    genres, mr = dicts
    with np.errstate(all="ignore"):
        eids, escores = O.find_similar_movie(genres, mr, q, f.buff_limit, f.buff_point, nres)
    c = int(oc)
    assert c == len(eids), (q, nres)
    assert np.array_equal(f._ids[oj[:c]], np.asarray(eids, np.int64)), (q, nres)
    assert np.array_equal(_bits(os_[:c]), _bits(np.asarray(escores, np.float64))), (q, nres)


def _find_checked(arrays, ex, f, queries, nres, dict_oracle=False):
    oj, os_, oc = f.find_many(queries, nres)
    dicts = to_dicts(arrays) if dict_oracle else None
    for t, q in enumerate(queries):
        _check_row(ex, f, q, nres, oj[t], os_[t], oc[t])
        if dict_oracle:
            _check_dict_oracle(dicts, f, q, nres, oj[t], os_[t], oc[t])


@pytest.fixture(scope="module")
def big(gpu):
    """The 8,300-movie data set, its restatement, a live finder and the rows
    of all movies from one launch."""
    arrays = synthetic_similar(SEED, M, U, CORE, PER_USER)
    ex = ExactSimilar(arrays, 0.05, 100)
    with _finder(arrays) as f:
        rows = f.find_many(None, 20)
        yield SimpleNamespace(arrays=arrays, ex=ex, f=f, rows=rows)


def _compared_queries(arrays):
    _, off, _, _, _, _, has = arrays
    deg = np.diff(off)
    no_genres = int(np.flatnonzero((has == 0) & (deg >= 3))[0])
    no_raters = int(np.flatnonzero(deg == 0)[0])
    qs = list(range(CORE)) + [x for p in twin_pairs(M, CORE) for x in p]
    qs += [0, 4095, 4096, 4097, 8191, 8192, M - 1, no_genres, no_raters, CORE]
    qs += np.random.RandomState(2).choice(M, 66, replace=False).tolist()
    return list(dict.fromkeys(qs)), no_genres, no_raters


def test_multi_range_parity(big):
    """a. NR = 3 in one launch of all movies; then a shuffled subset with a
    repeated index gives the same rows."""
    arrays, ex, f = big.arrays, big.ex, big.f
    _, off, uid, _, n_users, _, _ = arrays
    assert n_users > int(uid.max()) + 1 and 0 not in uid      # users without ratings
    assert not np.all(np.diff(arrays[0]) > 0)                 # ids are not monotone
    qs, no_genres, no_raters = _compared_queries(arrays)
    assert 95 <= len(qs) <= 100
    oj, os_, oc = big.rows
    assert oj.shape == (M, 20) and oc.shape == (M,)
    for q in qs:
        _check_row(ex, f, q, 20, oj[q], os_[q], oc[q], "all movies")
    assert oc[no_genres] == 0 and oc[no_raters] == 0
    for a, b in twin_pairs(M, CORE):                          # twins find each other
        assert b in oj[a, :oc[a]] and a in oj[b, :oc[b]]
    assert ex.find(8200, 20)[2] > 1024                        # a popular movie of the last range

    sub = np.random.RandomState(3).permutation(qs)
    sub = np.concatenate([sub[:50], sub[7:8], sub[50:]])      # one index twice
    sj, ss, sc = f.find_many(sub, 20)
    for t, q in enumerate(sub.tolist()):
        c = int(oc[q])
        assert sc[t] == c, q
        assert np.array_equal(sj[t, :c], oj[q, :c]), q
        assert np.array_equal(_bits(ss[t, :c]), _bits(os_[q, :c])), q


def test_mid_stream_cut_runs(big):
    """b. By the kernel's rule (similar_cases.cut_ranges) the compared queries
    include lists cut mid-stream in two different ranges and lists that only
    take the final cut; all of them match."""
    arrays, ex, f = big.arrays, big.ex, big.f
    qs, _, _ = _compared_queries(arrays)
    cand = ex.candidates(qs)
    cuts = {q: cut_ranges(cand[q][0], M, 20) for q in qs}
    two_ranges = [q for q in qs if len(set(cuts[q][0])) >= 2]
    final_only = [q for q in qs if not cuts[q][0] and cuts[q][1]]
    print("mid-stream cuts per query:", {q: cuts[q][0] for q in qs if cuts[q][0]})
    print("final cut only:", {q: len(cand[q][0]) for q in final_only})
    assert len(two_ranges) >= 1 and len(final_only) >= 1
    assert max(cuts[q][2] for q in qs) <= SM_CAP
    oj, os_, oc = big.rows
    for q in two_ranges + final_only:
        _check_row(ex, f, q, 20, oj[q], os_[q], oc[q])
    _find_checked(arrays, ex, f, two_ranges[:4] + final_only[:4], 20)


def test_cut_threshold(big):
    """c. total == 20 * num_results (no cut, ordered by score then index)
    against total == 20 * num_results + 1 (cut, ordered by score, n, index)."""
    arrays, ex, f = big.arrays, big.ex, big.f
    cand = ex.candidates(range(400))
    at, above = [], []
    for q in range(400):
        total = len(cand[q][0])
        if total and total % 20 == 0 and total // 20 <= 51:
            at.append((q, total // 20))
        if total > 1 and (total - 1) % 20 == 0 and (total - 1) // 20 <= 51:
            above.append((q, (total - 1) // 20))
    print("total == T:", at, " total == T + 1:", above)
    assert len(at) >= 3 and len(above) >= 3
    for q, nres in at[:8] + above[:8]:
        _find_checked(arrays, ex, f, [q], nres)


def test_num_results_edges(big):
    """d. num_results 1 and 51 (T = 1020), every value for one core query,
    and the refusal of 0 and 52."""
    arrays, ex, f = big.arrays, big.ex, big.f
    qs = [0, 5, CORE, CORE + 1, 4095, 4096, 8200, 8192, M - 1]
    _find_checked(arrays, ex, f, qs, 1)
    _find_checked(arrays, ex, f, qs, 51)
    assert cut_ranges(ex.candidates([0])[0][0], M, 51)[0]     # cut mid-stream at T = 1020 too
    for nres in range(1, 52):
        _find_checked(arrays, ex, f, [7], nres)
    for bad in (0, 52):
        with pytest.raises(RuntimeError, match=r"num_results must be in 1\.\.51"):
            f.find_many([0], bad)
    _find_checked(arrays, ex, f, [0, CORE], 20)               # still usable


def _capacity_case(nres):
    """M = 4100; users 0-4 rated every movie of [0, 2048) and movie 3000 (6..10
    half-stars, varied), users 5-7 a few of them, users 8-9 nothing; one genre.
    The cut keeps by (n, index) whatever the scores are, so the last movie it
    keeps and the first it drops, for the queries 3000 and 5, then get the
    query's own ratings (cosine 1, the top score): a cut that is off by one in
    either direction changes the returned list.  Returns the arrays and, per
    query, (last kept, first dropped)."""
    Mc, T = 4100, 20 * nres
    ratings = [dict() for _ in range(Mc)]
    for u in range(5):
        for m in list(range(2048)) + [3000]:
            ratings[m][u] = 6 + (m * 7 + u * 3 + (m >> 4)) % 5
    extra = {5: list(range(0, 2048, 97)) + [3000],
             6: [5, 700, 1500, 2047, 3000],
             7: list(range(1020, 1101)) + [3000]}
    for u, ms in extra.items():
        for m in ms:
            ratings[m][u] = 6 + (m + u) % 5
    ids = (np.random.RandomState(1).permutation(Mc) * 2 + 5).astype(np.int64)

    def pack():
        return _arrays(ids, [list(r.items()) for r in ratings], 10, np.ones(Mc), np.ones(Mc))

    def same_as_query(m):
        for u, r in enumerate((10, 6, 10, 6, 10)):            # proportional to no other movie's
            ratings[m][u] = r

    same_as_query(3000)
    same_as_query(5)
    cand = ExactSimilar(pack(), 0.05, 100).candidates([3000, 5])
    edge = {}
    for q in (3000, 5):
        j, n, _ = cand[q]
        order = np.lexsort((j, -n))
        edge[q] = (int(j[order[T - 1]]), int(j[order[T]]))
    for m in {m for e in edge.values() for m in e} - {5, 3000}:
        same_as_query(m)
    return pack(), edge


@pytest.mark.parametrize("nres", [20, 51])
def test_list_capacity(gpu, nres):
    """e. Exactly SM_CAP = 2048 candidates held at the first cut (a sort of
    2048 with no padding), almost all n tied; and 2047 with the query at 5."""
    arrays, edge = _capacity_case(nres)
    ex = ExactSimilar(arrays, 0.05, 100)
    cand = ex.candidates([3000, 5])
    assert cut_ranges(cand[3000][0], 4100, nres) == ([0], True, 2048)
    assert cut_ranges(cand[5][0], 4100, nres) == ([0], True, 2047)
    assert len(set(cand[3000][1].tolist())) >= 3              # some n differ
    for q, (last_kept, first_dropped) in edge.items():        # the cut's edge is in view
        top = ex.find(q, nres)[3].tolist()
        assert last_kept in top and first_dropped not in top, (q, edge[q], top)
    with _finder(arrays) as f:
        _find_checked(arrays, ex, f, [3000, 5, 0, 2047, 2048], nres, dict_oracle=True)


def _field_case(n_raters):
    rs = np.random.RandomState(4)
    users = np.arange(n_raters, dtype=np.int32)
    mixed = rs.randint(1, 256, n_raters).astype(np.uint8)
    mixed[:16] = 255
    top = np.full(n_raters, 255, np.uint8)
    off = np.array([0, 1, 2, 3], np.int64) * n_raters
    return (np.array([30, 10, 20], np.int64), off,
            np.concatenate([users, users[::-1], rs.permutation(users)]),
            np.concatenate([top, top, mixed]), n_raters,
            np.array([1, 1, 3], np.uint64), np.ones(3, np.uint8))


def test_field_limits(gpu):
    """f. D, A and B at the top of their 32-bit fields (255^2 * 66,000 =
    4,291,650,000 < 2^32 - 1), B beside A in one word; one step further the
    library refuses."""
    from movie_recommender_amd import _lib
    arrays = _field_case(66_000)
    ex = ExactSimilar(arrays, 0.05, 100)
    assert int((ex.R[0] @ ex.RT).toarray()[0, 1]) == 255 * 255 * 66_000 > 2 ** 32 - 2 ** 22
    with _finder(arrays) as f:
        _find_checked(arrays, ex, f, [0, 1, 2], 20, dict_oracle=True)
        oj, _, oc = f.find_many(None, 20)
        assert oc.tolist() == [2, 2, 2] and oj[0, 0] == 1 and oj[1, 0] == 0

    over = _field_case(66_100)
    with pytest.raises(RuntimeError, match="would overflow 32-bit fields"):
        _finder(over)
    _, off, uid, r2, n_users, mask, has = over
    h = _lib.lib().mr_similar_create(0, 3, n_users, off.ctypes.data_as(_lib.LLP),
                                     uid.ctypes.data_as(_lib.IP), r2.ctypes.data_as(UBP),
                                     mask.ctypes.data_as(ULLP), has.ctypes.data_as(UBP))
    assert not h and "would overflow 32-bit fields" in _lib.last_error()
    with _finder(arrays) as f:                                # the library goes on working
        _find_checked(arrays, ex, f, [2], 20)


def _arrays(ids, lists, n_users, mask, has):
    """from_arrays inputs of per-movie [(user, rating2), ...] lists."""
    off = np.zeros(len(ids) + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in lists])
    uid = np.array([u for x in lists for u, _ in x], np.int32)
    r2 = np.array([r for x in lists for _, r in x], np.uint8)
    return (np.asarray(ids, np.int64), off, uid, r2, n_users, np.asarray(mask, np.uint64),
            np.asarray(has, np.uint8))


def test_degenerate_inputs(gpu):
    """g. No movies, one movie, no ratings; queries without genres or raters;
    zero ratings whose cosine is 0 / 0."""
    with _finder(_arrays([], [], 0, [], [])) as f:
        oj, os_, oc = f.find_many(None, 20)
        assert oj.shape == (0, 20) and os_.shape == (0, 20) and oc.shape == (0,)
    with _finder(_arrays([], [], 4, [], [])) as f:
        assert f.find_many(None, 5)[2].shape == (0,)
    with _finder(_arrays([9], [[(0, 7), (1, 8), (2, 9)]], 3, [1], [1])) as f:
        assert f.find_many(None, 20)[2].tolist() == [0]
        assert f.find_similar_movie(0) == ([], [])
    with _finder(_arrays([5, 4, 3, 2, 1], [[]] * 5, 3, [1] * 5, [1] * 5)) as f:
        assert f.find_many(None, 20)[2].tolist() == [0] * 5
        assert f.find_many([4, 0, 4], 1)[2].tolist() == [0] * 3

    four = [0, 1, 2, 3]
    lists = [[(u, 0) for u in four],                          # 0: only zero ratings
             [(u, r) for u, r in zip(four, (4, 6, 8, 2))],    # 1
             [(u, 0) for u in four[:3]],                      # 2: only zero ratings
             [(u, r) for u, r in zip(four, (5, 6, 9, 2))],    # 3: similar to 1
             [(u, r) for u, r in zip(four, (4, 6, 8, 3))],    # 4: no genres
             [],                                              # 5: no raters
             [(u, r) for u, r in zip(four, (0, 6, 8, 0))]]    # 6: some zero ratings
    arrays = _arrays([70, 60, 50, 40, 30, 20, 10], lists, 6, [1, 1, 1, 1, 0, 1, 1],
                     [1, 1, 1, 1, 0, 1, 1])
    ex = ExactSimilar(arrays, 0.05, 100)
    with _finder(arrays) as f:
        _find_checked(arrays, ex, f, list(range(7)), 20, dict_oracle=True)
        oc = f.find_many(None, 20)[2]
        assert oc.tolist() == [0, 2, 0, 2, 0, 0, 2]           # 0 / 0 is not > 0.3


def _raw_find(L, h, n_query, query, boost, nres, rows=None, n_boost=None):
    """mr_similar_find as given (output buffers of ``rows`` rows)."""
    from movie_recommender_amd import _lib
    rows = n_query if rows is None else rows
    oj = np.zeros((max(rows, 1), max(nres, 1)), np.int32)
    os_ = np.zeros((max(rows, 1), max(nres, 1)))
    oc = np.zeros(max(rows, 1), np.int32)
    q = None if query is None else np.ascontiguousarray(query, np.int32)
    boost = np.ascontiguousarray(boost, np.float64)
    rc = L.mr_similar_find(h, n_query, q.ctypes.data_as(_lib.IP) if q is not None else None,
                           boost.ctypes.data_as(_lib.DP),
                           len(boost) if n_boost is None else n_boost, nres,
                           oj.ctypes.data_as(_lib.IP), os_.ctypes.data_as(_lib.DP),
                           oc.ctypes.data_as(_lib.IP))
    return rc, oj, os_, oc


def test_c_api_refusals(big):
    """h. Every refusal of mr_similar_find on a live handle and of
    mr_similar_create returns an error and sets the message; the handle then
    still answers."""
    from movie_recommender_amd import _lib
    from movie_recommender_amd.similar import boost_table
    L, f = _lib.lib(), big.f
    boost = boost_table(0.05, 100, 10)
    for kw, msg in ((dict(n_query=M - 1, query=None), "query == NULL needs n_query == n_movies"),
                    (dict(n_query=2, query=[0, -1]), "query index out of range"),
                    (dict(n_query=2, query=[M, 0]), "query index out of range"),
                    (dict(n_query=1, query=[0], n_boost=0), "boost table is empty"),
                    (dict(n_query=1, query=[0], nres=0), "num_results must be in 1..51"),
                    (dict(n_query=1, query=[0], nres=52), "num_results must be in 1..51")):
        rc, _, _, _ = _raw_find(L, f._h, kw["n_query"], kw["query"], boost, kw.get("nres", 20),
                                rows=2, n_boost=kw.get("n_boost"))
        assert rc != 0 and msg in _lib.last_error(), (kw, rc, _lib.last_error())
    assert L.mr_similar_find(None, 0, None, None, 0, 20, None, None, None) != 0

    def create(off, uid, n_users, n_movies=3):
        off = np.asarray(off, np.int64)
        uid = np.asarray(uid, np.int32)
        r2 = np.full(max(len(uid), 1), 6, np.uint8)
        mask, has = np.ones(n_movies, np.uint64), np.ones(n_movies, np.uint8)
        return L.mr_similar_create(0, n_movies, n_users, off.ctypes.data_as(_lib.LLP),
                                   uid.ctypes.data_as(_lib.IP), r2.ctypes.data_as(UBP),
                                   mask.ctypes.data_as(ULLP), has.ctypes.data_as(UBP))

    for off, uid, n_users, msg in (([0, 3, 2, 5], [0, 1, 2, 3, 4], 5, "offsets must not decrease"),
                                   ([1, 2, 3, 4], [0, 1, 2, 3], 4, "bad offsets"),
                                   ([0, 2, 4, 5], [0, 1, 2, 5, 3], 5, "user index out of range"),
                                   ([0, 2, 4, 5], [0, 1, -1, 2, 3], 5, "user index out of range")):
        h = create(off, uid, n_users)
        assert not h and msg in _lib.last_error(), (off, uid, _lib.last_error())
    h = create([0, 2, 4, 5], [0, 1, 2, 4, 3], 5)              # the same call, valid: accepted
    assert h
    L.mr_similar_destroy(h)

    _find_checked(big.arrays, big.ex, f, [0, CORE, 4096, M - 1], 20)


def test_boost_clamp(big):
    """i. A boost table shorter than the largest n: boost[min(n, n_boost - 1)]."""
    from movie_recommender_amd import _lib
    table = np.array([1.0, 1.0, 1.0, 1.0, 1.125, 1.25, 1.375, 1.75])
    ex = ExactSimilar(big.arrays, boost=table)
    qs = [0, CORE, 4095, 4096, 8200, 300, 2000, M - 1]
    cand = ex.candidates(qs)
    ns = np.concatenate([cand[q][1] for q in qs])
    assert ns.max() > 1000 and ns.min() < 7                   # clamped and unclamped entries
    rc, oj, os_, oc = _raw_find(_lib.lib(), big.f._h, len(qs), qs, table, 20)
    assert rc == 0, _lib.last_error()
    for t, q in enumerate(qs):
        _check_row(ex, big.f, q, 20, oj[t], os_[t], oc[t], "clamp")
