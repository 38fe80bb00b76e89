"""Decoding of the similar-movies fixtures (tests/golden/similar_*.npz), a
seeded generator of ``SimilarMovieFinder.from_arrays`` inputs for cases larger
than the fixtures, and an exact, vectorised restatement of the search for
them (pinned to the fixtures and to oracle/similar_oracle.py by
tests/test_similar_oracle.py)."""
import numpy as np

from conftest import load_golden

SM_RS = 4096     # csrc/similar.hip: movies per accumulation range
SM_NT = 1024     #                   movies per candidate chunk (threads per query)
SM_CAP = 2048    #                   capacity of the LDS candidate list


def fixture(name):
    d = load_golden(f"similar_{name}.npz")
    o = d["off"]
    users, ratings = d["users"].tolist(), d["ratings"].tolist()
    d["movie_ratings"] = [(int(m), dict(zip(users[o[i]:o[i + 1]], ratings[o[i]:o[i + 1]])))
                          for i, m in enumerate(d["movie_ids"])]
    g = d["g_off"]
    vals = d["g_vals"].tolist()
    d["genres"] = {int(k): set(vals[g[i]:g[i + 1]]) for i, k in enumerate(d["g_keys"])}
    return d


def expected(d, nres):
    c = d[f"n{nres}_count"]
    out, o = [], 0
    for n in c:
        out.append((tuple(d[f"n{nres}_ids"][o:o + n].tolist()),
                    tuple(d[f"n{nres}_scores"][o:o + n].tolist())))
        o += n
    return out


def fixture_arrays(d):
    """The ``from_arrays`` inputs of a decoded fixture (dense user indices in
    order of first appearance, genre id = bit number)."""
    users = {}
    uid = np.array([users.setdefault(u, len(users)) for u in d["users"].tolist()], np.int32)
    r2 = np.round(2 * d["ratings"]).astype(np.uint8)
    assert np.array_equal(r2 / 2.0, d["ratings"])
    M = len(d["movie_ids"])
    mask, has = np.zeros(M, np.uint64), np.zeros(M, np.uint8)
    for m, mid in enumerate(d["movie_ids"].tolist()):
        if mid in d["genres"]:
            has[m] = 1
            mask[m] = sum(1 << g for g in d["genres"][mid])
    return (d["movie_ids"].astype(np.int64), d["off"].astype(np.int64), uid, r2, len(users),
            mask, has)


# ---------------------------------------------------------------------------
# synthetic from_arrays inputs
# ---------------------------------------------------------------------------
def twin_pairs(M, core):
    """(a, b) index pairs that ``synthetic_similar`` makes bit-identical (b
    gets a's raters, ratings and genres): across the first range boundary, a
    core movie with one of the third range, and two core movies."""
    pairs = [(4095, 4096), (10, 8200), (2, core - 3)]
    return [(a, b) for a, b in pairs if a < b < M]


def synthetic_similar(seed, M, U, core, per_user, n_genres=6, p_core=0.6, p_no_genres=0.03,
                      p_idle=0.02, no_raters=(33, 4097)):
    """Seeded ``SimilarMovieFinder.from_arrays`` inputs ``(movie_ids, off,
    user_index, rating2, n_users, genre_mask, has_genres)``: power-law
    popularity by index, a core of the first ``core`` movies that about
    ``p_core`` of the users rated, half-star ratings ``rating2`` in 1..10 from
    a small taste model, 1-2 genre bits out of ``n_genres``, about
    ``p_no_genres`` of the movies without genres, users without any rating
    (user 0, the last five and about ``p_idle`` of the rest, so ``n_users``
    exceeds the largest index + 1), movies without raters (``no_raters`` and
    whatever the tail leaves empty), the ``twin_pairs`` and movie ids that are
    a permutation (an index returned as an id is wrong almost everywhere).
    Within a movie the raters are in no particular order."""
    rs = np.random.RandomState(seed)
    movie_ids = (rs.permutation(M) * 3 + 11).astype(np.int64)
    pop = 1.0 / (1 + np.arange(M)) ** 0.7
    pop /= pop.sum()
    taste = rs.normal(0, 1, (U, 3))
    prof = rs.normal(0, 1, (M, 3))
    idle = rs.random_sample(U) < p_idle
    idle[0] = True
    idle[U - 5:] = True
    ratings = [dict() for _ in range(M)]          # movie -> {user: rating2}
    for u in np.flatnonzero(~idle).tolist():
        n = int(min(M // 2, max(3, rs.lognormal(np.log(per_user) - 0.32, 0.8))))
        ms = set(rs.choice(M, n, replace=False, p=pop).tolist())
        if rs.random_sample() < p_core:
            ms |= set(range(core))
        ms = sorted(ms)
        x = 3 + prof[ms] @ taste[u] + rs.normal(0, 0.7, len(ms))
        for m, v in zip(ms, np.clip(np.round(2 * x), 1, 10).astype(int).tolist()):
            ratings[m][u] = v
    for m in no_raters:
        if m < M:
            ratings[m] = {}
    has = (rs.random_sample(M) >= p_no_genres).astype(np.uint8)
    has[:core] = 1
    bits = rs.randint(0, n_genres, (M, 2))
    two = rs.random_sample(M) < 0.5
    mask = (1 << bits[:, 0]) | np.where(two, 1 << bits[:, 1], 0)
    active = np.flatnonzero(~idle)
    for a, b in twin_pairs(M, core):
        for u in rs.choice(active, 12, replace=False).tolist():   # tail movies: enough raters
            ratings[a].setdefault(u, int(rs.randint(1, 11)))
        ratings[b] = dict(ratings[a])
        has[a] = has[b] = 1
        mask[b] = mask[a]
    mask = np.where(has != 0, mask, 0).astype(np.uint64)
    off = np.zeros(M + 1, np.int64)
    uid, r2 = [], []
    for m in range(M):
        us = list(ratings[m])
        us = [us[t] for t in rs.permutation(len(us))]
        uid += us
        r2 += [ratings[m][u] for u in us]
        off[m + 1] = len(uid)
    return (movie_ids, off, np.asarray(uid, np.int32), np.asarray(r2, np.uint8), U, mask, has)


def to_dicts(arrays):
    """``(movie_genres, movie_ratings)`` of from_arrays inputs, as
    oracle/similar_oracle.py and the reference take them (genre ids = bit
    numbers, user ids = user indices, ratings = rating2 / 2)."""
    ids, off, uid, r2, _, mask, has = arrays
    uid, r = np.asarray(uid).tolist(), (np.asarray(r2) / 2.0).tolist()
    mr = [(int(ids[m]), dict(zip(uid[off[m]:off[m + 1]], r[off[m]:off[m + 1]])))
          for m in range(len(ids))]
    genres = {int(ids[m]): {b for b in range(64) if (int(mask[m]) >> b) & 1}
              for m in range(len(ids)) if has[m]}
    return genres, mr


# ---------------------------------------------------------------------------
# exact restatement on sparse integer matrices
# ---------------------------------------------------------------------------
def _popcount(x):
    x = np.ascontiguousarray(x, np.uint64)
    return np.unpackbits(x.view(np.uint8).reshape(x.shape + (8,)), axis=-1).sum(-1).astype(np.int64)


class ExactSimilar:
    """The reference's search on from_arrays inputs.  Per query i and movie j
    the integer sums over their common raters, n = P P^T, D = R R^T,
    A = R^2 P^T (the query's squares), B = P (R^2)^T, are exact int64 sparse
    products (R = rating2, P = its pattern), and the score is the fp64
    expression of csrc/similar.hip, ``(D/4) / (sqrt(A/4) sqrt(B/4)) * boost[n]``:
    with exact sums the value of the reference's ``dot / (norm * norm)``.
    ``boost`` defaults to ``similar.boost_table``; a given table is indexed by
    ``min(n, len - 1)`` as the C API does."""

    def __init__(self, arrays, buff_limit=0.05, buff_point=100, boost=None):
        import scipy.sparse as sp
        from movie_recommender_amd.similar import boost_table
        ids, off, uid, r2, U, mask, has = arrays
        self.ids = np.asarray(ids, np.int64)
        M = self.M = len(self.ids)
        self.mask = np.asarray(mask, np.uint64)[:M]
        self.has = np.asarray(has)[:M] != 0
        deg = np.diff(np.asarray(off, np.int64)) if M else np.zeros(0, np.int64)
        nnz = int(off[M])
        rows = np.repeat(np.arange(M), deg)
        uid = np.asarray(uid, np.int64)[:nnz]
        r = np.asarray(r2)[:nnz].astype(np.int64)

        def mat(v):
            return sp.csr_matrix((v, (rows, uid)), shape=(M, max(int(U), 1)), dtype=np.int64)
        self.P, self.R, self.R2 = mat(np.ones(nnz, np.int64)), mat(r), mat(r * r)
        self.PT, self.RT, self.R2T = (x.T.tocsr() for x in (self.P, self.R, self.R2))
        if boost is None:
            boost = boost_table(buff_limit, buff_point, max(int(deg.max()) if M else 0, 3))
        self.boost = np.asarray(boost, np.float64)
        self._cand = {}

    def candidates(self, queries):
        """{q: (index, n, score)} of the movies that pass every filter (n >= 3,
        genres on both sides, the genre gate, j != q, score > 0.3), in index
        order.  Cached per query."""
        todo = [int(q) for q in dict.fromkeys(int(q) for q in queries) if int(q) not in self._cand]
        pc = _popcount(self.mask)
        for s in range(0, len(todo), 64):
            qs = np.asarray(todo[s:s + 64])
            n = (self.P[qs] @ self.PT).toarray()
            D = (self.R[qs] @ self.RT).toarray()
            A = (self.R2[qs] @ self.PT).toarray()
            B = (self.P[qs] @ self.R2T).toarray()
            with np.errstate(all="ignore"):
                score = ((D * 0.25) / (np.sqrt(A * 0.25) * np.sqrt(B * 0.25))
                         * self.boost[np.minimum(n, len(self.boost) - 1)])
            common = _popcount(self.mask[qs][:, None] & self.mask[None, :])
            gate = 2 * common >= np.minimum(pc[qs][:, None], pc[None, :])
            ok = (n >= 3) & self.has[qs][:, None] & self.has[None, :] & gate & (score > 0.3)
            ok[np.arange(len(qs)), qs] = False
            for t, q in enumerate(qs.tolist()):
                j = np.flatnonzero(ok[t])
                self._cand[q] = (j, n[t, j], score[t, j])
        return {int(q): self._cand[int(q)] for q in queries}

    def find(self, q, num_results=20):
        """(movie ids, scores, total candidates, list indices) of query q in
        the order of the reference's stable sorts: with more than
        20 * num_results candidates, the first 20 * num_results by (n desc,
        index) ordered by (score desc, n desc, index); else (score desc,
        index)."""
        j, n, s = self.candidates([q])[int(q)]
        total, T = len(j), 20 * num_results
        if total > T:
            keep = np.lexsort((j, -n))[:T]
            j, n, s = j[keep], n[keep], s[keep]
            order = np.lexsort((j, -n, -s))
        else:
            order = np.lexsort((j, -s))
        order = order[:num_results]
        return self.ids[j[order]], s[order], total, j[order]


def exact_similar(arrays, queries, buff_limit=0.05, buff_point=100, num_results=20):
    """Per query: (movie ids, scores, total) by ``ExactSimilar``."""
    ex = ExactSimilar(arrays, buff_limit, buff_point)
    ex.candidates(queries)
    return [ex.find(q, num_results)[:3] for q in queries]


def cut_ranges(cand_index, M, num_results):
    """The accumulation ranges in which csrc/similar.hip cuts the candidate
    list of one query mid-stream, and whether the final cut runs.  The
    kernel's rule: per chunk of SM_NT movies (SM_RS / SM_NT chunks in each of
    the ceil(M / SM_RS) ranges) it cuts when held + SM_NT > SM_CAP, after
    which held = min(held, 20 * num_results); then the chunk's candidates are
    appended.  Also returns the largest list length at any cut."""
    T = 20 * num_results
    per = SM_RS // SM_NT
    nchunk = -(-M // SM_RS) * per
    cnt = np.bincount(np.asarray(cand_index, np.int64) // SM_NT, minlength=nchunk)
    held, cuts, peak = 0, [], 0
    for c in range(nchunk):
        if held + SM_NT > SM_CAP:
            cuts.append(c // per)
            peak = max(peak, held)
            held = min(held, T)
        held += int(cnt[c])
        assert held <= SM_CAP
    return cuts, len(cand_index) > T, peak
