"""The reference's tag-count recommender (``tag_count``) on the GPU.

Mirrors:

* ``TagCount_UserProfile`` -- ``python/app_local/models.py:24-336`` (identical
  in ``python/full_data/tag_count_predictor.py:6-239`` apart from
  ``get_param_list``): a per-user tag profile and genre profile, and two small
  least-squares models on the dot products of a movie with them;
* ``tag_count_eval``     -- ``python/full_data/worker_process.py:376-418``
  (``_tag_count_eval``): one batched fit and one evaluation for all test users;
* ``median_eval``        -- ``worker_process.py:344-372`` (``_median_eval``);
* ``TagCountTable``      -- the device-resident movie table all of them run
  on, with batched ``fit``, ``scores``, ``top_n`` and ``evaluate``.

Profiles, dot products, the rows that enter each system and the choice of the
model per movie are bit-equal to the reference; the two coefficient vectors
are the minimum-norm least-squares solutions with NumPy's rank rule, inside
the reference's own rounding spread; given the coefficients, scores, rankings
and agreement counts are exact (``include/mr_tagcount.h``).  There is no CPU
fallback: without the HIP library every entry point raises.
"""
import numpy as np

from . import _lib
from .content import TagTable
from .serving import ROTATION_SIZE, _dp, _ip, _llp

MAX_GENRES = 1024


class TagCountFit:
    """Models of a batch of users on one ``TagCountTable``:

    ``genre_dense`` f64[B, n_genres] (the genre profiles by genre index); the
    tag profiles as CSR (``tp_off`` int64[B + 1], ``tp_idx`` int32 ascending
    inside a user, ``tp_val`` f64, the values that are not 0); ``x0`` f64[B,
    3], ``x1`` f64[B, 2] with ``has0`` / ``has1``; from a fit also ``n0``
    (rows of A0), ``rank0``, ``rank1``.  ``tag_profile(u)`` and
    ``genre_profile(u)`` give user u's profiles as dictionaries."""

    def __init__(self, table, genre_profile, tp_off, tp_idx, tp_val, x0, x1, has0, has1,
                 n0=None, rank0=None, rank1=None):
        self.table = table
        self.has0 = np.ascontiguousarray(has0, np.int32)
        B = len(self.has0)
        self.has1 = np.ascontiguousarray(has1, np.int32)
        self.genre_dense = np.ascontiguousarray(genre_profile, np.float64).reshape(
            B, table.num_genres)
        self.tp_off = np.ascontiguousarray(tp_off, np.int64)
        self.tp_idx = np.ascontiguousarray(tp_idx, np.int32)
        self.tp_val = np.ascontiguousarray(tp_val, np.float64)
        self.x0 = np.ascontiguousarray(x0, np.float64).reshape(B, 3)
        self.x1 = np.ascontiguousarray(x1, np.float64).reshape(B, 2)
        self.n0, self.rank0, self.rank1 = n0, rank0, rank1

    def __len__(self):
        return len(self.has0)

    def x_factors0(self, u):
        """The reference's ``x_factors0`` of user u: shape (3, 1), or None."""
        return self.x0[u].reshape(3, 1).copy() if self.has0[u] else None

    def x_factors1(self, u):
        """The reference's ``x_factors1`` of user u: shape (2, 1), or None."""
        return self.x1[u].reshape(2, 1).copy() if self.has1[u] else None

    def tag_profile(self, u):
        """{tag id: value} of user u, the values that are not 0."""
        a, b = self.tp_off[u], self.tp_off[u + 1]
        return dict(zip(self.table.tag_ids[self.tp_idx[a:b]].tolist(), self.tp_val[a:b].tolist()))

    def genre_profile(self, u):
        """{genre id: value} of user u, the values that are not 0."""
        row = self.genre_dense[u]
        nz = np.nonzero(row)[0]
        return dict(zip(self.table.genre_ids[nz].tolist(), row[nz].tolist()))

    def _args(self):
        """The eight model arrays as the C ABI takes them (buffers of at
        least one element)."""
        one = lambda a, dt: a if a.size else np.zeros(1, dt)   # noqa: E731
        self._keep = (one(self.genre_dense, np.float64), self.tp_off, one(self.tp_idx, np.int32),
                      one(self.tp_val, np.float64), one(self.x0, np.float64),
                      one(self.x1, np.float64), one(self.has0, np.int32),
                      one(self.has1, np.int32))
        g, o, i, v, x0, x1, h0, h1 = self._keep
        return [_dp(g), _llp(o), _ip(i), _dp(v), _dp(x0), _dp(x1), _ip(h0), _ip(h1)]

    @staticmethod
    def from_models(table, models):
        """``[(tag_profile dict, genre_profile dict, x_factors0 or None,
        x_factors1 or None)]`` -- the reference's objects -- to a
        TagCountFit.  A profile member that is 0, or whose tag / genre no
        candidate of the table has, adds nothing to any score and is left
        out."""
        B = len(models)
        gp = np.zeros((B, table.num_genres))
        x0, x1 = np.zeros((B, 3)), np.zeros((B, 2))
        has0, has1 = np.zeros(B, np.int32), np.zeros(B, np.int32)
        off = np.zeros(B + 1, np.int64)
        idx, val = [], []
        for u, (tp, gpd, xf0, xf1) in enumerate(models):
            ent = sorted((table.tag_index[t], float(v)) for t, v in tp.items()
                         if t in table.tag_index and v != 0)
            idx += [i for i, _ in ent]
            val += [v for _, v in ent]
            off[u + 1] = len(idx)
            for g, v in gpd.items():
                if g in table.genre_index:
                    gp[u, table.genre_index[g]] = v
            for xf, x, has, n in ((xf0, x0, has0, 3), (xf1, x1, has1, 2)):
                if xf is not None:
                    xf = np.asarray(xf, np.float64).reshape(-1)
                    if len(xf) != n:
                        raise ValueError("x_factors0 has 3 coefficients and x_factors1 has 2")
                    x[u], has[u] = xf, 1
        return TagCountFit(table, gp, off, np.array(idx, np.int32), np.array(val, np.float64),
                           x0, x1, has0, has1)

    @staticmethod
    def no_models(table, B):
        """B users without any model: every prediction is the movie's median."""
        return TagCountFit(table, np.zeros((B, table.num_genres)), np.zeros(B + 1, np.int64),
                           np.zeros(0, np.int32), np.zeros(0), np.zeros((B, 3)),
                           np.zeros((B, 2)), np.zeros(B, np.int32), np.zeros(B, np.int32))


class TagCountTable:
    """The movie side of the tag-count model on one GPU.

    ``movie_genres`` ({movie id: set of genre ids}), ``movie_tags`` ({movie
    id: {tag id: ln(count) + 1}}), ``tag_counts`` ({tag id: count}),
    ``genre_counts`` ({genre id: count}) and ``movie_medians`` ({movie id:
    median}) are the reference's objects.  The movies ``predict`` can score --
    and a rating list may hold -- are those with a median, kept in
    ``movie_medians`` order.  A movie's tags are kept in ``movie_tags[m]``
    iteration order with their raw values and its genres in
    ``list(movie_genres[m])`` order as of now: the reference sums in these
    orders.  A tag or genre of such a movie without a count raises KeyError
    here (the reference raises it at first use)."""

    def __init__(self, movie_genres, movie_tags, tag_counts, genre_counts, movie_medians,
                 device=0):
        self.device = int(device)
        self.movie_medians = movie_medians
        mids = list(movie_medians)
        self.cand_mid = np.array(mids, np.int32)
        self.cand_med = np.array([movie_medians[m] for m in mids], np.float64)
        self.cand_index = {int(m): c for c, m in enumerate(mids)}
        self._cand_lut = np.full(int(self.cand_mid.max()) + 1 if mids else 1, -1, np.int32)
        self._cand_lut[self.cand_mid] = np.arange(len(mids), dtype=np.int32)
        glists = [list(movie_genres.get(m, ())) for m in mids]
        tlists = [list(movie_tags[m].items()) if m in movie_tags else [] for m in mids]
        self.genre_ids = np.array(sorted({g for l in glists for g in l}), np.int64)
        self.tag_ids = np.array(sorted({t for l in tlists for t, _ in l}), np.int64)
        if len(self.genre_ids) > MAX_GENRES:
            raise ValueError("at most 1024 distinct genres")
        self.genre_index = {int(g): i for i, g in enumerate(self.genre_ids)}
        self.tag_index = {int(t): i for i, t in enumerate(self.tag_ids)}
        self.genre_count = np.array([genre_counts[int(g)] for g in self.genre_ids], np.float64)
        self.tag_count = np.array([tag_counts[int(t)] for t in self.tag_ids], np.float64)
        for c in (self.genre_count, self.tag_count):
            if c.size and not (np.all(c > 0) and np.all(c < 2.0 ** 53)):
                raise ValueError("counts must be positive and below 2**53")
        self.genre_off = np.zeros(len(mids) + 1, np.int64)
        self.genre_off[1:] = np.cumsum([len(l) for l in glists])
        self.tag_off = np.zeros(len(mids) + 1, np.int64)
        self.tag_off[1:] = np.cumsum([len(l) for l in tlists])
        self.genre_idx = np.array([self.genre_index[g] for l in glists for g in l] or [0],
                                  np.int32)
        self.tag_idx = np.array([self.tag_index[t] for l in tlists for t, _ in l] or [0], np.int32)
        self.tag_val = np.array([v for l in tlists for _, v in l] or [0.0], np.float64)
        self._h = None

    # -- lifetime -----------------------------------------------------------
    def _handle(self):
        """The device table, uploaded at the first call that computes (the
        argument checks before it need no device)."""
        if self._h is None:
            one = lambda a: a if a.size else np.zeros(1)   # noqa: E731
            self._h = _lib.lib().mr_tagcount_create(
                self.device, self.num_candidates, _ip(self.cand_mid), _dp(self.cand_med),
                _llp(self.genre_off), _ip(self.genre_idx), _llp(self.tag_off), _ip(self.tag_idx),
                _dp(self.tag_val), self.num_genres, _dp(one(self.genre_count)), self.num_tags,
                _dp(one(self.tag_count)))
            if not self._h:
                raise RuntimeError("mr_tagcount_create failed: " + _lib.last_error())
        return self._h

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().mr_tagcount_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def num_candidates(self):
        return len(self.cand_mid)

    @property
    def num_genres(self):
        return len(self.genre_ids)

    @property
    def num_tags(self):
        return len(self.tag_ids)

    def kernel_ms(self):
        ms = np.zeros(8)
        _lib.check(_lib.lib().mr_tagcount_last_kernel_ms(self._handle(), _dp(ms)),
                   "mr_tagcount_last_kernel_ms")
        return dict(zip(["profile", "fit", "compact", "scatter", "scores", "exclude", "select",
                         "evaluate"], ms.tolist()))

    # rating lists: [[(movie id, rating)]] or a CSR triple, as TagTable takes them
    _lists_csr = TagTable._lists_csr

    # -- fit ------------------------------------------------------------------
    def fit(self, lists):
        """``TagCount_UserProfile.__init__`` for a batch of rating lists of
        any length (0 or 1 ratings give no model at all).  A movie without a
        median raises KeyError.  Returns a ``TagCountFit``."""
        off, c, r = self._lists_csr(lists, True)
        B = len(off) - 1
        cap = int(np.diff(self.tag_off)[c].sum()) if c.size else 0
        gp = np.zeros((B, self.num_genres))
        tp_off = np.zeros(B + 1, np.int64)
        tp_idx = np.zeros(max(cap, 1), np.int32)
        tp_val = np.zeros(max(cap, 1))
        x0, x1 = np.zeros((B, 3)), np.zeros((B, 2))
        ints = [np.zeros(max(B, 1), np.int32) for _ in range(5)]
        c = c if c.size else np.zeros(1, np.int32)
        r = r if r.size else np.zeros(1)
        _lib.check(_lib.lib().mr_tagcount_fit(
            self._handle(), B, _llp(off), _ip(c), _dp(r), _dp(gp if gp.size else np.zeros(1)),
            _llp(tp_off), _ip(tp_idx), _dp(tp_val), cap, _dp(x0 if B else np.zeros(3)),
            _dp(x1 if B else np.zeros(2)), *[_ip(a) for a in ints]), "mr_tagcount_fit")
        has0, has1, n0, rank0, rank1 = [a[:B] for a in ints]
        n = int(tp_off[-1])
        return TagCountFit(self, gp, tp_off, tp_idx[:n].copy(), tp_val[:n].copy(), x0, x1, has0,
                           has1, n0, rank0, rank1)

    # -- scoring ------------------------------------------------------------
    def scores(self, fit):
        """``predict`` of every candidate for each model of ``fit``: f64[B,
        num_candidates] (columns in ``cand_mid`` order)."""
        out = np.empty((len(fit), self.num_candidates))
        _lib.check(_lib.lib().mr_tagcount_scores(
            self._handle(), len(fit), *fit._args(), _dp(out if out.size else np.zeros(1))),
            "mr_tagcount_scores")
        return out

    def top_n(self, fit, rated=None, num_results=ROTATION_SIZE * 100):
        """``recommend.py:86-106`` per model: the first ``num_results`` movies
        by (score, movie id) descending that are not in ``rated[u]``.  Returns
        a list of ``[(score, movie_id)]``."""
        mids, sc, cnt = self.top_n_arrays(fit, rated, num_results)
        return [list(zip(sc[u, :cnt[u]].tolist(), mids[u, :cnt[u]].tolist()))
                for u in range(len(cnt))]

    def _exclusions(self, rated, B):
        """``rated`` (per-user movie-id containers, or a CSR pair) -> (offsets,
        candidate indices) of the movies the table knows."""
        if isinstance(rated, tuple) and len(rated) == 2 and isinstance(rated[0], np.ndarray):
            off = np.asarray(rated[0], np.int64)
            mids = np.asarray(rated[1], np.int64)
            if (off.shape != (B + 1,) or off[0] != 0 or np.any(np.diff(off) < 0)
                    or off[-1] != len(mids)):
                raise ValueError("rated offsets must be int64[B + 1], non-decreasing, from 0 to "
                                 "len(ids)")
            ok = (mids >= 0) & (mids < len(self._cand_lut))
            c = np.full(len(mids), -1, np.int32)
            c[ok] = self._cand_lut[mids[ok]]
            keep = c >= 0
            kept = np.concatenate([[0], np.cumsum(keep, dtype=np.int64)])
            return (np.ascontiguousarray(kept[off], np.int64),
                    np.ascontiguousarray(c[keep] if keep.any() else np.zeros(1, np.int32),
                                         np.int32))
        lists = [[self.cand_index[m] for m in r if m in self.cand_index] for r in rated]
        if len(lists) != B:
            raise ValueError("rated must hold one container per model")
        off = np.zeros(B + 1, np.int64)
        off[1:] = np.cumsum([len(l) for l in lists])
        flat = (np.concatenate([np.asarray(l, np.int32) for l in lists]) if off[-1]
                else np.zeros(1, np.int32))
        return off, np.ascontiguousarray(flat, np.int32)

    def top_n_arrays(self, fit, rated=None, num_results=ROTATION_SIZE * 100):
        """``top_n`` as arrays (movie ids int32[B, n], scores f64[B, n], count
        per user).  ``rated``: per-user movie-id containers, or a CSR pair
        ``(offsets int64[B + 1], movie_ids)``."""
        B, N = len(fit), int(num_results)
        if not 1 <= N <= 1024:
            raise ValueError("num_results must be in 1..1024")
        excl_off = excl = None
        if rated is not None:
            excl_off, excl = self._exclusions(rated, B)
        mids = np.zeros((max(B, 1), N), np.int32)
        sc = np.zeros((max(B, 1), N))
        cnt = np.zeros(max(B, 1), np.int32)
        _lib.check(_lib.lib().mr_tagcount_top_n(
            self._handle(), B, *fit._args(), _llp(excl_off) if excl_off is not None else None,
            _ip(excl) if excl is not None else None, N, _ip(mids), _dp(sc), _ip(cnt)),
            "mr_tagcount_top_n")
        return mids[:B], sc[:B], cnt[:B]

    # -- evaluation -----------------------------------------------------------
    def evaluate_fit(self, fit, test_lists):
        """``_test_model`` (``worker_process.py:231-258``) of model t on
        ``test_lists[t]``.  Returns a dict of arrays: agreement (NaN = None),
        n_agree, n_disagree, pred (per rating, NaN without a median), sse,
        n_pred."""
        off, c, r = self._lists_csr(test_lists, False)
        T = len(off) - 1
        if T != len(fit):
            raise ValueError("one test list per model")
        res = {n: np.zeros(max(T, 1)) for n in ("agreement", "sse")}
        for n in ("n_agree", "n_disagree", "n_pred"):
            res[n] = np.zeros(max(T, 1), np.int64)
        res["pred"] = np.zeros(max(1, off[-1]))
        c = c if c.size else np.zeros(1, np.int32)
        r = r if r.size else np.zeros(1)
        _lib.check(_lib.lib().mr_tagcount_evaluate(
            self._handle(), T, *fit._args(), _llp(off), _ip(c), _dp(r), _dp(res["agreement"]),
            _llp(res["n_agree"]), _llp(res["n_disagree"]), _dp(res["pred"]), _dp(res["sse"]),
            _llp(res["n_pred"])), "mr_tagcount_evaluate")
        res = {n: a[:T] for n, a in res.items() if n != "pred"} | {"pred": res["pred"][:off[-1]]}
        return res

    def evaluate(self, train_lists, test_lists):
        """Fit a model per ``train_lists[t]`` and evaluate it on
        ``test_lists[t]``; returns ``evaluate_fit``'s dict plus ``"fit"``."""
        fit = self.fit(train_lists)
        res = self.evaluate_fit(fit, test_lists)
        res["fit"] = fit
        return res


# --------------------------------------------------------------------------
# models.py:24-336 interface
# --------------------------------------------------------------------------
_TABLES = {}
MAX_CACHED_TABLES = 4


def tag_count_table_for(movie_genres, movie_tags, tag_counts, genre_counts, movie_medians,
                        device=0):
    """The ``TagCountTable`` of these reference objects, built once per
    process, as ``content.tag_table_for``: keyed on the identity of the five
    dictionaries, which are kept referenced and must not be mutated afterwards
    (build a ``TagCountTable`` yourself and pass ``table=`` otherwise).  At
    most ``MAX_CACHED_TABLES`` tables are kept; the least recently used one is
    closed."""
    objs = (movie_genres, movie_tags, tag_counts, genre_counts, movie_medians)
    key = tuple(id(o) for o in objs) + (int(device),)
    entry = _TABLES.pop(key, None)
    if entry is None:
        entry = (TagCountTable(*objs, device=device), objs)
        while len(_TABLES) >= MAX_CACHED_TABLES:
            _TABLES.pop(next(iter(_TABLES)))[0].close()
    _TABLES[key] = entry          # most recently used last
    return entry[0]


class TagCount_UserProfile:
    """Tag-count model of a single user (``models.py:24-336``).

    Same constructor arguments, attributes and methods as the reference, plus
    ``table``.  The keys of ``tag_profile`` / ``genre_profile`` -- members
    whose offsets cancelled to 0 included -- and their insertion order come
    from one host pass over this user's list; the values, both coefficient
    vectors and the predictions come from the GPU."""

    def __init__(self, movie_genres, movie_ratings, movie_tags, tag_counts, genre_counts,
                 movie_medians, genre_ids=None, tag_ids=None, table=None):
        self._table = table or tag_count_table_for(movie_genres, movie_tags, tag_counts,
                                                   genre_counts, movie_medians)
        self._genre_ids = genre_ids
        self._tag_ids = tag_ids
        movie_ratings = list(movie_ratings)
        self._fit = f = self._table.fit([movie_ratings])
        tp, gp = f.tag_profile(0), f.genre_profile(0)
        self.tag_profile, self.genre_profile = {}, {}
        for movie_id, rating in movie_ratings:
            if rating - 3 != 0:
                for t in movie_tags.get(movie_id, ()):
                    self.tag_profile.setdefault(t, tp.get(t, 0.0))
                for g in movie_genres.get(movie_id, ()):
                    self.genre_profile.setdefault(g, gp.get(g, 0.0))
        self.x_factors0 = f.x_factors0(0)
        self.x_factors1 = f.x_factors1(0)
        self._scores = None

    def is_valid(self):
        return True

    def predict(self, movie_id):
        """Predicted rating, or None without a median (``models.py:218-262``)."""
        c = self._table.cand_index.get(movie_id)
        if c is None:
            return None
        if self._scores is None:
            self._scores = self._table.scores(self._fit)[0]
        return float(self._scores[c])

    def get_param_list(self):
        """``models.py:265-336``: the top 100 of the tag profile and the genre
        profile by value descending, then both coefficient vectors, each
        under a ``__comment`` heading."""
        if self._genre_ids is None or self._tag_ids is None:
            return []
        genre_names = {i: n for n, i in self._genre_ids.items()}
        tag_names = {i: n for n, i in self._tag_ids.items()}
        out = []
        tags = [(tag_names[t], v) for t, v in self.tag_profile.items()]
        if tags:
            tags.sort(key=lambda e: e[1], reverse=True)
            out.append(("__comment", "Tag Profile (Top 100)"))
            out += tags[:100]
        genres = [(genre_names[g], v) for g, v in self.genre_profile.items()]
        if genres:
            genres.sort(key=lambda e: e[1], reverse=True)
            out.append(("__comment", "Genre Profile"))
            out += genres
        if self.x_factors0 is not None:
            out.append(("__comment", "For Movies with Tags"))
            out += [("tag importance", self.x_factors0[0][0]),
                    ("genre importance", self.x_factors0[1][0]),
                    ("user bias", self.x_factors0[2][0])]
        if self.x_factors1 is not None:
            out.append(("__comment", "For Movies without Tags"))
            out += [("genre importance", self.x_factors1[0][0]),
                    ("user bias", self.x_factors1[1][0])]
        return out


def _agreements(user_ratings_test, res, return_stats):
    out = [(uid, float(a)) for (uid, _), a in zip(user_ratings_test, res["agreement"])
           if not np.isnan(a)]
    return (out, res) if return_stats else out


def tag_count_eval(user_ratings_train, user_ratings_test, movie_genres, movie_tags, tag_counts,
                   genre_counts, movie_medians_train, device=0, table=None, return_stats=False):
    """``_tag_count_eval``: both arguments are ``[(user_id, [(movie_id,
    rating)])]``, aligned; returns ``[(user_id, agreement)]`` for the users
    with an agreement, in input order -- one batched fit and one evaluation."""
    own = table is None
    if own:
        table = TagCountTable(movie_genres, movie_tags, tag_counts, genre_counts,
                              movie_medians_train, device)
    try:
        res = table.evaluate([l for _, l in user_ratings_train],
                             [l for _, l in user_ratings_test])
    finally:
        if own:
            table.close()
    return _agreements(user_ratings_test, res, return_stats)


def median_eval(user_ratings_test, movie_medians_train, device=0, table=None,
                return_stats=False):
    """``_median_eval``: every prediction is the movie's training median.
    ``user_ratings_test`` is ``[(user_id, [(movie_id, rating)])]``; returns
    ``[(user_id, agreement)]`` for the users with an agreement -- the same
    evaluation as ``tag_count_eval`` with no model for anyone.

    The reference raises ``IndexError`` for a user none of whose test movies
    has a median; here that user simply has no agreement."""
    own = table is None
    if own:
        table = TagCountTable({}, {}, {}, {}, movie_medians_train, device)
    try:
        res = table.evaluate_fit(TagCountFit.no_models(table, len(user_ratings_test)),
                                 [l for _, l in user_ratings_test])
    finally:
        if own:
            table.close()
    return _agreements(user_ratings_test, res, return_stats)
