"""The reference's tag least-squares recommender (``tag_ls``) on the GPU.

Mirrors:

* ``TagLS_UserProfile`` -- ``python/app_local/models.py:342-640`` (identical in
  ``python/full_data/tag_ls_predictor.py``): a per-user profile of the most
  frequent genre / tag ids of its rating list and the coefficients
  ``scipy.sparse.linalg.lsqr`` returns for them;
* ``tag_ls_eval``       -- ``python/full_data/worker_process.py:421-461``
  (``_tag_ls_eval``): one batched fit and one evaluation for all test users;
* ``TagTable``          -- the device-resident feature table both run on, with
  batched ``fit``, ``scores``, ``top_n`` and ``evaluate``.

The model is LSQR's iterate at its own stopping test (``atol`` ends it after
a few dozen steps, far from the least-squares solution), so the fit runs LSQR
itself in fp64 with SciPy's stopping rules (``include/mr_content.h``).  Given
the coefficients, scores, rankings and agreement counts are exact.  There is
no CPU fallback: without the HIP library every entry point raises.
"""
import numpy as np

from . import _lib
from .serving import ROTATION_SIZE, _dp, _ip, _llp

MAX_FACTORS = 25          # _decide_num_factors' cap
ROW = MAX_FACTORS + 1     # coefficients, then the bias
TAG_OFFSET = 1000         # models.py:408: a tag id is counted as tag id + 1000


def decide_num_factors(num_ratings):
    """``_decide_num_factors`` (``models.py:416-442``)."""
    n, nf, width, mult = int(num_ratings), 0, 10, 2
    for _ in range(5):
        if n <= width:
            return nf + n // mult
        nf += 5
        n -= width
        width *= 2
        mult *= 2
    return nf


class TagFit:
    """Models of a batch of users: ``p`` int32[B], ``profile`` int32[B, 25]
    (-1 past ``p``), ``x`` f64[B, 26] (``x[u, :p]`` the coefficients,
    ``x[u, p]`` the bias), ``itn`` / ``istop`` of LSQR."""

    def __init__(self, p, profile, x, itn=None, istop=None):
        self.p = np.ascontiguousarray(p, np.int32)
        B = len(self.p)
        self.profile = np.ascontiguousarray(profile, np.int32).reshape(B, MAX_FACTORS)
        self.x = np.ascontiguousarray(x, np.float64).reshape(B, ROW)
        self.itn = itn
        self.istop = istop

    def __len__(self):
        return len(self.p)

    def x_factors(self, u):
        """The reference's ``x_factors`` of user u: shape (p + 1, 1)."""
        return self.x[u, :self.p[u] + 1].reshape(-1, 1).copy()

    def profile_list(self, u):
        return self.profile[u, :self.p[u]].tolist()

    @staticmethod
    def from_models(models):
        """``[(profile list, x_factors)]`` -> TagFit."""
        B = len(models)
        p = np.zeros(B, np.int32)
        prof = np.full((B, MAX_FACTORS), -1, np.int32)
        x = np.zeros((B, ROW))
        for u, (pr, xf) in enumerate(models):
            xf = np.asarray(xf, np.float64).reshape(-1)
            if len(pr) > MAX_FACTORS or len(xf) != len(pr) + 1 or len(set(pr)) != len(pr):
                raise ValueError("a model is a profile of at most 25 distinct ids and "
                                 "len(profile) + 1 coefficients")
            p[u] = len(pr)
            prof[u, :len(pr)] = pr
            x[u, :len(xf)] = xf
        return TagFit(p, prof, x)


class TagTable:
    """The movie side of the content model on one GPU.

    ``movie_genres`` ({movie id: set of genre ids}), ``movie_tags`` ({movie
    id: {tag id: ln(count) + 1}}), ``tag_counts`` ({tag id: count}) and
    ``movie_medians`` ({movie id: median}) are the reference's objects.  The
    movies ``predict`` can score -- and a rating list may hold -- are those
    with a median, kept in ``movie_medians`` order.  A tag's value
    ``movie_tags[m][t] / tag_counts[t]`` is divided here once, as the same
    Python division the reference does per use."""

    def __init__(self, movie_genres, movie_tags, tag_counts, movie_medians, device=0):
        self.device = int(device)
        self.movie_medians = movie_medians
        mids = list(movie_medians)
        self.cand_mid = np.array(mids, np.int32)
        self.cand_med = np.array([movie_medians[m] for m in mids], np.float64)
        self.cand_index = {int(m): c for c, m in enumerate(mids)}
        self._cand_lut = np.full(int(self.cand_mid.max()) + 1 if mids else 1, -1, np.int32)
        self._cand_lut[self.cand_mid] = np.arange(len(mids), dtype=np.int32)
        off = np.zeros(len(mids) + 1, np.int64)
        ids, vals = [], []
        for c, m in enumerate(mids):
            feats = [(int(g), 1.0) for g in movie_genres.get(m, ())]
            for g, _ in feats:
                if not 0 <= g < TAG_OFFSET:
                    raise ValueError("genre ids must be in 0..999")
            tags = movie_tags.get(m)
            if tags:
                feats += [(int(t) + TAG_OFFSET, tags[t] / tag_counts[t]) for t in tags]
            feats.sort()
            ids += [f for f, _ in feats]
            vals += [v for _, v in feats]
            off[c + 1] = len(ids)
        self.feat_off = off
        self.feat_id = np.array(ids if ids else [0], np.int32)
        self.feat_val = np.array(vals if vals else [0.0], np.float64)
        self._h = None

    # -- lifetime -----------------------------------------------------------
    def _handle(self):
        """The device table, uploaded at the first call that computes (the
        argument checks before it need no device)."""
        if self._h is None:
            self._h = _lib.lib().mr_content_create(
                self.device, self.num_candidates, _ip(self.cand_mid), _dp(self.cand_med),
                _llp(self.feat_off), _ip(self.feat_id), _dp(self.feat_val))
            if not self._h:
                raise RuntimeError("mr_content_create failed: " + _lib.last_error())
        return self._h

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().mr_content_destroy(self._h)
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

    def kernel_ms(self):
        ms = np.zeros(6)
        _lib.check(_lib.lib().mr_content_last_kernel_ms(self._handle(), _dp(ms)),
                   "mr_content_last_kernel_ms")
        return dict(zip(["profile", "fit", "scores", "exclude", "select", "evaluate"],
                        ms.tolist()))

    # -- rating lists ---------------------------------------------------------
    def _lists_csr(self, lists, need_median):
        """``[[(movie id, rating)]]`` or a CSR triple ``(offsets int64[B + 1],
        movie ids, ratings)`` -> (offsets, candidate index, ratings).  A movie
        without a median raises KeyError when ``need_median`` (the reference's
        ``movie_medians[movie_id]``), else its index is -1."""
        if isinstance(lists, tuple) and len(lists) == 3 and isinstance(lists[0], np.ndarray):
            off = np.ascontiguousarray(lists[0], np.int64)
            mids = np.asarray(lists[1], np.int64)
            r = np.ascontiguousarray(lists[2], np.float64)
            if (off.ndim != 1 or len(off) < 1 or off[0] != 0 or np.any(np.diff(off) < 0)
                    or off[-1] != len(mids) or len(mids) != len(r)):
                raise ValueError("offsets must be int64[B + 1], non-decreasing, from 0 to "
                                 "len(movie ids) == len(ratings)")
        else:
            # one conversion per list, no Python loop over ratings (movie ids
            # pass through fp64, exact below 2**53)
            off = np.zeros(len(lists) + 1, np.int64)
            off[1:] = np.cumsum([len(l) for l in lists])
            rows = [np.asarray(l, np.float64).reshape(-1, 2) for l in lists if len(l)]
            flat = np.concatenate(rows) if rows else np.zeros((0, 2))
            mids = flat[:, 0].astype(np.int64)
            r = np.ascontiguousarray(flat[:, 1])
        ok = (mids >= 0) & (mids < len(self._cand_lut))
        c = np.full(len(mids), -1, np.int32)
        c[ok] = self._cand_lut[mids[ok]]
        if need_median and np.any(c < 0):
            raise KeyError(int(mids[np.argmax(c < 0)]))
        return off, c, r

    # -- fit ------------------------------------------------------------------
    def fit(self, lists, atol=1e-6, btol=1e-6, conlim=1e8, iter_lim=1000):
        """``TagLS_UserProfile.__init__`` for a batch of rating lists (each at
        least 2 ratings; the reference raises on a single one).  ``iter_lim``
        is a scalar or one value per list.  Returns a ``TagFit``."""
        off, c, r = self._lists_csr(lists, True)
        B = len(off) - 1
        if B and np.diff(off).min() < 2:
            raise ValueError("a rating list needs at least 2 ratings")
        each = None
        if np.ndim(iter_lim):
            each = np.ascontiguousarray(iter_lim, np.int32)
            if each.shape != (B,):
                raise ValueError("iter_lim must be a scalar or one value per list")
            iter_lim = 0
        p = np.zeros(B, np.int32)
        prof = np.full((B, MAX_FACTORS), -1, np.int32)
        x = np.zeros((B, ROW))
        itn = np.zeros(B, np.int32)
        istop = np.zeros(B, np.int32)
        c = c if c.size else np.zeros(1, np.int32)
        r = r if r.size else np.zeros(1)
        _lib.check(_lib.lib().mr_content_fit(
            self._handle(), B, _llp(off), _ip(c), _dp(r), float(atol), float(btol), float(conlim),
            int(iter_lim), _ip(each) if each is not None else None, _ip(p), _ip(prof), _dp(x),
            _ip(itn), _ip(istop)), "mr_content_fit")
        return TagFit(p, prof, x, itn, istop)

    # -- scoring ------------------------------------------------------------
    def scores(self, fit):
        """``predict`` of every candidate for each model of ``fit``: f64[B,
        num_candidates] (columns in ``cand_mid`` order)."""
        out = np.empty((len(fit), self.num_candidates))
        _lib.check(_lib.lib().mr_content_scores(self._handle(), len(fit), _ip(fit.p), _ip(fit.profile),
                                                _dp(fit.x), _dp(out)), "mr_content_scores")
        return out

    def top_n(self, fit, rated=None, num_results=ROTATION_SIZE * 100):
        """``recommend.py:86-106`` per model: the first ``num_results`` movies
        by (score, movie id) descending that are not in ``rated[u]``.  Returns
        a list of ``[(score, movie_id)]``."""
        mids, sc, cnt = self.top_n_arrays(fit, rated, num_results)
        return [list(zip(sc[u, :cnt[u]].tolist(), mids[u, :cnt[u]].tolist()))
                for u in range(len(cnt))]

    def top_n_arrays(self, fit, rated=None, num_results=ROTATION_SIZE * 100):
        """``top_n`` as arrays (movie ids int32[B, n], scores f64[B, n], count
        per user).  ``rated``: per-user movie-id containers, or a CSR pair
        ``(offsets int64[B + 1], movie_ids)``."""
        B, N = len(fit), int(num_results)
        if not 1 <= N <= 1024:
            raise ValueError("num_results must be in 1..1024")
        excl_off = excl = None
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
            excl_off = np.ascontiguousarray(kept[off], np.int64)
            excl = np.ascontiguousarray(c[keep] if keep.any() else np.zeros(1, np.int32), np.int32)
        elif rated is not None:
            lists = [[self.cand_index[m] for m in r if m in self.cand_index] for r in rated]
            if len(lists) != B:
                raise ValueError("rated must hold one container per model")
            excl_off = np.zeros(B + 1, np.int64)
            excl_off[1:] = np.cumsum([len(l) for l in lists])
            excl = np.ascontiguousarray(np.concatenate([np.asarray(l, np.int32) for l in lists])
                                        if excl_off[-1] else np.zeros(1, np.int32), np.int32)
        mids = np.zeros((B, N), np.int32)
        sc = np.zeros((B, N))
        cnt = np.zeros(B, np.int32)
        _lib.check(_lib.lib().mr_content_top_n(
            self._handle(), B, _ip(fit.p), _ip(fit.profile), _dp(fit.x),
            _llp(excl_off) if excl_off is not None else None,
            _ip(excl) if excl is not None else None, N, _ip(mids), _dp(sc), _ip(cnt)),
            "mr_content_top_n")
        return mids, sc, cnt

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
        res = {n: np.zeros(T) for n in ("agreement", "sse")}
        for n in ("n_agree", "n_disagree", "n_pred"):
            res[n] = np.zeros(T, np.int64)
        res["pred"] = np.zeros(max(1, off[-1]))
        c = c if c.size else np.zeros(1, np.int32)
        r = r if r.size else np.zeros(1)
        _lib.check(_lib.lib().mr_content_evaluate(
            self._handle(), T, _ip(fit.p), _ip(fit.profile), _dp(fit.x), _llp(off), _ip(c), _dp(r),
            _dp(res["agreement"]), _llp(res["n_agree"]), _llp(res["n_disagree"]),
            _dp(res["pred"]), _dp(res["sse"]), _llp(res["n_pred"])), "mr_content_evaluate")
        res["pred"] = res["pred"][:off[-1]]
        return res

    def evaluate(self, train_lists, test_lists, **fit_args):
        """Fit a model per ``train_lists[t]`` and evaluate it on
        ``test_lists[t]``; returns ``evaluate_fit``'s dict plus ``"fit"``."""
        fit = self.fit(train_lists, **fit_args)
        res = self.evaluate_fit(fit, test_lists)
        res["fit"] = fit
        return res


# --------------------------------------------------------------------------
# models.py:342-640 interface
# --------------------------------------------------------------------------
_TABLES = {}
MAX_CACHED_TABLES = 4


def tag_table_for(movie_genres, movie_tags, tag_counts, movie_medians, device=0):
    """The ``TagTable`` of these reference objects, built once per process
    (the app loads them once per process too).  The cache is keyed on the
    identity of the four dictionaries and keeps references to all four, so an
    entry's key cannot be taken by another object while it is cached.  The
    dictionaries must not be mutated afterwards: the device table is a
    snapshot (build a ``TagTable`` yourself and pass ``table=`` otherwise).
    At most ``MAX_CACHED_TABLES`` tables are kept; the least recently used one
    is closed, which frees its device memory."""
    key = (id(movie_genres), id(movie_tags), id(tag_counts), id(movie_medians), int(device))
    entry = _TABLES.pop(key, None)
    if entry is None:
        entry = (TagTable(movie_genres, movie_tags, tag_counts, movie_medians, device),
                 (movie_genres, movie_tags, tag_counts, movie_medians))
        while len(_TABLES) >= MAX_CACHED_TABLES:
            _TABLES.pop(next(iter(_TABLES)))[0].close()
    _TABLES[key] = entry          # most recently used last
    return entry[0]


class TagLS_UserProfile:
    """Tag least-squares model of a single user (``models.py:342-640``).

    Same constructor arguments and methods as the reference, plus ``table``;
    the profile, the LSQR fit and the predictions run on the GPU."""

    def __init__(self, movie_genres, movie_ratings, movie_tags, tag_counts, movie_medians,
                 genre_ids=None, tag_ids=None, table=None):
        self._table = table or tag_table_for(movie_genres, movie_tags, tag_counts, movie_medians)
        self._genre_ids = genre_ids
        self._tag_ids = tag_ids
        self._fit = self._table.fit([list(movie_ratings)])
        self.profile = self._fit.profile_list(0)
        self.x_factors = self._fit.x_factors(0)
        self.itn = int(self._fit.itn[0])
        self.istop = int(self._fit.istop[0])
        self._scores = None

    def is_valid(self):
        return True

    def predict(self, movie_id):
        """Predicted rating, or None without a median (``models.py:544-590``)."""
        c = self._table.cand_index.get(movie_id)
        if c is None:
            return None
        if self._scores is None:
            self._scores = self._table.scores(self._fit)[0]
        return float(self._scores[c])

    def get_param_list(self):
        """``models.py:593-639``: genres then tags, each sorted by
        coefficient descending under a ``__comment`` heading."""
        if self._genre_ids is None or self._tag_ids is None:
            return []
        genre_names = {i: n for n, i in self._genre_ids.items()}
        tag_names = {i: n for n, i in self._tag_ids.items()}
        genres, tags = [], []
        for i, pid in enumerate(self.profile):
            f = self.x_factors[i][0]
            if pid < TAG_OFFSET:
                genres.append((genre_names[pid], f))
            else:
                tags.append((tag_names[pid - TAG_OFFSET], f))
        out = []
        if genres:
            genres.sort(key=lambda e: e[1], reverse=True)
            out.append(("__comment", "Genre Parameters"))
            out += genres
        if tags:
            tags.sort(key=lambda e: e[1], reverse=True)
            out.append(("__comment", "Tag Parameters"))
            out += tags
        return out


def tag_ls_eval(user_ratings_train, user_ratings_test, movie_genres, movie_tags, tag_counts,
                movie_medians_train, device=0, table=None, return_stats=False):
    """``_tag_ls_eval``: both arguments are ``[(user_id, [(movie_id,
    rating)])]``, aligned; returns ``[(user_id, agreement)]`` for the users
    with an agreement, in input order -- one batched fit and one evaluation."""
    own = table is None
    if own:
        table = TagTable(movie_genres, movie_tags, tag_counts, movie_medians_train, device)
    try:
        res = table.evaluate([l for _, l in user_ratings_train],
                             [l for _, l in user_ratings_test])
    finally:
        if own:
            table.close()
    out = [(uid, float(a)) for (uid, _), a in zip(user_ratings_test, res["agreement"])
           if not np.isnan(a)]
    return (out, res) if return_stats else out
