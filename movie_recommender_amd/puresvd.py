"""PureSVD: the truncated SVD of the zero-filled users x items rating matrix
as a factor model (Cremonesi, Koren, Turrin: "Performance of recommender
algorithms on top-N recommendation tasks", RecSys 2010).

The rating matrix is factored once on the GPU (``svds``); the item factors
``Q = V_k`` (num_items x k) feed the serving kernels: a user's factors are
``r_u Q`` and the scores ``r_u Q Q^T``.  There is no alternating loop and no
bias; ``table()`` builds a ``serving.MovieTable`` with zero medians, as
``similar.similar_by_factors`` does.
"""
import numpy as np

from . import lsqr as _lsqr

__all__ = ["PureSVD"]

SERVING_MAX_K = 128


class PureSVD:
    """``PureSVD(user_ids, item_ids, ratings, num_users, num_items, k)``:
    zero-based ids, one rating per (user, item) pair.  ``movie_ids[i]`` is the
    standard id of item i (default: i).  Further keywords go to ``svds``
    (``ncv``, ``tol``, ``maxiter``, ``v0``, ``seed``)."""

    def __init__(self, user_ids, item_ids, ratings, num_users, num_items, k, movie_ids=None,
                 device=0, **svds_kw):
        uid = np.ascontiguousarray(user_ids, np.int64).ravel()
        iid = np.ascontiguousarray(item_ids, np.int64).ravel()
        r = np.ascontiguousarray(ratings, np.float64).ravel()
        self.num_users, self.num_items, self.k = int(num_users), int(num_items), int(k)
        self.device = int(device)
        n = len(r)
        if self.num_users < 1 or self.num_items < 1:
            raise ValueError("num_users and num_items must be positive")
        if len(uid) != n or len(iid) != n or n == 0:
            raise ValueError("user_ids, item_ids and ratings must hold the same, non-zero count")
        if uid.min() < 0 or uid.max() >= self.num_users:
            raise ValueError("user id out of range")
        if iid.min() < 0 or iid.max() >= self.num_items:
            raise ValueError("item id out of range")
        if not 1 <= self.k <= min(self.num_users, self.num_items):
            raise ValueError("k must be in 1..min(num_users, num_items)")
        if n >= 2 ** 31:
            raise ValueError("the rating matrix exceeds the int32 CSR form")
        key = uid * self.num_items + iid
        self._order = np.argsort(key, kind="stable")
        sk = key[self._order]
        if np.any(sk[1:] == sk[:-1]):
            raise ValueError("duplicate (user, item) pair")
        if movie_ids is None:
            movie_ids = np.arange(self.num_items)
        self.movie_ids = [int(m) for m in movie_ids]
        if len(self.movie_ids) != self.num_items or len(set(self.movie_ids)) != self.num_items:
            raise ValueError("movie_ids must hold num_items distinct ids")
        self._als_ids = {m: i for i, m in enumerate(self.movie_ids)}
        self._svds_kw = dict(svds_kw)
        rp = np.zeros(self.num_users + 1, np.int64)
        np.cumsum(np.bincount(uid, minlength=self.num_users), out=rp[1:])
        self._ctx = _lsqr.LsqrContext((rp, iid[self._order], r[self._order], self.num_items),
                                      device=self.device)
        self._table = None
        self._factor()

    def _factor(self):
        _, s, Vt = self._ctx.svds(k=self.k, **self._svds_kw)
        # descending, as a factor model lists its factors
        self.singular_values = s[::-1].copy()
        self.item_factors = np.ascontiguousarray(Vt[::-1].T)
        self.result = self._ctx.last_svds
        if self._table is not None:
            self._table.close()
            self._table = None

    def refit(self, ratings):
        """New ratings for the same (user, item) pairs, in the order given at
        construction: the resident structure is reused."""
        r = np.ascontiguousarray(ratings, np.float64).ravel()
        if len(r) != len(self._order):
            raise ValueError(f"ratings must hold {len(self._order)} entries")
        self._ctx.set_values(r[self._order])
        self._factor()
        return self

    def close(self):
        if self._table is not None:
            self._table.close()
            self._table = None
        self._ctx.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def user_factors(self, rating_lists):
        """``r_u Q`` per list of ``[(movie_id, rating)]``: f64[B, k] (host).
        Ids without factors are refused."""
        X = np.zeros((len(rating_lists), self.k))
        for u, lst in enumerate(rating_lists):
            for mid, rating in lst:
                if mid not in self._als_ids:
                    raise ValueError(f"movie id {mid} has no factors")
            idx = np.array([self._als_ids[mid] for mid, _ in lst], np.int64)
            rr = np.array([rating for _, rating in lst], np.float64)
            X[u] = rr @ self.item_factors[idx] if len(idx) else 0.0
        return X

    def table(self):
        """A ``serving.MovieTable`` over the item factors with zero medians."""
        if self.k > SERVING_MAX_K:
            raise ValueError("rec: k must be in 1..128")
        if self._table is None:
            from .serving import MovieTable
            self._table = MovieTable(self.k, self.item_factors, self._als_ids,
                                     {m: 0.0 for m in self.movie_ids}, self.device)
        return self._table

    def recommend(self, rating_lists, num_results=10):
        """Per list the ``num_results`` unrated movies by (score, movie id)
        descending, as ``[(score, movie_id)]``; the scores are ``r_u Q Q^T``
        on the serving kernels (bias column zero)."""
        table = self.table()
        X = np.zeros((len(rating_lists), self.k + 1))
        X[:, :self.k] = self.user_factors(rating_lists)
        rated = [[mid for mid, _ in lst] for lst in rating_lists]
        return table.top_n(X, rated, int(num_results))
