"""General sparse LSQR on the GPU (``include/mr_lsqr.h``) and the reference's
SciPy ALS on top of it.

``lsqr`` takes ``scipy.sparse.linalg.lsqr``'s arguments and returns its
10-tuple; the solver restates SciPy's (1.15) operation for operation on the
device.  ``LsqrContext`` keeps a matrix's structure on the device for any
number of solves and value updates; ``LsqrContext.solve_lsmr`` is SciPy's
LSMR on the same resident matrix (the ``lsmr`` module wraps it).  ``als_lsqr`` is the reference's
``fit_to_data`` (``python/100k_data/ratings_als.py:502-529``): one global
LSQR on the design matrix per half-step, the two design matrices' structure
built once and their values gathered on the device from the factor tables.

There is no CPU fallback: without the native library or a device every
entry point raises.
"""
import ctypes

import numpy as np

from . import _lib

__all__ = ["LsqrContext", "lsqr", "als_lsqr"]


def _csr_arrays(A):
    """(row_indices, col_indices, values, rows, cols) from a SciPy sparse
    matrix / dense 2-D array, or from the tuple (row_indices, col_indices,
    values, num_cols)."""
    if isinstance(A, tuple):
        if len(A) != 4:
            raise ValueError("expected (row_indices, col_indices, values, num_cols)")
        rp, ci, vals, cols = A
        rp = np.ascontiguousarray(rp, np.int64)
        if rp.ndim != 1 or len(rp) < 1:
            raise ValueError("row_indices must hold rows + 1 entries")
        rows = len(rp) - 1
    else:
        import scipy.sparse as sp
        if not sp.issparse(A):
            A = np.asarray(A)
            if A.ndim != 2:
                raise ValueError("A must be a sparse matrix, a 2-D array or a CSR tuple")
        M = sp.csr_matrix(A)
        rp, ci, vals = M.indptr, M.indices, M.data
        rows, cols = M.shape
        rp = np.ascontiguousarray(rp, np.int64)
    ci = np.ascontiguousarray(ci, np.int64).ravel()
    vals = np.ascontiguousarray(vals, np.float64).ravel()
    cols = int(cols)
    if cols < 0:
        raise ValueError("num_cols must be >= 0")
    if rp[0] != 0 or np.any(np.diff(rp) < 0):
        raise ValueError("row_indices must start at 0 and be non-decreasing")
    if rp[-1] >= 2 ** 31 or rows >= 2 ** 31 or cols >= 2 ** 31:
        raise ValueError("the matrix exceeds the int32 CSR form of mr_lsqr_create")
    if len(ci) != rp[-1] or len(vals) != rp[-1]:
        raise ValueError("col_indices / values must hold row_indices[-1] entries")
    if len(ci) and (ci.min() < 0 or ci.max() >= cols):
        raise ValueError("column index out of range")
    return rp.astype(np.int32), ci.astype(np.int32), vals, int(rows), cols


def _vec(v, n, name):
    v = np.ascontiguousarray(np.asarray(v, np.float64))
    if v.ndim > 1:
        v = np.ascontiguousarray(v.squeeze())
    v = np.atleast_1d(v)
    if v.shape != (n,):
        raise ValueError(f"{name} must hold {n} entries, got shape {v.shape}")
    return v


class LsqrContext:
    """A sparse matrix resident on the device: structure uploaded and sorted
    once, values replaceable, any number of LSQR solves."""

    def __init__(self, A, device=0):
        rp, ci, vals, self.rows, self.cols = _csr_arrays(A)
        self.nnz = int(rp[-1])
        self._L = _lib.lib()
        self._h = self._L.mr_lsqr_create(int(device), self.rows, self.cols,
                                         rp.ctypes.data_as(_lib.IP), ci.ctypes.data_as(_lib.IP),
                                         vals.ctypes.data_as(_lib.DP))
        if not self._h:
            raise RuntimeError(f"mr_lsqr_create failed: {_lib.last_error()}")

    def close(self):
        if getattr(self, "_h", None):
            self._L.mr_lsqr_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        self.close()

    def _handle(self):
        if not self._h:
            raise RuntimeError("the LSQR context is closed")
        return self._h

    def solve(self, b, damp=0.0, atol=1e-6, btol=1e-6, conlim=1e8, iter_lim=None, x0=None):
        """(x, result) with result = dict(istop, itn, r1norm, r2norm, anorm,
        acond, arnorm, xnorm), as ``scipy.sparse.linalg.lsqr`` defines them."""
        b = _vec(b, self.rows, "b")
        x0p = None
        if x0 is not None:
            x0 = _vec(x0, self.cols, "x0")
            x0p = x0.ctypes.data_as(_lib.DP)
        if iter_lim is None:
            iter_lim = 2 * self.cols
        iter_lim = int(iter_lim)
        if iter_lim >= 2 ** 31:
            raise ValueError("iter_lim exceeds int32")
        x = np.zeros(self.cols, np.float64)
        res = _lib.MrLsqrResult()
        _lib.check(self._L.mr_lsqr_solve(self._handle(), b.ctypes.data_as(_lib.DP), x0p,
                                         float(damp), float(atol), float(btol), float(conlim),
                                         iter_lim, x.ctypes.data_as(_lib.DP), ctypes.byref(res)),
                   "mr_lsqr_solve")
        return x, {"istop": res.istop, "itn": res.itn, "r1norm": res.r1norm,
                   "r2norm": res.r2norm, "anorm": res.anorm, "acond": res.acond,
                   "arnorm": res.arnorm, "xnorm": res.xnorm}

    def solve_lsmr(self, b, damp=0.0, atol=1e-6, btol=1e-6, conlim=1e8, maxiter=None, x0=None):
        """LSMR on the resident matrix: (x, result) with result = dict(istop,
        itn, normr, normar, norma, conda, normx), as
        ``scipy.sparse.linalg.lsmr`` defines them; ``maxiter=None`` means
        min(rows, columns), SciPy's rule for LSMR."""
        b = _vec(b, self.rows, "b")
        x0p = None
        if x0 is not None:
            x0 = _vec(x0, self.cols, "x0")
            x0p = x0.ctypes.data_as(_lib.DP)
        if maxiter is None:
            maxiter = min(self.rows, self.cols)
        maxiter = int(maxiter)
        if maxiter >= 2 ** 31:
            raise ValueError("maxiter exceeds int32")
        x = np.zeros(self.cols, np.float64)
        res = _lib.MrLsmrResult()
        _lib.check(self._L.mr_lsqr_solve_lsmr(self._handle(), b.ctypes.data_as(_lib.DP), x0p,
                                              float(damp), float(atol), float(btol),
                                              float(conlim), maxiter, x.ctypes.data_as(_lib.DP),
                                              ctypes.byref(res)),
                   "mr_lsqr_solve_lsmr")
        return x, {"istop": res.istop, "itn": res.itn, "normr": res.normr,
                   "normar": res.normar, "norma": res.norma, "conda": res.conda,
                   "normx": res.normx}

    def svds(self, k=6, ncv=None, tol=0, which="LM", v0=None, maxiter=None,
             return_singular_vectors=True, seed=0):
        """The k largest singular triplets of the resident matrix, with
        ``scipy.sparse.linalg.svds``'s arguments and return value (``svds``
        module); the result struct is left in ``last_svds``."""
        from . import svds as S
        k, ncv, tol, maxiter, v0, want = S._check_args(self.rows, self.cols, k, ncv, tol, which,
                                                       v0, maxiter, return_singular_vectors)
        s = np.zeros(k, np.float64)
        U = np.zeros((self.rows, k), np.float64) if want else None
        Vt = np.zeros((k, self.cols), np.float64) if want else None
        res = _lib.MrSvdsResult()
        _lib.check(self._L.mr_lsqr_svds(
            self._handle(), k, ncv, tol, maxiter,
            None if v0 is None else v0.ctypes.data_as(_lib.DP), int(seed) & (2 ** 64 - 1),
            1 if want else 0, s.ctypes.data_as(_lib.DP),
            U.ctypes.data_as(_lib.DP) if want else None,
            Vt.ctypes.data_as(_lib.DP) if want else None, ctypes.byref(res)), "mr_lsqr_svds")
        resid = np.zeros(k, np.float64)
        _lib.check(self._L.mr_lsqr_svds_residuals(self._handle(), k,
                                                  resid.ctypes.data_as(_lib.DP)),
                   "mr_lsqr_svds_residuals")
        self.last_svds = dict(res.as_dict(), residuals=resid)
        return S._finish(U, s, Vt, self.last_svds, want)

    def svds_stats(self):
        st = _lib.MrSvdsStats()
        _lib.check(self._L.mr_svds_get_stats(self._handle(), ctypes.byref(st)),
                   "mr_svds_get_stats")
        return st.as_dict()

    def set_values(self, values):
        """New values for the same structure, in the order given at creation."""
        v = _vec(values, self.nnz, "values")
        _lib.check(self._L.mr_lsqr_set_values(self._handle(), v.ctypes.data_as(_lib.DP)),
                   "mr_lsqr_set_values")

    def set_value_map(self, index):
        """index[nnz]: -1 = the constant 1.0, otherwise an index into the
        table of ``set_values_from_table``."""
        idx = np.ascontiguousarray(index, np.int64).ravel()
        if idx.shape != (self.nnz,):
            raise ValueError(f"index must hold {self.nnz} entries")
        if len(idx) and (idx.min() < -1 or idx.max() >= 2 ** 31):
            raise ValueError("value map entries are -1 or a table index")
        idx = idx.astype(np.int32)
        _lib.check(self._L.mr_lsqr_set_value_map(self._handle(), idx.ctypes.data_as(_lib.IP)),
                   "mr_lsqr_set_value_map")

    def set_values_from_table(self, table):
        t = np.ascontiguousarray(np.asarray(table, np.float64).ravel())
        _lib.check(self._L.mr_lsqr_set_values_from_table(self._handle(),
                                                         t.ctypes.data_as(_lib.DP), len(t)),
                   "mr_lsqr_set_values_from_table")

    def residual_l1(self, b, x):
        """sum_i |b_i - (A x)_i| on the device."""
        b = _vec(b, self.rows, "b")
        x = _vec(x, self.cols, "x")
        out = ctypes.c_double(0.0)
        _lib.check(self._L.mr_lsqr_residual_l1(self._handle(), b.ctypes.data_as(_lib.DP),
                                               x.ctypes.data_as(_lib.DP), ctypes.byref(out)),
                   "mr_lsqr_residual_l1")
        return out.value

    def stats(self):
        st = _lib.MrLsqrStats()
        _lib.check(self._L.mr_lsqr_get_stats(self._handle(), ctypes.byref(st)),
                   "mr_lsqr_get_stats")
        return st.as_dict()

    def reset_stats(self):
        _lib.check(self._L.mr_lsqr_reset_stats(self._handle()), "mr_lsqr_reset_stats")

    def set_timing(self, enable):
        _lib.check(self._L.mr_lsqr_set_timing(self._handle(), 1 if enable else 0),
                   "mr_lsqr_set_timing")

    def set_gather_path(self, mode):
        _lib.check(self._L.mr_lsqr_set_gather_path(self._handle(), int(mode)),
                   "mr_lsqr_set_gather_path")


def lsqr(A, b, damp=0.0, atol=1e-6, btol=1e-6, conlim=1e8, iter_lim=None, show=False,
         calc_var=False, x0=None, device=0):
    """``scipy.sparse.linalg.lsqr`` on the GPU: returns (x, istop, itn, r1norm,
    r2norm, anorm, acond, arnorm, xnorm, var) with var all zero.  ``show`` and
    ``calc_var`` are not offered (ValueError); ``iter_lim=None`` means
    2 * columns."""
    if show:
        raise ValueError("show is not offered by the GPU solver")
    if calc_var:
        raise ValueError("calc_var is not offered by the GPU solver")
    with LsqrContext(A, device=device) as ctx:
        if iter_lim is None:
            iter_lim = 2 * ctx.cols
        x, r = ctx.solve(b, damp=damp, atol=atol, btol=btol, conlim=conlim, iter_lim=iter_lim,
                         x0=x0)
        cols = ctx.cols
    return (x, r["istop"], r["itn"], r["r1norm"], r["r2norm"], r["anorm"], r["acond"],
            r["arnorm"], r["xnorm"], np.zeros(cols))


def als_lsqr(user_ids, item_ids, ratings, k, num_users, num_items, movies0=None, seed=None,
             max_iterations=30, iter_lim=100, device=0, callback=None):
    """The reference's SciPy ALS (``ratings_als.py:502-529``): users, then
    movies, by one global LSQR each (SciPy's default tolerances, ``iter_lim``
    iterations at most) until the mean absolute training error improves by
    less than 1 % or ``max_iterations`` have run.

    Returns (users[num_users * (k + 1)], movies[num_items * k], iterations,
    errors) in the reference's flat layouts; a user's bias is column k.
    ``movies0`` (or uniform(-1, 1) from ``seed``) starts the loop.
    ``callback(info)`` is called after every iteration with the iteration
    number, copies of both tables, the error and each half-step's LSQR result.
    """
    return _als(lambda ctx, rhs: ctx.solve(rhs, iter_lim=iter_lim), user_ids, item_ids, ratings,
                k, num_users, num_items, movies0, seed, max_iterations, device, callback)


def _als(solve, user_ids, item_ids, ratings, k, num_users, num_items, movies0, seed,
         max_iterations, device, callback):
    """The loop of ``als_lsqr`` / ``lsmr.als_lsmr``: ``solve(ctx, rhs)`` is one
    half-step's global solve on an ``LsqrContext``, returning (x, result)."""
    uid = np.ascontiguousarray(user_ids, np.int64).ravel()
    iid = np.ascontiguousarray(item_ids, np.int64).ravel()
    r = np.ascontiguousarray(ratings, np.float64).ravel()
    k, num_users, num_items = int(k), int(num_users), int(num_items)
    n = len(r)
    if k < 1 or num_users < 1 or num_items < 1:
        raise ValueError("k, num_users and num_items must be positive")
    if len(uid) != n or len(iid) != n or n == 0:
        raise ValueError("user_ids, item_ids and ratings must hold the same, non-zero count")
    if uid.min() < 0 or uid.max() >= num_users or iid.min() < 0 or iid.max() >= num_items:
        raise ValueError("id out of range")
    if max(num_users * (k + 1), num_items * k, n * (k + 1)) >= 2 ** 31:
        raise ValueError("the design matrices exceed the int32 CSR form")
    if movies0 is None:
        movies = np.random.default_rng(seed).uniform(-1, 1, num_items * k)
    else:
        movies = _vec(movies0, num_items * k, "movies0").copy()
    j1, j0 = np.arange(k + 1), np.arange(k)
    # users' rows [V_i, 1] on columns u (k + 1) ..; movies' rows U_u[:k] on i k ..
    cols_u = (uid[:, None] * (k + 1) + j1[None, :]).ravel()
    map_u = np.concatenate([iid[:, None] * k + j0[None, :], np.full((n, 1), -1)], axis=1).ravel()
    cols_i = (iid[:, None] * k + j0[None, :]).ravel()
    map_i = (uid[:, None] * (k + 1) + j0[None, :]).ravel()
    rp_u = np.arange(n + 1, dtype=np.int64) * (k + 1)
    rp_i = np.arange(n + 1, dtype=np.int64) * k
    errors = []
    users = None
    iterations = 0
    with LsqrContext((rp_u, cols_u, np.ones(len(cols_u)), num_users * (k + 1)), device) as cu, \
            LsqrContext((rp_i, cols_i, np.ones(len(cols_i)), num_items * k), device) as cm:
        cu.set_value_map(map_u)
        cm.set_value_map(map_i)
        old_error = None
        for it in range(int(max_iterations)):
            cu.set_values_from_table(movies)
            users, ru = solve(cu, r)
            cm.set_values_from_table(users)
            rhs = r - users[k::k + 1][uid]
            movies, rm = solve(cm, rhs)
            error = cm.residual_l1(rhs, movies) / n
            errors.append(error)
            iterations = it + 1
            if callback is not None:
                callback({"iteration": it, "users": users.copy(), "movies": movies.copy(),
                          "error": error, "user_solve": ru, "item_solve": rm})
            if old_error is not None and error > 0.99 * old_error:
                break
            old_error = error
    return users, movies, iterations, errors
