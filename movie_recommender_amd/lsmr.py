"""Sparse LSMR on the GPU (``mr_lsqr_solve_lsmr`` in ``include/mr_lsqr.h``)
and the reference's SciPy ALS with LSMR in place of LSQR.

``lsmr`` takes ``scipy.sparse.linalg.lsmr``'s arguments and returns its
8-tuple; the solver restates SciPy's (1.15) operation for operation on the
device, on the resident matrix of ``lsqr.LsqrContext`` (whose ``solve_lsmr``
serves any number of solves and value updates).  The reference times both
solvers side by side (``python/basics/lsmr.py``); ``als_lsmr`` is
``lsqr.als_lsqr`` with one global LSMR per half-step.

There is no CPU fallback: without the native library or a device every
entry point raises.
"""
from . import lsqr as _lsqr

__all__ = ["lsmr", "als_lsmr"]


def lsmr(A, b, damp=0.0, atol=1e-6, btol=1e-6, conlim=1e8, maxiter=None, show=False, x0=None,
         device=0):
    """``scipy.sparse.linalg.lsmr`` on the GPU: returns (x, istop, itn, normr,
    normar, norma, conda, normx).  ``show`` is not offered (ValueError);
    ``maxiter=None`` means min(rows, columns)."""
    if show:
        raise ValueError("show is not offered by the GPU solver")
    with _lsqr.LsqrContext(A, device=device) as ctx:
        if maxiter is None:
            maxiter = min(ctx.rows, ctx.cols)
        x, r = ctx.solve_lsmr(b, damp=damp, atol=atol, btol=btol, conlim=conlim, maxiter=maxiter,
                              x0=x0)
    return (x, r["istop"], r["itn"], r["normr"], r["normar"], r["norma"], r["conda"],
            r["normx"])


def als_lsmr(user_ids, item_ids, ratings, k, num_users, num_items, movies0=None, seed=None,
             max_iterations=30, iter_lim=100, device=0, callback=None):
    """``lsqr.als_lsqr`` with LSMR: users, then movies, by one global LSMR each
    (SciPy's default tolerances, ``maxiter=iter_lim``) until the mean absolute
    training error improves by less than 1 % or ``max_iterations`` have run.
    Arguments, return value and ``callback`` are ``als_lsqr``'s; a half-step's
    result is ``solve_lsmr``'s dict."""
    return _lsqr._als(lambda ctx, rhs: ctx.solve_lsmr(rhs, maxiter=iter_lim), user_ids, item_ids,
                      ratings, k, num_users, num_items, movies0, seed, max_iterations, device,
                      callback)
