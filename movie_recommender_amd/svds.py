"""Truncated sparse SVD on the GPU (``mr_lsqr_svds``, ``include/mr_lsqr.h``).

``svds`` takes ``scipy.sparse.linalg.svds``'s arguments and returns its
``(U, s, Vt)`` with ``s`` ascending; ``LsqrContext.svds`` is the same on a
matrix that is already resident.  The solver is a thick-restart
Golub-Kahan-Lanczos bidiagonalisation with full re-orthogonalisation in fp64:
the products run on the context's SpMV, the basis kernels are
``csrc/svds.hip``.

Differences from SciPy: only ``which='LM'`` and whole singular vectors (or
none) are offered; ``v0`` always has ``A.shape[1]`` entries (ARPACK's start
vector belongs to the smaller dimension); without ``v0`` the start vector
comes from ``seed``, and the same inputs give the same bits; ``tol=0`` means
a residual of ``8 ncv eps sigma_1``.  A single Lanczos vector finds one vector
of a multiple singular value, as ARPACK does.

There is no CPU fallback: without the native library or a device every entry
point raises.
"""
import numpy as np

from . import lsqr as _lsqr

__all__ = ["svds", "SvdsNoConvergence"]


class SvdsNoConvergence(RuntimeError):
    """Fewer than k triplets converged within ``maxiter`` restarts.  The
    converged ones are ``singular_values`` (ascending), ``U`` and ``Vt`` (None
    without vectors), as ``ArpackNoConvergence`` carries its eigenpairs."""

    def __init__(self, msg, singular_values, U, Vt, result):
        super().__init__(msg)
        self.singular_values = singular_values
        self.U = U
        self.Vt = Vt
        self.result = result


def default_ncv(k, mn):
    return min(mn, max(2 * k + 1, 20))


def _check_args(rows, cols, k, ncv, tol, which, v0, maxiter, return_singular_vectors):
    """The refusals that need no device, and the defaults; returns (k, ncv,
    tol, maxiter, v0, want_vectors)."""
    if which != "LM":
        raise ValueError("which: only 'LM' is offered")
    if return_singular_vectors not in (True, False):
        raise ValueError("return_singular_vectors: only True or False is offered")
    mn = min(rows, cols)
    k = int(k)
    if not 1 <= k <= mn:
        raise ValueError(f"k must be in 1..min(A.shape) = {mn}, got {k}")
    ncv = default_ncv(k, mn) if ncv is None else int(ncv)
    if not (k < ncv <= mn or ncv == k == mn):
        raise ValueError(f"ncv must satisfy k < ncv <= min(A.shape) = {mn}, got {ncv}")
    tol = float(tol)
    if not (tol >= 0 and np.isfinite(tol)):
        raise ValueError("tol must be finite and >= 0")
    maxiter = 10 * mn if maxiter is None else int(maxiter)
    if not 1 <= maxiter < 2 ** 31:
        raise ValueError("maxiter must be in 1..2^31 - 1")
    if v0 is not None:
        v0 = _lsqr._vec(v0, cols, "v0")
        if not np.all(np.isfinite(v0)):
            raise ValueError("v0 must be finite")
        if not np.any(v0):
            raise ValueError("v0 must not be zero")
    return k, ncv, tol, maxiter, v0, bool(return_singular_vectors)


def _finish(U, s, Vt, result, want):
    """SciPy's order (ascending), or SvdsNoConvergence with the converged triplets."""
    if not result["converged"]:
        n = result["nconv"]
        raise SvdsNoConvergence(
            f"svds: {n} of {len(s)} singular triplets converged in {result['restarts']} restarts",
            s[:n][::-1].copy(), U[:, :n][:, ::-1].copy() if want else None,
            Vt[:n][::-1].copy() if want else None, result)
    if not want:
        return s[::-1].copy()
    return U[:, ::-1].copy(), s[::-1].copy(), Vt[::-1].copy()


def svds(A, k=6, ncv=None, tol=0, which="LM", v0=None, maxiter=None,
         return_singular_vectors=True, seed=0, device=0):
    """``scipy.sparse.linalg.svds`` on the GPU: ``(U, s, Vt)`` with ``s``
    ascending, or ``s`` alone.  ``A`` is a SciPy sparse matrix, a dense 2-D
    array or the tuple (row_indices, col_indices, values, num_cols)."""
    if which != "LM":
        raise ValueError("which: only 'LM' is offered")
    if return_singular_vectors not in (True, False):
        raise ValueError("return_singular_vectors: only True or False is offered")
    with _lsqr.LsqrContext(A, device=device) as ctx:
        return ctx.svds(k=k, ncv=ncv, tol=tol, which=which, v0=v0, maxiter=maxiter,
                        return_singular_vectors=return_singular_vectors, seed=seed)
