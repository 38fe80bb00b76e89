"""Implicit-feedback ALS (Hu, Koren, Volinsky 2008) on the device-resident
engine: plays, clicks or view counts instead of ratings.

A stored ``(user, item, r)`` with ``r >= 0`` means "preference 1 with
confidence ``1 + alpha r``"; every other pair means "preference 0 with
confidence 1".  The loss runs over ALL pairs,

    J = sum_ui c_ui (p_ui - x_u . y_i)^2 + reg (pen_users + pen_items),

and is never formed densely (``AlsContext.set_implicit``, DESIGN.md "Implicit
feedback").  There is no user bias in this model.

Behind a trained model (DESIGN.md "Ranking evaluation and implicit fold-in"):
``fold_in`` solves the user half-step for users that were not in the training
set, and ``ImplicitModel`` bundles fold-in (of users and of items, non-negative
for a non-negative model), ranking evaluation and top-N.
"""
import numpy as np

from . import _lib
from .engine import AlsContext, check_implicit, check_regularization

FOLD_IN_MAX_K = 128


def als_implicit(user_ids, item_ids, confidence, k, num_users, num_items, alpha=40.0,
                 reg=0.01, reg_mode="constant", solver="cholesky", max_iterations=15,
                 tol=1e-4, seed=0):
    """Trains one implicit-feedback model.  ``confidence`` holds the counts /
    strengths ``r >= 0`` of the stored pairs.  U0 then V0 are drawn from
    ``numpy.random.RandomState(seed)`` (uniform(-1, 1), ``cpp_ls.als``'s
    shapes; the bias column is dropped); ALS iterations run until the relative
    decrease of J falls below ``tol`` or ``max_iterations`` is reached.
    Returns ``(X[num_users, k], Y[num_items, k], iterations, [J after every
    iteration])``; the score of a pair is ``X[u] @ Y[i]``.

    ``solver="nnls"`` constrains every factor to be >= 0 (each half-step is
    the exact non-negative block minimiser, ``AlsContext.set_nnls``): X and Y
    come back non-negative, so every score is a non-negative affinity."""
    alpha = check_implicit(alpha)
    if not alpha > 0.0:
        raise ValueError("alpha must be > 0")
    check_regularization(reg, reg_mode)
    k, num_users, num_items = int(k), int(num_users), int(num_items)
    rs = np.random.RandomState(seed)
    U0 = rs.uniform(-1, 1, num_users * (k + 1))
    V0 = rs.uniform(-1, 1, num_items * k)
    history = []
    with AlsContext(user_ids, item_ids, confidence, k, num_users, num_items, solver=solver,
                    reg=reg, reg_mode=reg_mode, implicit_alpha=alpha) as ctx:
        ctx.set_factors(U0, V0)
        iterations = 0
        while iterations < max_iterations:
            ctx.iterate(1)
            iterations += 1
            history.append(ctx.objective()["J"])
            if len(history) > 1 and history[-2] - history[-1] < tol * abs(history[-2]):
                break
        U, V = ctx.get_factors()
    X = U.reshape(num_users, k + 1)[:, :k].copy()
    Y = V.reshape(num_items, k).copy()
    return X, Y, iterations, history


def _lists_csr(item_lists):
    """(offsets int64[B + 1], items int64[nnz], r f64[nnz]) of ``item_lists``:
    a sequence of ``[(item, r)]`` lists, or a CSR triple ``(offsets, items,
    r)`` whose first member is an ndarray."""
    if isinstance(item_lists, tuple) and len(item_lists) == 3 and \
            isinstance(item_lists[0], np.ndarray):
        off = np.ascontiguousarray(item_lists[0], np.int64)
        items, r = np.asarray(item_lists[1]), np.asarray(item_lists[2], np.float64)
        if off.ndim != 1 or off.size < 1 or off[0] != 0 or np.any(np.diff(off) < 0) or \
                items.ndim != 1 or off[-1] != len(items) or r.shape != items.shape:
            raise ValueError("offsets must be int64[B + 1], non-decreasing, from 0 to len(items); "
                             "items and r 1-D of that length")
    else:
        lists = [list(l) for l in item_lists]
        off = np.zeros(len(lists) + 1, np.int64)
        off[1:] = np.cumsum([len(l) for l in lists])
        items = np.array([it for l in lists for it, _ in l])
        r = np.array([rv for l in lists for _, rv in l], np.float64)
    if items.size and not np.issubdtype(items.dtype, np.integer):
        raise ValueError("item ids must be integers")
    return off, items.astype(np.int64), r


def fold_in(Y, item_lists, alpha=40.0, reg=0.01, reg_mode="constant", device=0):
    """Factors of users that were not in the training set, from the item
    factors ``Y[I, k]`` (``k <= 128``) of an implicit model: per user, with
    ``w = alpha r``, the Cholesky solve (fp64) of

        (Y^T Y + sum w y y^T + lambda_u I) x = sum (1 + w) y,

    ``lambda_u = reg`` (``"constant"``) or ``reg`` times the length of the
    user's list (``"weighted"``) -- ``als_implicit``'s user half-step.
    ``item_lists`` is a sequence of ``[(item, r)]`` lists (``r >= 0``), or a
    CSR triple ``(offsets int64[B + 1], items, r)``.  Returns ``(X[B, k],
    status int32[B])``: status 1 solved, 0 a pivot was not positive (only
    with ``reg = 0``; the row is zero).  An empty list gives the zero row.

    ``ValueError`` before any native call for a bad ``alpha`` / ``reg`` /
    ``reg_mode``, ``k`` outside 1..128, factors that are not finite, an item
    id out of range or an ``r`` that is negative or not finite."""
    alpha = check_implicit(alpha)
    reg, mode = check_regularization(reg, reg_mode)
    Y = np.ascontiguousarray(Y, np.float64)
    if Y.ndim != 2 or not 1 <= Y.shape[1] <= FOLD_IN_MAX_K:
        raise ValueError(f"Y must be [items, k] with k in 1..{FOLD_IN_MAX_K}")
    if not np.all(np.isfinite(Y)):
        raise ValueError("factors must be finite")
    n_items, k = Y.shape
    off, items, r = _lists_csr(item_lists)
    if items.size and (items.min() < 0 or items.max() >= n_items):
        raise ValueError("item id out of range")
    if not np.all(np.isfinite(r)) or np.any(r < 0):
        raise ValueError("r must be finite and >= 0")
    B = len(off) - 1
    X = np.zeros((max(B, 1), k))
    status = np.zeros(max(B, 1), np.int32)
    item32 = np.ascontiguousarray(items if items.size else np.zeros(1), np.int32)
    r = np.ascontiguousarray(r if r.size else np.zeros(1), np.float64)
    ip, dp = _lib.IP, _lib.DP
    _lib.check(_lib.lib().mr_implicit_fold_in(
        int(device), k, n_items, Y.ctypes.data_as(dp), alpha, reg, mode, B,
        off.ctypes.data_as(_lib.LLP), item32.ctypes.data_as(ip), r.ctypes.data_as(dp),
        X.ctypes.data_as(dp), status.ctypes.data_as(ip)), "mr_implicit_fold_in")
    return X[:B], status[:B]


class ImplicitModel:
    """A trained implicit-feedback model ``(X[U, k], Y[I, k])`` with the
    hyper-parameters it was trained with: fold-in of new users, ranking
    evaluation and top-N on one GPU.  The score of a pair is ``X[u] @ Y[i]``
    in the exact order of ``ranking.rank_counts``.  ``nonneg=True`` for a
    model trained with ``solver="nnls"``: folded-in rows are then the exact
    non-negative minimisers, like the trained ones."""

    def __init__(self, X, Y, alpha=40.0, reg=0.01, reg_mode="constant", device=0, nonneg=False):
        self.alpha = check_implicit(alpha)
        self.reg, _ = check_regularization(reg, reg_mode)
        self.reg_mode = reg_mode
        self.X = np.ascontiguousarray(X, np.float64)
        self.Y = np.ascontiguousarray(Y, np.float64)
        if self.X.ndim != 2 or self.Y.ndim != 2 or self.X.shape[1] != self.Y.shape[1]:
            raise ValueError("X and Y must be 2-D arrays with the same number of factors")
        self.k = self.Y.shape[1]
        self.device = int(device)
        self.nonneg = bool(nonneg)
        self._table = None

    def fold_in(self, lists):
        """``fold_in`` with the model's Y, alpha and regularisation: ``(X[B,
        k], status)``.  A non-negative model goes through ``foldin.fold_in``
        (status -1: the solve stopped at its round cap)."""
        if self.nonneg:
            from .foldin import fold_in as general
            return general(self.Y, lists, "implicit", alpha=self.alpha, reg=self.reg,
                           reg_mode=self.reg_mode, nonneg=True, device=self.device)[:2]
        return fold_in(self.Y, lists, self.alpha, self.reg, self.reg_mode, self.device)

    def fold_in_items(self, lists):
        """Factors of new items from ``[(user, r)]`` lists (or a CSR triple):
        the model's item half-step on its user table X.  Returns ``(Y_new[B,
        k], status)``."""
        from .foldin import fold_in as general
        return general(self.X, lists, "implicit", alpha=self.alpha, reg=self.reg,
                       reg_mode=self.reg_mode, nonneg=self.nonneg, device=self.device)[:2]

    def _explain(self, table, lists, targets, top, full):
        if self.nonneg:
            raise ValueError("explanations cover the unconstrained solve only: a model with "
                             "nonneg=True is not supported")
        from .foldin import explain
        return explain(table, lists, targets, "implicit", alpha=self.alpha, reg=self.reg,
                       reg_mode=self.reg_mode, top=top, full=full, device=self.device)

    def explain(self, lists, targets, top=10, full=False):
        """Why items score what they score for folded-in users: per user of
        ``lists`` (as ``fold_in`` takes them) and per item of ``targets[u]``
        the ``top`` entries of the user's own list by their contribution to
        ``x_u . Y[t]`` (``foldin.explain``; the contributions of a target sum
        to its score).  Returns a ``foldin.Explanation``.  A model with
        ``nonneg=True`` raises ``ValueError``."""
        return self._explain(self.Y, lists, targets, top, full)

    def explain_items(self, lists, targets, top=10, full=False):
        """``explain`` for folded-in items: ``lists`` hold ``(user, r)``,
        ``targets`` users of X."""
        return self._explain(self.X, lists, targets, top, full)

    def rank_eval(self, test, exclude=None, n=10, weights=None):
        """``ranking.rank_eval`` of the model's own users on held-out pairs."""
        from .ranking import rank_eval
        return rank_eval(self.X, self.Y, test, exclude, n, weights, device=self.device)

    def top_n(self, x_rows, rated=None, num_results=10):
        """Per row of ``x_rows[B, k]`` (trained or folded-in user factors)
        the first ``num_results`` items by (score, item id) descending that
        are not in ``rated[u]``: a list of ``[(score, item)]`` per user.  Runs
        on a ``MovieTable`` with the identity id map, zero medians and a zero
        bias column; adding 0.0 twice leaves every comparison as it is."""
        from .serving import MovieTable
        if self._table is None:
            n_items = self.Y.shape[0]
            ids = {i: i for i in range(n_items)}
            self._table = MovieTable(self.k, self.Y.reshape(-1), ids, dict.fromkeys(ids, 0.0),
                                     self.device)
        x = np.atleast_2d(np.asarray(x_rows, np.float64))
        if x.shape[1] != self.k:
            raise ValueError("user factor rows must have k entries")
        xb = np.concatenate([x, np.zeros((x.shape[0], 1))], axis=1)
        return self._table.top_n(xb, rated, num_results)

    def close(self):
        if self._table is not None:
            self._table.close()
            self._table = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
