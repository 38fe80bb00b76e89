"""Fold-in for every trained model (``include/mr_foldin.h``, DESIGN.md
"Fold-in"): factors of users or items that were not in the training set, from
the opposite factor table, by the half-step the model was trained with.

* explicit models (``als_train_regularized``): the ridge system of ALS-WR,
  with the user intercept (``fold_in_users``) or the users' intercepts as row
  offsets (``fold_in_items``);
* implicit models (``als_implicit``): ``mode="implicit"``;
* ``nonneg=True``: the exact non-negative minimiser (``solver="nnls"``).

Everything runs in fp64 on one GPU; there is no CPU fallback.
"""
import numpy as np

from . import _lib
from .engine import check_implicit, check_regularization
from .implicit import _lists_csr

MAX_K = 128
MODES = {"explicit": 0, "implicit": 1}   # MR_FOLD_* of include/mr_foldin.h


def fold_in(T, lists, mode="explicit", intercept=False, row_offset=None, alpha=40.0, reg=0.01,
            reg_mode="constant", nonneg=False, max_rounds=0, device=0):
    """Factors of ``B`` new entities from the opposite table ``T[n, k]``
    (``k <= 128``).  ``lists`` is a sequence of ``[(row of T, r)]`` lists or a
    CSR triple ``(offsets int64[B + 1], rows, r)``.  Per entity with ``M``
    entries, ``a_j = T[row_j]``:

    * ``mode="explicit"``: ``G = sum [a, 1][a, 1]^T``, ``c = sum (r -
      row_offset[row]) [a, 1]`` (the 1 only with ``intercept``);
    * ``mode="implicit"``: ``G = T^T T + sum w a a^T``, ``c = sum (1 + w) a``,
      ``w = alpha r`` (no intercept, no row offsets, ``r >= 0``);

    plus ``reg`` (``"constant"``) or ``reg M`` (``"weighted"``) on the first
    ``k`` diagonal entries.  ``nonneg=False``: the Cholesky solve of ``G x =
    c``.  ``nonneg=True``: the minimiser with ``x[:k] >= 0`` by block
    principal pivoting from the empty free set, at most ``max_rounds`` rounds
    (0: ``4 (k + 1)``); the intercept stays free.

    Returns ``(X[B, k + intercept], status int32[B], rounds int32[B])``:
    status 1 solved, 0 a diagonal entry or pivot was not positive (zero row),
    -1 stopped at the round cap (the last x, clamped).  An empty list gives
    the zero row with status 1 and rounds 0.

    ``ValueError`` before any native call for everything the C entry point
    refuses."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {sorted(MODES)}, not {mode!r}")
    implicit = mode == "implicit"
    intercept, nonneg = bool(intercept), bool(nonneg)
    if implicit and (intercept or row_offset is not None):
        raise ValueError("the implicit mode takes no intercept and no row_offset")
    alpha = check_implicit(alpha)
    reg, rmode = check_regularization(reg, reg_mode)
    if isinstance(max_rounds, bool) or not isinstance(max_rounds, (int, np.integer)) or \
            not 0 <= max_rounds < 2 ** 31:
        raise ValueError("max_rounds must be an integer >= 0")
    T = np.ascontiguousarray(T, np.float64)
    if T.ndim != 2 or not 1 <= T.shape[1] <= MAX_K:
        raise ValueError(f"T must be [rows, k] with k in 1..{MAX_K}")
    if not np.all(np.isfinite(T)):
        raise ValueError("factors must be finite")
    n_rows, k = T.shape
    if row_offset is not None:
        row_offset = np.ascontiguousarray(row_offset, np.float64)
        if row_offset.shape != (n_rows,) or not np.all(np.isfinite(row_offset)):
            raise ValueError("row_offset must be finite f64[rows of T]")
    off, rows, r = _lists_csr(lists)
    if rows.size and (rows.min() < 0 or rows.max() >= n_rows):
        raise ValueError("id out of range")
    if not np.all(np.isfinite(r)) or (implicit and np.any(r < 0)):
        raise ValueError("r must be finite" + (" and >= 0" if implicit else ""))
    B, K = len(off) - 1, k + int(intercept)
    X = np.zeros((max(B, 1), K))
    status = np.zeros(max(B, 1), np.int32)
    rounds = np.zeros(max(B, 1), np.int32)
    rows32 = np.ascontiguousarray(rows if rows.size else np.zeros(1), np.int32)
    r = np.ascontiguousarray(r if r.size else np.zeros(1), np.float64)
    ip, dp = _lib.IP, _lib.DP
    _lib.check(_lib.lib().mr_fold_in(
        int(device), k, n_rows, T.ctypes.data_as(dp),
        row_offset.ctypes.data_as(dp) if row_offset is not None else None, MODES[mode],
        int(intercept), alpha, reg, rmode, int(nonneg), int(max_rounds), B,
        off.ctypes.data_as(_lib.LLP), rows32.ctypes.data_as(ip), r.ctypes.data_as(dp),
        X.ctypes.data_as(dp), status.ctypes.data_as(ip), rounds.ctypes.data_as(ip)), "mr_fold_in")
    return X[:B], status[:B], rounds[:B]


def fold_in_users(V, lists, reg, reg_mode, nonneg=False, max_rounds=0, device=0):
    """New users of an explicit model from the item table ``V[I, k]``: the
    engine's user half-step (``lists`` hold ``(item, r)`` with ``r`` as the
    model was trained on, e.g. median-subtracted).  Returns ``(X[B, k + 1],
    status, rounds)``, the intercept (user bias) last."""
    return fold_in(V, lists, "explicit", True, None, 0.0, reg, reg_mode, nonneg, max_rounds,
                   device)


def fold_in_items(U, lists, reg, reg_mode, nonneg=False, max_rounds=0, device=0):
    """New items of an explicit model from the user table ``U[n, k + 1]``
    (the user bias last): the engine's item half-step, ``lists`` holding
    ``(user, r)``.  Returns ``(Y[B, k], status, rounds)``."""
    U = np.asarray(U, np.float64)
    if U.ndim != 2 or U.shape[1] < 2:
        raise ValueError("U must be [users, k + 1] with the user bias in the last column")
    return fold_in(U[:, :-1], lists, "explicit", False, U[:, -1], 0.0, reg, reg_mode, nonneg,
                   max_rounds, device)
