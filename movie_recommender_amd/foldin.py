"""Fold-in for every trained model (``include/mr_foldin.h``, DESIGN.md
"Fold-in"): factors of users or items that were not in the training set, from
the opposite factor table, by the half-step the model was trained with.

* explicit models (``als_train_regularized``): the ridge system of ALS-WR,
  with the user intercept (``fold_in_users``) or the users' intercepts as row
  offsets (``fold_in_items``);
* implicit models (``als_implicit``): ``mode="implicit"``;
* ``nonneg=True``: the exact non-negative minimiser (``solver="nnls"``).

``explain`` (``include/mr_explain.h``, DESIGN.md "Explanations") splits the
score of a target row over the entries of the entity's own list: "because you
rated X and Y".

Everything runs in fp64 on one GPU; there is no CPU fallback.
"""
import numpy as np

from . import _lib
from .engine import check_implicit, check_regularization
from .implicit import _lists_csr

MAX_K = 128
MODES = {"explicit": 0, "implicit": 1}   # MR_FOLD_* of include/mr_foldin.h
MAX_TOP = 64                             # mr_explain's largest top
PHI_CHUNK = (1 << 28) // 8               # doubles of one entity's phi block mr_explain accepts


def _checked(T, lists, mode, intercept, row_offset, alpha, reg, reg_mode):
    """The validation ``fold_in`` and ``explain`` share; ``ValueError`` or
    ``(T, row_offset, alpha, reg, rmode, off, rows, r)``."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {sorted(MODES)}, not {mode!r}")
    implicit = mode == "implicit"
    if implicit and (intercept or row_offset is not None):
        raise ValueError("the implicit mode takes no intercept and no row_offset")
    alpha = check_implicit(alpha)
    reg, rmode = check_regularization(reg, reg_mode)
    T = np.ascontiguousarray(T, np.float64)
    if T.ndim != 2 or not 1 <= T.shape[1] <= MAX_K:
        raise ValueError(f"T must be [rows, k] with k in 1..{MAX_K}")
    if not np.all(np.isfinite(T)):
        raise ValueError("factors must be finite")
    n_rows = T.shape[0]
    if row_offset is not None:
        row_offset = np.ascontiguousarray(row_offset, np.float64)
        if row_offset.shape != (n_rows,) or not np.all(np.isfinite(row_offset)):
            raise ValueError("row_offset must be finite f64[rows of T]")
    off, rows, r = _lists_csr(lists)
    if rows.size and (rows.min() < 0 or rows.max() >= n_rows):
        raise ValueError("id out of range")
    if not np.all(np.isfinite(r)) or (implicit and np.any(r < 0)):
        raise ValueError("r must be finite" + (" and >= 0" if implicit else ""))
    return T, row_offset, alpha, reg, rmode, off, rows, r


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
    intercept, nonneg = bool(intercept), bool(nonneg)
    T, row_offset, alpha, reg, rmode, off, rows, r = _checked(
        T, lists, mode, intercept, row_offset, alpha, reg, reg_mode)
    if isinstance(max_rounds, bool) or not isinstance(max_rounds, (int, np.integer)) or \
            not 0 <= max_rounds < 2 ** 31:
        raise ValueError("max_rounds must be an integer >= 0")
    n_rows, k = T.shape
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


class Explanation:
    """What ``explain`` returns.  ``x[B, K]`` and ``status[B]`` are
    ``fold_in``'s; ``score[e]`` is an array with ``A_t . x`` per target of
    entity ``e`` (row offsets or medians not added); ``top[e][q]`` is the list
    ``[(row of T, position in the entity's list, contribution)]`` of target
    ``q``, largest contribution first; ``phi[e]`` is the full ``[Q_e, M_e]``
    array of contributions, or ``None`` without ``full``."""

    __slots__ = ("x", "status", "score", "top", "phi")

    def __init__(self, x, status, score, top, phi):
        self.x, self.status, self.score, self.top, self.phi = x, status, score, top, phi


def _targets_csr(targets, B):
    """(offsets int64[B + 1], rows int64) of ``targets``: a sequence of row
    lists, one per entity, or a CSR pair ``(offsets, rows)`` whose first member
    is an ndarray."""
    if isinstance(targets, tuple) and len(targets) == 2 and isinstance(targets[0], np.ndarray):
        toff = np.ascontiguousarray(targets[0], np.int64)
        rows = np.asarray(targets[1])
        if toff.ndim != 1 or toff.size < 1 or toff[0] != 0 or np.any(np.diff(toff) < 0) or \
                rows.ndim != 1 or toff[-1] != len(rows):
            raise ValueError("target offsets must be int64[B + 1], non-decreasing, from 0 to "
                             "len(rows)")
    else:
        tl = [list(t) for t in targets]
        toff = np.zeros(len(tl) + 1, np.int64)
        toff[1:] = np.cumsum([len(t) for t in tl])
        rows = np.array([t for l in tl for t in l])
    if rows.size and not np.issubdtype(rows.dtype, np.integer):
        raise ValueError("target ids must be integers")
    if len(toff) - 1 != B:
        raise ValueError("targets must hold one row list per entity")
    return toff, rows.astype(np.int64)


def explain_arrays(T, lists, targets, mode="explicit", intercept=False, row_offset=None,
                   alpha=40.0, reg=0.01, reg_mode="constant", top=10, full=False, device=0):
    """``explain`` without the per-entity Python objects, for large batches:
    the flat arrays of ``include/mr_explain.h`` as a dict -- ``x``, ``status``,
    ``off`` / ``rows`` (the lists' CSR), ``toff`` (targets' CSR offsets),
    ``score[nt]``, ``top_pos[nt, top]``, ``top_val[nt, top]``, ``top_cnt[nt]``
    and, with ``full``, ``poff`` and ``phi``."""
    intercept = bool(intercept)
    T, row_offset, alpha, reg, rmode, off, rows, r = _checked(
        T, lists, mode, intercept, row_offset, alpha, reg, reg_mode)
    if isinstance(top, bool) or not isinstance(top, (int, np.integer)) or \
            not 0 <= top <= MAX_TOP:
        raise ValueError(f"top must be an integer in 0..{MAX_TOP}")
    top = int(top)
    n_rows, k = T.shape
    B, K = len(off) - 1, k + int(intercept)
    toff, trows = _targets_csr(targets, B)
    if trows.size and (trows.min() < 0 or trows.max() >= n_rows):
        raise ValueError("target id out of range")
    Q, M = np.diff(toff), np.diff(off)
    poff = np.zeros(B + 1, np.int64)
    if full:
        if B and np.max(Q * M) > PHI_CHUNK:
            raise ValueError("the contributions of one entity exceed 256 MiB; ask for fewer "
                             "targets at a time")
        poff[1:] = np.cumsum(Q * M)
    nt = int(toff[-1])
    X = np.zeros((max(B, 1), K))
    status = np.zeros(max(B, 1), np.int32)
    score = np.zeros(max(nt, 1))
    phi = np.zeros(max(int(poff[-1]), 1)) if full else None
    tpos = np.full((max(nt, 1), top), -1, np.int32)
    tval = np.zeros((max(nt, 1), top))
    tcnt = np.zeros(max(nt, 1), np.int32)
    rows32 = np.ascontiguousarray(rows if rows.size else np.zeros(1), np.int32)
    r = np.ascontiguousarray(r if r.size else np.zeros(1), np.float64)
    trows32 = np.ascontiguousarray(trows if trows.size else np.zeros(1), np.int32)
    ip, dp, llp = _lib.IP, _lib.DP, _lib.LLP
    _lib.check(_lib.lib().mr_explain(
        int(device), k, n_rows, T.ctypes.data_as(dp),
        row_offset.ctypes.data_as(dp) if row_offset is not None else None, MODES[mode],
        int(intercept), alpha, reg, rmode, B, off.ctypes.data_as(llp), rows32.ctypes.data_as(ip),
        r.ctypes.data_as(dp), toff.ctypes.data_as(llp), trows32.ctypes.data_as(ip), top,
        X.ctypes.data_as(dp), status.ctypes.data_as(ip), score.ctypes.data_as(dp),
        poff.ctypes.data_as(llp) if full else None, phi.ctypes.data_as(dp) if full else None,
        tpos.ctypes.data_as(ip), tval.ctypes.data_as(dp), tcnt.ctypes.data_as(ip)), "mr_explain")
    out = dict(x=X[:B], status=status[:B], off=off, rows=rows, toff=toff, score=score[:nt],
               top_pos=tpos[:nt], top_val=tval[:nt], top_cnt=tcnt[:nt])
    if full:
        out.update(poff=poff, phi=phi[:int(poff[-1])])
    return out


def explain(T, lists, targets, mode="explicit", intercept=False, row_offset=None, alpha=40.0,
            reg=0.01, reg_mode="constant", top=10, full=False, device=0):
    """Why a target row scores what it scores: with ``fold_in``'s system ``G x
    = c`` of an entity (``nonneg=False``), ``c = sum_j coef_j A_j``, so for a
    target row ``t`` of ``T``

        ``A_t . x = sum_j phi[t, j]``,  ``phi[t, j] = coef_j A_t^T G^-1 A_j``,

    ``A = [a, 1]`` with ``intercept``; ``coef_j = r_j - row_offset[row_j]``
    (explicit) or ``1 + alpha r_j`` (implicit).  ``phi[t, j]`` is what entry
    ``j`` of the entity's list contributes to the score of ``t``.

    ``T``, ``lists`` and the form are ``fold_in``'s.  ``targets`` is a
    sequence of row lists, one per entity (empty and repeated rows are fine),
    or a CSR pair ``(offsets int64[B + 1], rows)``.  Per target the ``top``
    (0 .. 64) largest contributions are selected on the GPU: descending, equal
    values by the smaller list position.  ``full=True`` also returns every
    contribution.  An entity with status 0 or an empty list has zero scores
    and empty top lists.  Returns an ``Explanation``.

    ``ValueError`` before any native call for everything the C entry point
    refuses."""
    a = explain_arrays(T, lists, targets, mode, intercept, row_offset, alpha, reg, reg_mode, top,
                       full, device)
    off, rows, toff = a["off"], a["rows"], a["toff"]
    score, tpos, tval, tcnt = a["score"], a["top_pos"], a["top_val"], a["top_cnt"]
    B = len(off) - 1
    Q, M = np.diff(toff), np.diff(off)
    if full:
        poff, phi = a["poff"], a["phi"]
    scores, tops, phis = [], [], ([] if full else None)
    for e in range(B):
        lrows = rows[off[e]:off[e + 1]]
        scores.append(score[toff[e]:toff[e + 1]].copy())
        per = []
        for t in range(int(toff[e]), int(toff[e + 1])):
            pos = tpos[t, :tcnt[t]]
            per.append(list(zip(lrows[pos].tolist(), pos.tolist(), tval[t, :tcnt[t]].tolist())))
        tops.append(per)
        if full:
            phis.append(phi[poff[e]:poff[e + 1]].reshape(int(Q[e]), int(M[e])).copy())
    return Explanation(a["x"], a["status"], scores, tops, phis)


def explain_users(V, lists, targets, reg, reg_mode, top=10, full=False, device=0):
    """``explain`` for new users of an explicit model, the tables and lists of
    ``fold_in_users``: ``targets`` are items, the score is ``V[t] . x[:k] +
    x[k]`` (the user bias contributes through every rating's share of it)."""
    return explain(V, lists, targets, "explicit", True, None, 0.0, reg, reg_mode, top, full,
                   device)


def explain_items(U, lists, targets, reg, reg_mode, top=10, full=False, device=0):
    """``explain`` for new items of an explicit model, the tables and lists of
    ``fold_in_items``: ``targets`` are users, the score is ``U[t, :k] . y``
    (the caller adds the user's bias ``U[t, k]``)."""
    U = np.asarray(U, np.float64)
    if U.ndim != 2 or U.shape[1] < 2:
        raise ValueError("U must be [users, k + 1] with the user bias in the last column")
    return explain(U[:, :-1], lists, targets, "explicit", False, U[:, -1], 0.0, reg, reg_mode,
                   top, full, device)
