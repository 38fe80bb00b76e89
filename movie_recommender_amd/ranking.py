"""Ranking evaluation of a factor model on the GPU: for every held-out
``(user, item)`` pair the rank of the item among all items the user has not
seen, and the metrics built on it (expected percentile rank of Hu, Koren and
Volinsky 2008, precision / recall / NDCG / MRR / hit rate at N).

The score of a pair is ``((sum_j X[u, j] * Y[i, j]) + user_bias[u]) +
item_offset[i]`` in fp64, the sum from 0.0 in index order with every product
and addition rounded on its own -- the arithmetic of ``MovieTable.scores``,
so the bits are the same.  The B x I score matrix is never stored
(``include/mr_ranking.h``, DESIGN.md "Ranking evaluation and implicit
fold-in").  There is no CPU fallback: without the HIP library
``rank_counts`` raises.
"""
import numpy as np

from . import _lib


def _ids(pairs, what, n_users, n_items):
    """(user ids, item ids) as int64 arrays of equal length, range-checked."""
    if pairs is None:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    try:
        u, i = pairs
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a (user_ids, item_ids) pair") from None
    u, i = np.asarray(u), np.asarray(i)
    if u.ndim != 1 or u.shape != i.shape:
        raise ValueError(f"{what}: user_ids and item_ids must be 1-D arrays of equal length")
    if u.size and not (np.issubdtype(u.dtype, np.integer) and np.issubdtype(i.dtype, np.integer)):
        raise ValueError(f"{what}: ids must be integers")
    u, i = u.astype(np.int64), i.astype(np.int64)
    if u.size and (u.min() < 0 or u.max() >= n_users):
        raise ValueError(f"{what}: user id out of range")
    if i.size and (i.min() < 0 or i.max() >= n_items):
        raise ValueError(f"{what}: item id out of range")
    return u, i


def _csr(u, n_users):
    """Stable order of the pairs by user and the int64[n_users + 1] offsets."""
    order = np.argsort(u, kind="stable")
    off = np.zeros(n_users + 1, np.int64)
    np.cumsum(np.bincount(u, minlength=n_users), out=off[1:])
    return order, off


def _vector(v, n, what):
    if v is None:
        return None
    v = np.ascontiguousarray(v, np.float64)
    if v.shape != (n,):
        raise ValueError(f"{what} must have shape ({n},)")
    if not np.all(np.isfinite(v)):
        raise ValueError(f"{what} must be finite")
    return v


def rank_counts(X, Y, test, exclude=None, user_bias=None, item_offset=None, device=0):
    """Rank counts of the held-out pairs ``test = (user_ids, item_ids)`` (any
    order, duplicates allowed) under the factors ``X[B, k]``, ``Y[I, k]``
    (``k <= 512``).  ``exclude = (user_ids, item_ids)`` are the pairs a user
    has already seen (the training set; duplicates are dropped): they leave
    the user's candidate set ``E_u``.  Returns a dict of arrays aligned with
    the input order of ``test``:

    * ``above``        items of ``E_u`` other than the pair's that score higher,
    * ``tied``         ... that score equal (-0.0 equals +0.0),
    * ``tied_before``  the tied ones with a larger item id,
    * ``score``        the pair's own score,

    and per user ``n_eligible[B] = |E_u|``, plus ``kernel_ms`` (HIP-event
    time per kernel class).  ``above + tied_before`` is the pair's 0-based
    position in the (score, id)-descending list ``MovieTable.top_n`` returns.

    ``ValueError`` (before any native call) for factors that are not finite
    2-D arrays of equal width, ids out of range, or a test pair that is also
    excluded."""
    X = np.ascontiguousarray(X, np.float64)
    Y = np.ascontiguousarray(Y, np.float64)
    if X.ndim != 2 or Y.ndim != 2 or X.shape[1] != Y.shape[1]:
        raise ValueError("X and Y must be 2-D arrays with the same number of factors")
    (B, k), n_items = X.shape, Y.shape[0]
    if not 1 <= k <= 512:
        raise ValueError("the number of factors must be in 1..512")
    if not (np.all(np.isfinite(X)) and np.all(np.isfinite(Y))):
        raise ValueError("factors must be finite")
    user_bias = _vector(user_bias, B, "user_bias")
    item_offset = _vector(item_offset, n_items, "item_offset")
    tu, ti = _ids(test, "test", B, n_items)
    eu, ei = _ids(exclude, "exclude", B, n_items)
    ekey = np.unique(eu * max(n_items, 1) + ei)          # de-duplicated, sorted by (user, item)
    if ekey.size and tu.size and np.any(np.isin(tu * n_items + ti, ekey)):
        raise ValueError("a test pair is also excluded")
    order, toff = _csr(tu, B)
    titem = np.ascontiguousarray(ti[order], np.int32)
    eoff = eitem = None
    if ekey.size:
        eoff = np.zeros(B + 1, np.int64)
        np.cumsum(np.bincount(ekey // n_items, minlength=B), out=eoff[1:])
        eitem = np.ascontiguousarray(ekey % n_items, np.int32)
    n = len(tu)
    res = {name: np.zeros(max(n, 1), np.int32) for name in ("above", "tied", "tied_before")}
    score = np.zeros(max(n, 1))
    n_eligible = np.zeros(max(B, 1), np.int32)
    ms = np.zeros(3)
    ip, dp, llp = _lib.IP, _lib.DP, _lib.LLP
    L = _lib.lib()
    _lib.check(L.mr_rank_counts(
        int(device), k, B, n_items, X.ctypes.data_as(dp),
        user_bias.ctypes.data_as(dp) if user_bias is not None else None,
        Y.ctypes.data_as(dp),
        item_offset.ctypes.data_as(dp) if item_offset is not None else None,
        toff.ctypes.data_as(llp), titem.ctypes.data_as(ip) if n else None,
        eoff.ctypes.data_as(llp) if eoff is not None else None,
        eitem.ctypes.data_as(ip) if eitem is not None else None,
        res["above"].ctypes.data_as(ip), res["tied"].ctypes.data_as(ip),
        res["tied_before"].ctypes.data_as(ip), score.ctypes.data_as(dp),
        n_eligible.ctypes.data_as(ip), ms.ctypes.data_as(dp)), "mr_rank_counts")
    out = {}
    for name, a in list(res.items()) + [("score", score)]:
        b = np.empty(n, a.dtype)
        b[order] = a[:n]                                  # back to the input order
        out[name] = b
    out["n_eligible"] = n_eligible[:B]
    out["kernel_ms"] = dict(zip(["pair_scores", "tile_counts", "exclusions"], ms.tolist()))
    return out


def metrics_from_counts(counts, test_users, n=10, weights=None):
    """Ranking metrics from ``rank_counts``' output (host only).

    Per pair: ``pos = above + tied_before`` and the percentile rank ``pr =
    (above + 0.5 tied) / (n_eligible - 1)`` (0 best, 1 worst; a tie counts as
    half).  Pairs of users with fewer than 2 eligible items have no rank:
    they are dropped from every metric and counted in ``n_dropped``.

    ``mpr = sum w pr / sum w`` (``weights`` per pair, default 1) is the
    expected percentile rank: 0 is best, 0.5 is random.  Per user with at
    least one remaining pair (``users``, ascending): ``hits = #(pos < n)``,
    ``precision = hits / n``, ``recall = hits / n_test``, ``ndcg`` with binary
    gains (DCG = sum over pos < n of 1 / log2(pos + 2), IDCG the same sum over
    the first min(n_test, n) positions) and ``rr = 1 / (min pos + 1)``.  The
    means over those users are ``precision``, ``recall``, ``ndcg``, ``mrr``
    and ``hit_rate`` (share of users with a hit); the per-user arrays are
    under ``per_user``."""
    n = int(n)
    if n < 1:
        raise ValueError("n must be >= 1")
    tu = np.asarray(test_users, np.int64)
    above = np.asarray(counts["above"], np.int64)
    tied = np.asarray(counts["tied"], np.int64)
    pos = above + np.asarray(counts["tied_before"], np.int64)
    n_el = np.asarray(counts["n_eligible"], np.int64)
    if not (tu.shape == above.shape == tied.shape == pos.shape) or tu.ndim != 1:
        raise ValueError("counts and test_users must be 1-D arrays of equal length")
    w = np.ones(len(tu)) if weights is None else np.asarray(weights, np.float64)
    if w.shape != tu.shape or not np.all(np.isfinite(w)) or np.any(w < 0):
        raise ValueError("weights must be finite, >= 0 and aligned with the test pairs")
    keep = n_el[tu] >= 2 if len(tu) else np.zeros(0, bool)
    n_dropped = int(len(tu) - keep.sum())
    tu, above, tied, pos, w = tu[keep], above[keep], tied[keep], pos[keep], w[keep]
    pr = (above + 0.5 * tied) / (n_el[tu] - 1)
    wsum = float(w.sum())
    mpr = float(np.dot(w, pr) / wsum) if wsum > 0 else float("nan")
    users, inv = np.unique(tu, return_inverse=True)
    nu = len(users)
    n_test = np.bincount(inv, minlength=nu)
    hit = pos < n
    hits = np.bincount(inv, weights=hit, minlength=nu)
    dcg = np.bincount(inv, weights=np.where(hit, 1.0 / np.log2(pos + 2.0), 0.0), minlength=nu)
    ideal = np.concatenate([[0.0], np.cumsum(1.0 / np.log2(np.arange(n) + 2.0))])
    idcg = ideal[np.minimum(n_test, n)]
    best = np.full(nu, np.iinfo(np.int64).max)
    np.minimum.at(best, inv, pos)
    per_user = {"users": users, "n_test": n_test, "hits": hits.astype(np.int64),
                "precision": hits / n, "recall": hits / np.maximum(n_test, 1),
                "ndcg": dcg / np.where(idcg > 0, idcg, 1.0), "rr": 1.0 / (best + 1.0)}

    def mean(a):
        return float(np.mean(a)) if nu else float("nan")
    return {"mpr": mpr, "n": n, "n_pairs": int(len(tu)), "n_dropped": n_dropped, "n_users": nu,
            "precision": mean(per_user["precision"]), "recall": mean(per_user["recall"]),
            "ndcg": mean(per_user["ndcg"]), "mrr": mean(per_user["rr"]),
            "hit_rate": mean(hits > 0), "percentile_rank": pr, "kept": keep,
            "per_user": per_user}


def rank_eval(X, Y, test, exclude=None, n=10, weights=None, user_bias=None, item_offset=None,
              device=0):
    """``rank_counts`` then ``metrics_from_counts``; the counts are returned
    under ``"counts"``."""
    counts = rank_counts(X, Y, test, exclude, user_bias, item_offset, device)
    out = metrics_from_counts(counts, np.asarray(test[0]), n, weights)
    out["counts"] = counts
    return out
