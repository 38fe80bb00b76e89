"""CPU: the ranking metrics against values worked by hand, the Python face's
validation (before any native call), the C ABI's refusals that need no
device, and the declaration / export of the new entry points."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT


# ---------------------------------------------------------------------------
# metrics_from_counts by hand
# ---------------------------------------------------------------------------
def hand_counts():
    """User 0 (21 eligible items): positions 0, 3 and 12 of its three pairs,
    the second in a tie of three (one tied item before it).  User 1 (1
    eligible item): dropped.  User 2 (5 eligible): one pair at position 4."""
    return {"above": np.array([0, 2, 12, 0, 4]), "tied": np.array([0, 2, 0, 0, 0]),
            "tied_before": np.array([0, 1, 0, 0, 0]), "n_eligible": np.array([21, 1, 5])}, \
        np.array([0, 0, 0, 1, 2])


def test_metrics_by_hand():
    from movie_recommender_amd.ranking import metrics_from_counts
    counts, users = hand_counts()
    m = metrics_from_counts(counts, users, n=5)
    assert m["n_dropped"] == 1 and m["n_pairs"] == 4 and m["n_users"] == 2
    pr = np.array([0 / 20, (2 + 0.5 * 2) / 20, 12 / 20, 4 / 4])
    assert np.allclose(m["percentile_rank"], pr, rtol=0, atol=1e-15)
    assert m["mpr"] == pytest.approx(pr.mean(), abs=1e-15)
    pu = m["per_user"]
    assert pu["users"].tolist() == [0, 2] and pu["n_test"].tolist() == [3, 1]
    assert pu["hits"].tolist() == [2, 1]                  # positions 0, 3 | 4 are < 5
    assert pu["precision"].tolist() == [2 / 5, 1 / 5]
    assert pu["recall"].tolist() == [2 / 3, 1.0]
    idcg3 = 1 / np.log2(2) + 1 / np.log2(3) + 1 / np.log2(4)
    ndcg = [(1 / np.log2(2) + 1 / np.log2(5)) / idcg3, (1 / np.log2(6)) / 1.0]
    assert np.allclose(pu["ndcg"], ndcg, rtol=0, atol=1e-15)
    assert pu["rr"].tolist() == [1.0, 1 / 5]
    assert m["precision"] == pytest.approx(0.3) and m["recall"] == pytest.approx(5 / 6)
    assert m["ndcg"] == pytest.approx(np.mean(ndcg)) and m["mrr"] == pytest.approx(0.6)
    assert m["hit_rate"] == 1.0
    # n = 3: user 0 keeps one hit (position 0), user 2 none; IDCG over min(n_test, n)
    m3 = metrics_from_counts(counts, users, n=3)
    assert m3["per_user"]["hits"].tolist() == [1, 0] and m3["hit_rate"] == 0.5
    assert m3["per_user"]["ndcg"][0] == pytest.approx(1.0 / idcg3)
    assert m3["per_user"]["rr"].tolist() == [1.0, 1 / 5]  # rr does not depend on n


def test_metrics_weights_and_empty():
    from movie_recommender_amd.ranking import metrics_from_counts
    counts, users = hand_counts()
    w = np.array([1.0, 3.0, 0.0, 100.0, 4.0])            # the dropped pair's weight is ignored
    m = metrics_from_counts(counts, users, n=5, weights=w)
    assert m["mpr"] == pytest.approx((1 * 0 + 3 * 0.15 + 0 + 4 * 1.0) / 8.0, abs=1e-15)
    none = metrics_from_counts({"above": np.zeros(0, int), "tied": np.zeros(0, int),
                                "tied_before": np.zeros(0, int),
                                "n_eligible": np.array([4])}, np.zeros(0, int))
    assert none["n_pairs"] == 0 and np.isnan(none["mpr"]) and np.isnan(none["precision"])
    for bad in ({"weights": w[:3]}, {"weights": -w}, {"n": 0}):
        with pytest.raises(ValueError):
            metrics_from_counts(counts, users, **bad)


# ---------------------------------------------------------------------------
# validation precedes the native call
# ---------------------------------------------------------------------------
@pytest.fixture
def no_native(monkeypatch):
    from movie_recommender_amd import _lib

    def fail():
        raise AssertionError("native library touched before validation")
    monkeypatch.setattr(_lib, "lib", fail)


def test_rank_counts_rejects_before_any_native_call(no_native):
    from movie_recommender_amd.ranking import rank_counts
    X, Y = np.ones((3, 2)), np.ones((4, 2))
    ok = (np.array([0, 2]), np.array([1, 3]))
    nan_x, inf_y = X.copy(), Y.copy()
    nan_x[1, 1] = np.nan
    inf_y[0, 0] = np.inf
    cases = [
        dict(X=nan_x), dict(Y=inf_y), dict(X=np.ones((3, 3))), dict(X=np.ones(3)),
        dict(X=np.ones((3, 513)), Y=np.ones((4, 513))),
        dict(test=(np.array([0, 3]), np.array([1, 1]))),       # user id out of range
        dict(test=(np.array([0, 1]), np.array([1, 4]))),       # item id out of range
        dict(test=(np.array([0, -1]), np.array([1, 1]))),
        dict(test=(np.array([0.0]), np.array([1.0]))),         # not integers
        dict(test=(np.array([0, 1]), np.array([1]))),
        dict(exclude=(np.array([0]), np.array([4]))),
        dict(exclude=(np.array([1, 2, 2]), np.array([0, 3, 3]))),   # test pair (2, 3) excluded
        dict(user_bias=np.ones(4)), dict(item_offset=np.array([0, 0, 0, np.nan])),
    ]
    for kw in cases:
        args = dict(X=X, Y=Y, test=ok)
        args.update(kw)
        with pytest.raises(ValueError):
            rank_counts(**args)
    with pytest.raises(AssertionError, match="native library touched"):
        rank_counts(X, Y, ok, (np.array([1, 1]), np.array([0, 0])))   # valid: reaches the library


def test_fold_in_rejects_before_any_native_call(no_native):
    from movie_recommender_amd.implicit import ImplicitModel, fold_in
    Y = np.ones((4, 2))
    ok = [[(0, 1.0)], []]
    off = np.array([0, 1], np.int64)
    cases = [
        dict(alpha=-1.0), dict(alpha=float("nan")), dict(alpha="8"), dict(reg=-0.1),
        dict(reg=float("inf")), dict(reg_mode="ridge"),
        dict(Y=np.ones((4, 129))), dict(Y=np.ones(4)), dict(Y=np.full((4, 2), np.nan)),
        dict(item_lists=[[(4, 1.0)]]), dict(item_lists=[[(-1, 1.0)]]),
        dict(item_lists=[[(0, -0.5)]]), dict(item_lists=[[(0, float("nan"))]]),
        dict(item_lists=[[(0.5, 1.0)]]),
        dict(item_lists=(off, np.array([0, 1]), np.array([1.0, 1.0]))),       # off[-1] != len
        dict(item_lists=(np.array([1, 1], np.int64), np.array([0]), np.array([1.0]))),
        dict(item_lists=(off, np.array([0]), np.array([1.0, 2.0]))),
    ]
    for kw in cases:
        args = dict(Y=Y, item_lists=ok)
        args.update(kw)
        with pytest.raises(ValueError):
            fold_in(**args)
    with pytest.raises(AssertionError, match="native library touched"):
        fold_in(Y, ok)
    with pytest.raises(AssertionError, match="native library touched"):
        fold_in(Y, (off, np.array([3]), np.array([0.0])), reg_mode="weighted")
    for kw in (dict(alpha=-1.0), dict(reg=-1.0), dict(reg_mode="x"), dict(X=np.ones((3, 3)))):
        args = dict(X=np.ones((3, 2)), Y=Y)
        args.update(kw)
        with pytest.raises(ValueError):
            ImplicitModel(**args)
    model = ImplicitModel(np.ones((3, 2)), Y, alpha=8.0, reg=0.5, reg_mode="weighted")
    with pytest.raises(ValueError):
        model.fold_in([[(9, 1.0)]])
    with pytest.raises(ValueError):
        model.rank_eval((np.array([5]), np.array([0])))


def test_als_implicit_signature_is_unchanged():
    import inspect
    from movie_recommender_amd import implicit
    assert list(inspect.signature(implicit.als_implicit).parameters) == [
        "user_ids", "item_ids", "confidence", "k", "num_users", "num_items", "alpha", "reg",
        "reg_mode", "solver", "max_iterations", "tol", "seed"]
    p = inspect.signature(implicit.fold_in).parameters
    assert list(p) == ["Y", "item_lists", "alpha", "reg", "reg_mode", "device"]
    assert (p["alpha"].default, p["reg"].default, p["reg_mode"].default) == (40.0, 0.01, "constant")


# ---------------------------------------------------------------------------
# the C ABI: declared, bound, exported; refusals that need no device
# ---------------------------------------------------------------------------
NEW = ["mr_rank_counts", "mr_rank_set_tuning", "mr_implicit_fold_in"]


def test_symbols_declared_bound_and_exported():
    from movie_recommender_amd import _lib
    src = open(os.path.join(ROOT, "include", "mr_ranking.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = re.findall(r"^int (\w+)\(", src, flags=re.M)
    assert sorted(declared) == sorted(NEW)
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    n_args = {n: len(re.search(rf"int {n}\((.*?)\);", src, flags=re.S).group(1).split(","))
              for n in NEW}
    assert n_args == {n: len(_lib.SIGNATURES[n][1]) for n in NEW}
    mk = open(os.path.join(ROOT, "movie_recommender_amd", "csrc", "Makefile")).read()
    assert "ranking.hip" in mk and "mr_ranking.h" in mk


def test_c_abi_refuses_without_a_device():
    """Every precondition is checked on the host before the device is
    touched, so the refusals and their messages can be seen anywhere."""
    from movie_recommender_amd import _lib
    L = _lib.lib()
    ip, dp, llp = _lib.IP, _lib.DP, _lib.LLP
    X, Y = np.ones((2, 3)), np.ones((4, 3))
    out = [np.full(4, -7, np.int32) for _ in range(3)]
    ne = np.full(2, -7, np.int32)

    def counts(k, toff, titem, eoff=None, eitem=None):
        toff, titem = np.asarray(toff, np.int64), np.asarray(titem, np.int32)
        eo = np.asarray(eoff, np.int64) if eoff is not None else None
        ei = np.asarray(eitem, np.int32) if eitem is not None else None
        return L.mr_rank_counts(0, k, 2, 4, X.ctypes.data_as(dp), None, Y.ctypes.data_as(dp), None,
                                toff.ctypes.data_as(llp), titem.ctypes.data_as(ip),
                                eo.ctypes.data_as(llp) if eo is not None else None,
                                ei.ctypes.data_as(ip) if ei is not None else None,
                                out[0].ctypes.data_as(ip), out[1].ctypes.data_as(ip),
                                out[2].ctypes.data_as(ip), None, ne.ctypes.data_as(ip), None)
    for args, word in [((0, [0, 1, 2], [0, 1]), "1..512"), ((513, [0, 1, 2], [0, 1]), "1..512"),
                       ((3, [0, 1, 2], [0, 4]), "out of range"),
                       ((3, [0, 1, 2], [0, -1]), "out of range"),
                       ((3, [0, 2, 1], [0, 1]), "offsets"), ((3, [1, 1, 2], [0, 1]), "offsets"),
                       ((3, [0, 1, 2], [0, 1], [0, 2, 2], [1, 1]), "duplicate"),
                       ((3, [0, 1, 2], [0, 1], [0, 1, 3], [2, 3, 1]), "also excluded"),
                       ((3, [0, 1, 2], [0, 1], [0, 1, 2], [2, 9]), "out of range"),
                       ((3, [0, 1, 2], [0, 1], [0, 2, 1], [2, 3]), "offsets")]:
        assert counts(*args) == -1, args
        assert word in _lib.last_error(), (args, _lib.last_error())
    assert all(np.all(a == -7) for a in out) and np.all(ne == -7)   # nothing was written
    # no test pairs: answered on the host (n_eligible only)
    assert counts(3, [0, 0, 0], [0], [0, 1, 3], [2, 3, 1]) == 0
    assert ne.tolist() == [3, 2]

    def fold(k, alpha, reg, mode, off, item, r, n_items=4):
        off, item = np.asarray(off, np.int64), np.asarray(item, np.int32)
        r = np.asarray(r, np.float64)
        x = np.zeros((len(off) - 1, max(k, 1)))
        return L.mr_implicit_fold_in(0, k, n_items, Y.ctypes.data_as(dp), alpha, reg, mode,
                                     len(off) - 1, off.ctypes.data_as(llp),
                                     item.ctypes.data_as(ip), r.ctypes.data_as(dp),
                                     x.ctypes.data_as(dp), None)
    good = ([0, 1], [0], [1.0])
    for args, word in [((0, 8.0, 0.5, 0) + good, "1..128"), ((129, 8.0, 0.5, 0) + good, "1..128"),
                       ((3, -1.0, 0.5, 0) + good, "alpha"),
                       ((3, float("nan"), 0.5, 0) + good, "alpha"),
                       ((3, 8.0, -0.5, 0) + good, "reg"),
                       ((3, 8.0, float("inf"), 0) + good, "reg"),
                       ((3, 8.0, 0.5, 2) + good, "mode"),
                       ((3, 8.0, 0.5, 0, [0, 1], [4], [1.0]), "out of range"),
                       ((3, 8.0, 0.5, 0, [0, 1], [0], [-1.0]), "r must be"),
                       ((3, 8.0, 0.5, 0, [0, 1], [0], [float("nan")]), "r must be"),
                       ((3, 8.0, 0.5, 0, [0, 2, 1], [0, 1], [1.0, 1.0]), "offsets")]:
        assert fold(*args) == -1, args
        assert word in _lib.last_error(), (args, _lib.last_error())
    assert L.mr_rank_set_tuning(0, 0, 2049) == -1 and L.mr_rank_set_tuning(0, 70000, 0) == -1
    assert L.mr_rank_set_tuning(0, 0, 0) == 0
