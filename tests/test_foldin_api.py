"""CPU: the general fold-in's declaration / binding / export, the Python
face's validation (before any native call) and the C entry point's refusals
that need no device."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def test_symbol_declared_bound_and_exported():
    from movie_recommender_amd import _lib
    src = open(os.path.join(ROOT, "include", "mr_foldin.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.findall(r"^int (\w+)\(", src, flags=re.M) == ["mr_fold_in"]
    assert "MR_FOLD_EXPLICIT = 0" in src and "MR_FOLD_IMPLICIT = 1" in src
    L = _lib.lib()
    assert "mr_fold_in" in _lib.SIGNATURES and hasattr(L, "mr_fold_in")
    n_args = len(re.search(r"int mr_fold_in\((.*?)\);", src, flags=re.S).group(1).split(","))
    assert n_args == len(_lib.SIGNATURES["mr_fold_in"][1]) == 19
    mk = open(os.path.join(ROOT, "movie_recommender_amd", "csrc", "Makefile")).read()
    assert "foldin.hip" in mk and "mr_foldin.h" in mk


@pytest.fixture
def no_native(monkeypatch):
    from movie_recommender_amd import _lib

    def fail():
        raise AssertionError("native library touched before validation")
    monkeypatch.setattr(_lib, "lib", fail)


def test_fold_in_rejects_before_any_native_call(no_native):
    from movie_recommender_amd.foldin import fold_in, fold_in_items, fold_in_users
    T = np.ones((4, 2))
    ok = [[(0, 1.0)], []]
    off = np.array([0, 1], np.int64)
    nan_t, inf_off = T.copy(), np.zeros(4)
    nan_t[2, 1] = np.nan
    inf_off[3] = np.inf
    cases = [
        dict(T=np.ones((4, 129))), dict(T=np.ones((4, 0))), dict(T=np.ones(4)),      # k
        dict(mode="implicit", intercept=True),
        dict(mode="implicit", row_offset=np.zeros(4)),
        dict(mode="ridge"), dict(mode=1), dict(reg_mode="ridge"),
        dict(alpha=-1.0), dict(alpha=float("nan")), dict(alpha="8"),
        dict(reg=-0.1), dict(reg=float("inf")), dict(reg=float("nan")),
        dict(max_rounds=-1), dict(max_rounds=1.5), dict(max_rounds=float("nan")),
        dict(lists=[[(4, 1.0)]]), dict(lists=[[(-1, 1.0)]]), dict(lists=[[(0.5, 1.0)]]),
        dict(lists=[[(0, float("nan"))]]), dict(lists=[[(0, float("inf"))]]),
        dict(mode="implicit", lists=[[(0, -0.5)]]),
        dict(T=nan_t), dict(row_offset=inf_off), dict(row_offset=np.zeros(3)),
        dict(lists=(np.array([1, 1], np.int64), np.array([0]), np.array([1.0]))),   # off[0] != 0
        dict(lists=(np.array([0, 2, 1], np.int64), np.array([0]), np.array([1.0]))),   # decreases
        dict(lists=(off, np.array([0, 1]), np.array([1.0, 1.0]))),                  # off[-1] != len
    ]
    for kw in cases:
        args = dict(T=T, lists=ok)
        args.update(kw)
        with pytest.raises(ValueError):
            fold_in(**args)
    # valid calls reach the library: a negative r is fine in the explicit mode
    for kw in (dict(), dict(lists=[[(0, -0.5)]]), dict(mode="implicit", alpha=0.0),
               dict(intercept=True, row_offset=np.zeros(4), nonneg=True, max_rounds=3),
               dict(lists=(off, np.array([3]), np.array([0.0])), reg_mode="weighted")):
        with pytest.raises(AssertionError, match="native library touched"):
            fold_in(T, **{"lists": ok, **kw})
    for f, tab in ((fold_in_users, T), (fold_in_items, np.ones((4, 3)))):
        for kw in (dict(reg=-1.0), dict(reg_mode="x"), dict(lists=[[(4, 1.0)]]),
                   dict(max_rounds=-2)):
            args = dict(lists=ok, reg=0.5, reg_mode="weighted")
            args.update(kw)
            with pytest.raises(ValueError):
                f(tab, **args)
        with pytest.raises(AssertionError, match="native library touched"):
            f(tab, ok, 0.5, "weighted")
    with pytest.raises(ValueError):
        fold_in_items(np.ones((4, 1)), ok, 0.5, "weighted")       # no factor column


def test_implicit_model_faces_reject_before_any_native_call(no_native):
    from movie_recommender_amd.implicit import ImplicitModel
    model = ImplicitModel(np.ones((3, 2)), np.ones((4, 2)), alpha=8.0, reg=0.5, nonneg=True)
    with pytest.raises(ValueError):
        model.fold_in([[(4, 1.0)]])
    with pytest.raises(ValueError):
        model.fold_in([[(0, -1.0)]])
    with pytest.raises(ValueError):
        model.fold_in_items([[(3, 1.0)]])           # X has 3 rows
    with pytest.raises(AssertionError, match="native library touched"):
        model.fold_in([[(3, 1.0)]])
    with pytest.raises(AssertionError, match="native library touched"):
        model.fold_in_items([[(2, 1.0)]])


def test_signatures():
    from movie_recommender_amd import foldin, implicit
    from movie_recommender_amd.serving import MovieTable
    p = inspect.signature(implicit.fold_in).parameters           # unchanged
    assert list(p) == ["Y", "item_lists", "alpha", "reg", "reg_mode", "device"]
    assert (p["alpha"].default, p["reg"].default, p["reg_mode"].default) == (40.0, 0.01, "constant")
    p = inspect.signature(foldin.fold_in).parameters
    assert list(p) == ["T", "lists", "mode", "intercept", "row_offset", "alpha", "reg", "reg_mode",
                       "nonneg", "max_rounds", "device"]
    assert [p[n].default for n in list(p)[2:]] == ["explicit", False, None, 40.0, 0.01,
                                                   "constant", False, 0, 0]
    for f, first in ((foldin.fold_in_users, "V"), (foldin.fold_in_items, "U")):
        p = inspect.signature(f).parameters
        assert list(p)[:5] == [first, "lists", "reg", "reg_mode", "nonneg"]
        assert p["nonneg"].default is False
    p = inspect.signature(implicit.ImplicitModel.__init__).parameters
    assert list(p) == ["self", "X", "Y", "alpha", "reg", "reg_mode", "device", "nonneg"]
    assert p["nonneg"].default is False
    p = inspect.signature(MovieTable.fold_in_ridge).parameters
    assert list(p) == ["self", "rating_lists", "reg", "reg_mode", "nonneg", "subtract_median"]
    assert (p["reg_mode"].default, p["nonneg"].default, p["subtract_median"].default) == \
        ("weighted", False, True)


def test_c_abi_refuses_without_a_device():
    """Every precondition is checked on the host before the device is
    touched; a refused call writes no output and the library stays usable."""
    from movie_recommender_amd import _lib
    L = _lib.lib()
    ip, dp, llp = _lib.IP, _lib.DP, _lib.LLP
    T = np.ones((4, 3))
    roff = np.zeros(4)
    x = np.full((2, 4), -7.0)
    st, rd = np.full(2, -7, np.int32), np.full(2, -7, np.int32)

    def fold(k=3, mode=0, intercept=0, alpha=8.0, reg=0.5, reg_mode=0, nonneg=0, max_rounds=0,
             off=(0, 1), idx=(0,), r=(1.0,), table=T, row_offset=None):
        off, idx = np.asarray(off, np.int64), np.asarray(idx, np.int32)
        r = np.asarray(r, np.float64)
        return L.mr_fold_in(0, k, 4, table.ctypes.data_as(dp),
                            row_offset.ctypes.data_as(dp) if row_offset is not None else None,
                            mode, intercept, alpha, reg, reg_mode, nonneg, max_rounds,
                            len(off) - 1, off.ctypes.data_as(llp), idx.ctypes.data_as(ip),
                            r.ctypes.data_as(dp), x.ctypes.data_as(dp), st.ctypes.data_as(ip),
                            rd.ctypes.data_as(ip))
    nan_t, nan_off = T.copy(), roff.copy()
    nan_t[1, 2] = np.nan
    nan_off[2] = np.inf
    for kw, word in [(dict(k=0), "1..128"), (dict(k=129), "1..128"),
                     (dict(mode=1, intercept=1), "implicit"),
                     (dict(mode=1, row_offset=roff), "implicit"),
                     (dict(mode=2), "mode"), (dict(reg_mode=2), "mode"),
                     (dict(alpha=-1.0), "alpha"), (dict(alpha=float("nan")), "alpha"),
                     (dict(reg=-0.5), "reg"), (dict(reg=float("inf")), "reg"),
                     (dict(max_rounds=-1), "max_rounds"),
                     (dict(idx=(4,)), "out of range"), (dict(idx=(-1,)), "out of range"),
                     (dict(r=(float("nan"),)), "r must be"),
                     (dict(mode=1, r=(-1.0,)), "r must be"),
                     (dict(table=nan_t), "T must be finite"),
                     (dict(row_offset=nan_off), "row_offset"),
                     (dict(off=(0, 2, 1), idx=(0, 1), r=(1.0, 1.0)), "offsets"),
                     (dict(off=(1, 1), idx=(0,), r=(1.0,)), "offsets")]:
        assert fold(**kw) == -1, kw
        assert word in _lib.last_error(), (kw, _lib.last_error())
    assert np.all(x == -7.0) and np.all(st == -7) and np.all(rd == -7)   # nothing was written
    assert fold(off=(0,), idx=(0,), r=(0.0,)) == 0                        # no entities: a no-op
    assert np.all(x == -7.0)
