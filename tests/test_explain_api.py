"""CPU: the explanations' declaration / binding / export, the Python faces'
validation (before any native call) and the C entry point's refusals that need
no device.  The NumPy restatement of explain_cases.py is checked against
itself as well: the contributions of a target sum to its score."""
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def test_symbol_declared_bound_and_exported():
    from movie_recommender_amd import _lib
    src = open(os.path.join(ROOT, "include", "mr_explain.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.findall(r"^int (\w+)\(", src, flags=re.M) == ["mr_explain"]
    L = _lib.lib()
    assert "mr_explain" in _lib.SIGNATURES and hasattr(L, "mr_explain")
    n_args = len(re.search(r"int mr_explain\((.*?)\);", src, flags=re.S).group(1).split(","))
    assert n_args == len(_lib.SIGNATURES["mr_explain"][1]) == 25
    mk = open(os.path.join(ROOT, "movie_recommender_amd", "csrc", "Makefile")).read()
    assert "explain.hip" in mk and "mr_explain.h" in mk and "foldin_device.h" in mk


@pytest.fixture
def no_native(monkeypatch):
    from movie_recommender_amd import _lib

    def fail():
        raise AssertionError("native library touched before validation")
    monkeypatch.setattr(_lib, "lib", fail)


def test_explain_rejects_before_any_native_call(no_native):
    from movie_recommender_amd.foldin import explain, explain_arrays, explain_items, explain_users
    T = np.ones((4, 2))
    ok, tg = [[(0, 1.0)], []], [[1, 3], []]
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
        dict(lists=[[(4, 1.0)], []]), dict(lists=[[(-1, 1.0)], []]),
        dict(lists=[[(0.5, 1.0)], []]),
        dict(lists=[[(0, float("nan"))], []]), dict(lists=[[(0, float("inf"))], []]),
        dict(mode="implicit", lists=[[(0, -0.5)], []]),
        dict(T=nan_t), dict(row_offset=inf_off), dict(row_offset=np.zeros(3)),
        dict(lists=(np.array([1, 1], np.int64), np.array([0]), np.array([1.0])), targets=[[1]]),
        dict(lists=(off, np.array([0, 1]), np.array([1.0, 1.0])), targets=[[1]]),
        dict(top=-1), dict(top=65), dict(top=2.5), dict(top=True), dict(top=None),
        dict(targets=[[4], []]), dict(targets=[[-1], []]), dict(targets=[[0.5], []]),
        dict(targets=[[1]]), dict(targets=[[1], [], []]),                # one list per entity
        dict(targets=(np.array([1, 1, 1], np.int64), np.array([], np.int64))),   # off[0] != 0
        dict(targets=(np.array([0, 2, 1], np.int64), np.array([0]))),            # decreases
        dict(targets=(np.array([0, 1, 1], np.int64), np.array([0, 1]))),         # off[-1] != len
    ]
    for f in (explain, explain_arrays):
        for kw in cases:
            args = dict(T=T, lists=ok, targets=tg)
            args.update(kw)
            with pytest.raises(ValueError):
                f(**args)
        # valid calls reach the library
        for kw in (dict(), dict(top=0), dict(top=64, full=True), dict(mode="implicit", alpha=0.0),
                   dict(intercept=True, row_offset=np.zeros(4)), dict(targets=[[], []]),
                   dict(targets=[[1, 1, 1], [0]]),
                   dict(targets=(np.array([0, 2, 2], np.int64), np.array([3, 3])))):
            with pytest.raises(AssertionError, match="native library touched"):
                f(T, **{"lists": ok, "targets": tg, **kw})
    # one entity whose own block is over 256 MiB, only when the block is asked for
    big = (np.array([0, 6000], np.int64), np.zeros(6000, np.int64), np.ones(6000))
    big_t = (np.array([0, 6000], np.int64), np.zeros(6000, np.int64))
    with pytest.raises(ValueError, match="256 MiB"):
        explain_arrays(T, big, big_t, full=True)
    with pytest.raises(AssertionError, match="native library touched"):
        explain_arrays(T, big, big_t)
    for f, tab in ((explain_users, T), (explain_items, np.ones((4, 3)))):
        for kw in (dict(reg=-1.0), dict(reg_mode="x"), dict(lists=[[(4, 1.0)], []]),
                   dict(targets=[[4], []]), dict(top=65)):
            args = dict(lists=ok, targets=tg, reg=0.5, reg_mode="weighted")
            args.update(kw)
            with pytest.raises(ValueError):
                f(tab, **args)
        with pytest.raises(AssertionError, match="native library touched"):
            f(tab, ok, tg, 0.5, "weighted")
    with pytest.raises(ValueError):
        explain_items(np.ones((4, 1)), ok, tg, 0.5, "weighted")       # no factor column


def test_model_faces_reject_before_any_native_call(no_native):
    from movie_recommender_amd.implicit import ImplicitModel
    model = ImplicitModel(np.ones((3, 2)), np.ones((4, 2)), alpha=8.0, reg=0.5)
    with pytest.raises(ValueError):
        model.explain([[(4, 1.0)]], [[0]])
    with pytest.raises(ValueError):
        model.explain([[(0, 1.0)]], [[4]])
    with pytest.raises(ValueError):
        model.explain_items([[(0, 1.0)]], [[3]])          # X has 3 rows
    with pytest.raises(ValueError):
        model.explain([[(0, 1.0)]], [[0]], top=65)
    with pytest.raises(AssertionError, match="native library touched"):
        model.explain([[(3, 1.0)]], [[3]])
    with pytest.raises(AssertionError, match="native library touched"):
        model.explain_items([[(2, 1.0)]], [[2]], top=3, full=True)
    nn = ImplicitModel(np.ones((3, 2)), np.ones((4, 2)), alpha=8.0, reg=0.5, nonneg=True)
    for f in (nn.explain, nn.explain_items):
        with pytest.raises(ValueError, match="nonneg"):
            f([[(0, 1.0)]], [[0]])


def test_signatures():
    from movie_recommender_amd import foldin, implicit
    from movie_recommender_amd.serving import MovieTable
    p = inspect.signature(foldin.explain).parameters
    assert list(p) == ["T", "lists", "targets", "mode", "intercept", "row_offset", "alpha", "reg",
                       "reg_mode", "top", "full", "device"]
    assert [p[n].default for n in list(p)[3:]] == ["explicit", False, None, 40.0, 0.01,
                                                   "constant", 10, False, 0]
    assert list(inspect.signature(foldin.explain_arrays).parameters) == list(p)
    for f, first in ((foldin.explain_users, "V"), (foldin.explain_items, "U")):
        q = inspect.signature(f).parameters
        assert list(q) == [first, "lists", "targets", "reg", "reg_mode", "top", "full", "device"]
        assert (q["top"].default, q["full"].default) == (10, False)
    for f in (implicit.ImplicitModel.explain, implicit.ImplicitModel.explain_items):
        q = inspect.signature(f).parameters
        assert list(q) == ["self", "lists", "targets", "top", "full"]
        assert (q["top"].default, q["full"].default) == (10, False)
    q = inspect.signature(MovieTable.explain_ridge).parameters
    assert list(q) == ["self", "rating_lists", "movie_ids_per_user", "reg", "reg_mode",
                       "subtract_median", "top"]
    assert (q["reg_mode"].default, q["subtract_median"].default, q["top"].default) == \
        ("weighted", True, 10)
    assert set(foldin.Explanation.__slots__) == {"x", "status", "score", "top", "phi"}


def test_c_abi_refuses_without_a_device():
    """Every precondition is checked on the host before the device is
    touched; a refused call writes no output and the library stays usable."""
    from movie_recommender_amd import _lib
    L = _lib.lib()
    ip, dp, llp = _lib.IP, _lib.DP, _lib.LLP
    T = np.ones((4, 3))
    roff = np.zeros(4)
    x = np.full((2, 4), -7.0)
    st = np.full(2, -7, np.int32)
    sc, phi, tv = np.full(8, -7.0), np.full(8, -7.0), np.full(64, -7.0)
    tp, tc = np.full(64, -7, np.int32), np.full(8, -7, np.int32)

    def ptr(a, t):
        return None if a is None else a.ctypes.data_as(t)

    def call(k=3, mode=0, intercept=0, alpha=8.0, reg=0.5, reg_mode=0, off=(0, 1), idx=(0,),
             r=(1.0,), table=T, row_offset=None, toff=(0, 2), tidx=(1, 2), top=2, poff=(0, 2),
             want_phi=True, want_top=True):
        off, toff, poff = (np.asarray(a, np.int64) for a in (off, toff, poff))
        idx, tidx = np.asarray(idx, np.int32), np.asarray(tidx, np.int32)
        r = np.asarray(r, np.float64)
        return L.mr_explain(0, k, 4, ptr(table, dp), ptr(row_offset, dp), mode, intercept, alpha,
                            reg, reg_mode, len(off) - 1, ptr(off, llp), ptr(idx, ip), ptr(r, dp),
                            ptr(toff, llp), ptr(tidx, ip), top, ptr(x, dp), ptr(st, ip),
                            ptr(sc, dp), ptr(poff, llp), ptr(phi, dp) if want_phi else None,
                            ptr(tp, ip) if want_top else None, ptr(tv, dp) if want_top else None,
                            ptr(tc, ip) if want_top else None)
    nan_t, nan_off = T.copy(), roff.copy()
    nan_t[1, 2] = np.nan
    nan_off[2] = np.inf
    for kw, word in [(dict(k=0), "1..128"), (dict(k=129), "1..128"),
                     (dict(mode=1, intercept=1), "implicit"),
                     (dict(mode=1, row_offset=roff), "implicit"),
                     (dict(mode=2), "mode"), (dict(reg_mode=2), "mode"),
                     (dict(alpha=-1.0), "alpha"), (dict(alpha=float("nan")), "alpha"),
                     (dict(reg=-0.5), "reg"), (dict(reg=float("inf")), "reg"),
                     (dict(idx=(4,)), "out of range"), (dict(idx=(-1,)), "out of range"),
                     (dict(r=(float("nan"),)), "r must be"),
                     (dict(mode=1, r=(-1.0,)), "r must be"),
                     (dict(table=nan_t), "T must be finite"),
                     (dict(row_offset=nan_off), "row_offset"),
                     (dict(off=(0, 2, 1), idx=(0, 1), r=(1.0, 1.0), toff=(0, 1, 2),
                           poff=(0, 2, 1)), "offsets"),
                     (dict(off=(1, 1)), "offsets"),
                     (dict(top=-1), "top"), (dict(top=65), "top"),
                     (dict(tidx=(1, 4)), "target id"), (dict(tidx=(-1, 2)), "target id"),
                     (dict(toff=(1, 2)), "target offsets"),
                     (dict(off=(0, 1, 1), toff=(0, 2, 1), poff=(0, 2, 2)), "target offsets"),
                     (dict(poff=(0, 3)), "running sum"), (dict(poff=(1, 3)), "running sum"),
                     (dict(off=(0, 1, 1), toff=(0, 1, 2), poff=(0, 1, 2)), "running sum"),
                     (dict(want_phi=False, want_top=False), "requested")]:
        assert call(**kw) == -1, kw
        assert word in _lib.last_error(), (kw, _lib.last_error())
    # one entity whose phi block is over 256 MiB
    n = 6000
    assert call(off=(0, n), idx=np.zeros(n, np.int32), r=np.ones(n), toff=(0, n),
                tidx=np.zeros(n, np.int32), poff=(0, n * n)) == -1
    assert "256 MiB" in _lib.last_error()
    for a in (x, sc, phi, tv):
        assert np.all(a == -7.0)                                          # nothing was written
    for a in (st, tp, tc):
        assert np.all(a == -7)
    assert call(off=(0,), toff=(0,), poff=(0,)) == 0                      # no entities: a no-op
    assert np.all(x == -7.0) and np.all(tc == -7)
    assert call(k=0, off=(0,), toff=(0,), poff=(0,)) == -1                # still validated


@pytest.mark.parametrize("form", ["explicit_icpt", "explicit", "implicit"])
def test_restatement_is_consistent(form):
    """The NumPy restatement: the contributions of a target sum to its score,
    x* solves G x = A^T coef, and the top rule is the stable descending sort
    (-0.0 ties with +0.0 and the smaller position wins)."""
    import explain_cases as C
    T, offs, lists, targets = C.case(20, False)
    for lst, tg in zip(lists, targets):
        if not lst or not tg:
            continue
        ref = C.reference(T, offs, lst, tg, form, 0.05, "weighted")
        G, A, coef = C.system(T, offs, lst, form, 0.05, "weighted")
        assert ref["phi"].shape == (len(tg), len(lst)) and ref["cond"] <= C.COND_MAX
        assert np.allclose(G @ ref["x"], A.T @ coef, rtol=0, atol=1e-9)
        assert np.all(np.abs(ref["phi"].sum(axis=1) - ref["score"])
                      <= ref["phi_bound"].sum(axis=1) + ref["score_bound"])
    pos, val = C.top_of([1.0, -0.0, 3.0, 0.0, 3.0, -2.0], 4)
    assert pos.tolist() == [2, 4, 0, 1] and np.signbit(val[3])
    assert C.top_of([0.5], 3)[0].tolist() == [0]
