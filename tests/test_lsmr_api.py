"""CPU: the Python surface of the sparse LSMR (``movie_recommender_amd.lsmr``,
``LsqrContext.solve_lsmr``) -- SciPy's 8-tuple, the ``maxiter=None`` rule,
``als_lsmr``'s argument checks and its ``maxiter=iter_lim`` -- with the device
context replaced by a recorder; and the C ABI's additions in the header, the
binding and the built library."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from movie_recommender_amd import _lib
from movie_recommender_amd import lsqr as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Recorder:
    calls = []

    def __init__(self, A, device=0):
        rp, ci, vals, self.rows, self.cols = Q._csr_arrays(A)
        self.nnz = len(ci)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def set_value_map(self, index):
        pass

    def set_values_from_table(self, table):
        pass

    def residual_l1(self, b, x):
        return 1.0

    def solve(self, b, **kw):
        raise AssertionError("als_lsmr / lsmr must not call the LSQR solve")

    def solve_lsmr(self, b, **kw):
        Recorder.calls.append(kw)
        return np.arange(self.cols, dtype=np.float64), dict(
            istop=2, itn=5, normr=1.5, normar=2.5, norma=3.5, conda=4.5, normx=5.5)


@pytest.fixture()
def recorder(monkeypatch):
    Recorder.calls = []
    monkeypatch.setattr(Q, "LsqrContext", Recorder)
    return Recorder


A = sp.random(30, 7, density=0.3, random_state=1, format="csr")


def test_exports():
    from movie_recommender_amd import lsmr as M
    assert M.__all__ == ["lsmr", "als_lsmr"]
    assert set(Q.__all__) == {"LsqrContext", "lsqr", "als_lsqr"}     # unchanged
    assert callable(Q.LsqrContext.solve_lsmr)


def test_tuple_is_scipys(recorder):
    from movie_recommender_amd import lsmr as M
    out = M.lsmr(A, np.ones(30), damp=0.5, x0=np.zeros(7))
    assert len(out) == 8
    x, istop, itn, normr, normar, norma, conda, normx = out
    assert np.array_equal(x, np.arange(7.0))
    assert (istop, itn, normr, normar, norma, conda, normx) == (2, 5, 1.5, 2.5, 3.5, 4.5, 5.5)
    kw = recorder.calls[-1]
    assert kw["damp"] == 0.5 and kw["atol"] == 1e-6 and kw["btol"] == 1e-6 and kw["conlim"] == 1e8
    assert np.array_equal(kw["x0"], np.zeros(7))


def test_maxiter_none_is_the_smaller_dimension(recorder):
    from movie_recommender_amd import lsmr as M
    M.lsmr(A, np.ones(30))
    assert recorder.calls[-1]["maxiter"] == 7
    M.lsmr(A.T.tocsr(), np.ones(7))
    assert recorder.calls[-1]["maxiter"] == 7
    M.lsmr(A, np.ones(30), maxiter=3)
    assert recorder.calls[-1]["maxiter"] == 3
    M.lsmr((A.indptr, A.indices, A.data, 9), np.ones(30))
    assert recorder.calls[-1]["maxiter"] == 9
    M.lsmr((A.indptr, A.indices, A.data, 50), np.ones(30))
    assert recorder.calls[-1]["maxiter"] == 30


def test_show_is_refused(recorder):
    from movie_recommender_amd import lsmr as M
    with pytest.raises(ValueError):
        M.lsmr(A, np.ones(30), show=True)
    assert not recorder.calls


@pytest.mark.parametrize("kw", [dict(k=0), dict(num_users=0), dict(user_ids=[0, 9]),
                                dict(item_ids=[0, 5]), dict(ratings=[1.0]),
                                dict(movies0=np.ones(3))])
def test_als_argument_checks_need_no_device(kw):
    from movie_recommender_amd import lsmr as M
    args = dict(user_ids=[0, 1], item_ids=[0, 1], ratings=[1.0, 2.0], k=2, num_users=2,
                num_items=2)
    args.update(kw)
    with pytest.raises(ValueError):
        M.als_lsmr(**args)


def test_als_lsmr_solves_with_maxiter_iter_lim(recorder):
    from movie_recommender_amd import lsmr as M
    seen = []
    users, movies, iterations, errors = M.als_lsmr([0, 1, 1], [0, 1, 0], [1.0, 2.0, 3.0], 2, 2, 2,
                                                   seed=1, max_iterations=2, iter_lim=17,
                                                   callback=seen.append)
    # the recorder's error never improves: the 1 % rule ends the loop at 2
    assert iterations == 2 and errors == [1.0 / 3, 1.0 / 3] and len(seen) == 2
    assert recorder.calls == [dict(maxiter=17)] * 4
    assert users.shape == (2 * 3,) and movies.shape == (2 * 2,)
    assert seen[0]["user_solve"]["normar"] == 2.5


def test_als_lsqr_still_solves_with_iter_lim(monkeypatch):
    calls = []

    class LsqrRecorder(Recorder):
        def solve(self, b, **kw):
            calls.append(kw)
            return np.arange(self.cols, dtype=np.float64), {}

        def solve_lsmr(self, b, **kw):
            raise AssertionError("als_lsqr must not call the LSMR solve")

    monkeypatch.setattr(Q, "LsqrContext", LsqrRecorder)
    Q.als_lsqr([0, 1, 1], [0, 1, 0], [1.0, 2.0, 3.0], 2, 2, 2, seed=1, max_iterations=1,
               iter_lim=9)
    assert calls == [dict(iter_lim=9)] * 2


def test_c_abi_is_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "mr_lsqr.h")) as f:
        header = f.read()
    flat = re.sub(r"\s+", " ", header)
    assert ("typedef struct mr_lsmr_result { int istop, itn; double normr, normar, norma, conda, "
            "normx; } mr_lsmr_result;") in flat
    assert ("int mr_lsqr_solve_lsmr(mr_lsqr* ctx, const double* b, const double* x0_or_null, "
            "double damp, double atol, double btol, double conlim, int maxiter, double* x_out, "
            "mr_lsmr_result* out);") in flat
    assert [n for n, _ in _lib.MrLsmrResult._fields_] == ["istop", "itn", "normr", "normar",
                                                          "norma", "conda", "normx"]
    assert ctypes.sizeof(_lib.MrLsmrResult) == 2 * 4 + 5 * 8
    L = _lib.lib()
    fn = L.mr_lsqr_solve_lsmr
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 10
    assert fn.argtypes[-1] == ctypes.POINTER(_lib.MrLsmrResult)
