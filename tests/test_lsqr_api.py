"""CPU: the Python surface of the sparse LSQR (``movie_recommender_amd.lsqr``)
-- argument checks, SciPy's 10-tuple and the ``iter_lim=None`` rule -- with
the device context replaced by a recorder."""
import numpy as np
import pytest
import scipy.sparse as sp

from movie_recommender_amd import lsqr as M


class Recorder:
    calls = []

    def __init__(self, A, device=0):
        rp, ci, vals, self.rows, self.cols = M._csr_arrays(A)
        self.nnz = len(ci)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def solve(self, b, **kw):
        Recorder.calls.append(kw)
        return np.arange(self.cols, dtype=np.float64), dict(
            istop=2, itn=5, r1norm=1.5, r2norm=2.5, anorm=3.5, acond=4.5, arnorm=5.5, xnorm=6.5)


@pytest.fixture()
def recorder(monkeypatch):
    Recorder.calls = []
    monkeypatch.setattr(M, "LsqrContext", Recorder)
    return Recorder


A = sp.random(30, 7, density=0.3, random_state=1, format="csr")


def test_exports():
    assert set(M.__all__) == {"LsqrContext", "lsqr", "als_lsqr"}
    for name in ("solve", "set_values", "set_value_map", "set_values_from_table", "residual_l1",
                 "stats", "set_timing", "set_gather_path", "__enter__", "__exit__"):
        assert callable(getattr(M.LsqrContext, name))


def test_tuple_is_scipys(recorder):
    out = M.lsqr(A, np.ones(30), damp=0.5, x0=np.zeros(7))
    assert len(out) == 10
    x, istop, itn, r1norm, r2norm, anorm, acond, arnorm, xnorm, var = out
    assert np.array_equal(x, np.arange(7.0))
    assert (istop, itn, r1norm, r2norm, anorm, acond, arnorm, xnorm) == (2, 5, 1.5, 2.5, 3.5, 4.5,
                                                                        5.5, 6.5)
    assert var.shape == (7,) and not var.any()
    kw = recorder.calls[-1]
    assert kw["damp"] == 0.5 and kw["atol"] == 1e-6 and kw["btol"] == 1e-6 and kw["conlim"] == 1e8


def test_iter_lim_none_is_twice_the_columns(recorder):
    M.lsqr(A, np.ones(30))
    assert recorder.calls[-1]["iter_lim"] == 14
    M.lsqr(A, np.ones(30), iter_lim=3)
    assert recorder.calls[-1]["iter_lim"] == 3
    M.lsqr((A.indptr, A.indices, A.data, 9), np.ones(30))
    assert recorder.calls[-1]["iter_lim"] == 18


def test_show_and_calc_var_are_refused(recorder):
    with pytest.raises(ValueError):
        M.lsqr(A, np.ones(30), show=True)
    with pytest.raises(ValueError):
        M.lsqr(A, np.ones(30), calc_var=True)
    assert not recorder.calls


@pytest.mark.parametrize("bad", [
    (np.array([1, 2]), np.array([0, 0]), np.ones(2), 3),              # does not start at 0
    (np.array([0, 2, 1]), np.array([0, 0]), np.ones(2), 3),           # not monotone
    (np.array([0, 2]), np.array([0, 3]), np.ones(2), 3),              # column out of range
    (np.array([0, 2]), np.array([0, -1]), np.ones(2), 3),
    (np.array([0, 2]), np.array([0]), np.ones(2), 3),                 # short ids
    (np.array([0, 2]), np.array([0, 1]), np.ones(3), 3),              # long values
    (np.array([0, 2]), np.array([0, 1]), np.ones(2), -1),
    (np.array([0, 2]), np.array([0, 1]), np.ones(2)),                 # no column count
])
def test_matrix_checks_need_no_device(bad):
    with pytest.raises(ValueError):
        M.LsqrContext(bad)


def test_duplicates_and_unsorted_ids_are_legal():
    rp, ci, vals, rows, cols = M._csr_arrays((np.array([0, 4]), np.array([2, 0, 2, 2]),
                                              np.ones(4), 3))
    assert (rows, cols) == (1, 3) and list(ci) == [2, 0, 2, 2] and ci.dtype == np.int32


def test_vector_checks():
    with pytest.raises(ValueError):
        M._vec(np.ones(4), 5, "b")
    assert M._vec(np.ones((5, 1)), 5, "b").shape == (5,)


@pytest.mark.parametrize("kw", [dict(k=0), dict(num_users=0), dict(user_ids=[0, 9]),
                                dict(item_ids=[0, 5]), dict(ratings=[1.0]),
                                dict(movies0=np.ones(3))])
def test_als_argument_checks_need_no_device(kw):
    args = dict(user_ids=[0, 1], item_ids=[0, 1], ratings=[1.0, 2.0], k=2, num_users=2,
                num_items=2)
    args.update(kw)
    with pytest.raises(ValueError):
        M.als_lsqr(**args)
