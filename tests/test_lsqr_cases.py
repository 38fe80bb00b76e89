"""CPU: the helpers of tests/lsqr_cases.py and every input condition of the
GPU tests of the sparse LSQR, against SciPy itself."""
import math

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse import linalg

import cgls_cases as C
import lsqr_cases as L

SMALL = C.small_cases()


@pytest.fixture(scope="module")
def zoo():
    return C.zoo()


@pytest.mark.parametrize("case", SMALL + ["zoo"], ids=[c.name for c in SMALL] + ["zoo"])
def test_exact_setup_is_what_scipy_returns(case, zoo):
    case = zoo if isinstance(case, str) else case
    b, x0, e, m, S = L.exact_setup(case)
    assert int(np.sum(e != 0)) == 4 ** m and S < 2 ** 52
    A = L.csr_of(case)
    assert np.array_equal(b - A @ x0, e)
    for bb, xx in ((b, x0), (e, None)):
        r = linalg.lsqr(A, bb, iter_lim=0, x0=xx)
        assert np.array_equal(r[0], x0 if xx is not None else np.zeros(case.cols))
        assert (r[1], r[2]) == (0, 0)
        assert r[3] == r[4] == 2.0 ** m
        assert r[7] == math.sqrt(S)
        assert r[5] == r[6] == r[8] == 0


def test_permutation_case_is_exact_in_scipy():
    rp, ci, vals, rows, cols, b = L.permutation_case()
    assert (rows, cols) == (305, 307) and int(np.sum(b != 0)) == 256
    A = sp.csr_matrix((vals, ci, rp), shape=(rows, cols))
    r = linalg.lsqr(A, b)
    assert (r[1], r[2]) == (1, 1) and np.array_equal(r[0], A.T @ b)
    r = linalg.lsqr(A, 3 * b, atol=0, btol=0, conlim=0, iter_lim=5)
    assert (r[1], r[2]) == (1, 1) and np.array_equal(r[0], 3 * (A.T @ b))


def test_fp64_restatement_is_scipy():
    """lsqr_recurrence in fp64 with the tests on gives SciPy's stop and x."""
    case = L.case_by_name("full_block_256x8")
    A = L.csr_of(case)
    b, x0 = L.gaussian_rhs(case, 5)
    for kw in (dict(), dict(damp=0.5), dict(conlim=3.0)):
        ref = linalg.lsqr(A, b, **kw)
        x, n, _ = L.lsqr_recurrence(A, b, kw.get("damp", 0.0), None, 2 * case.cols, np.float64,
                                    atol=1e-6, btol=1e-6, conlim=kw.get("conlim", 1e8), stop=True)
        assert (n["istop"], n["itn"]) == (ref[1], ref[2])
        assert L.rel_max(x, ref[0]) <= 1e-12
        for key, val in zip(L.NORM_KEYS, ref[3:9]):
            assert abs(n[key] - val) <= 1e-12 * abs(val)


@pytest.mark.parametrize("name,iter_lim,variant", L.FIXED_CASES,
                         ids=[f"{n}-it{i}-v{v}" for n, i, v in L.FIXED_CASES])
def test_fixed_iteration_conditions(name, iter_lim, variant):
    """SciPy returns (7, iter_lim) in three row orders (asserted inside) and
    the bound stays in the range the reference's own error gives."""
    ref, bound, errs = L.fixed_reference(name, iter_lim, variant)
    print(f"{name} it={iter_lim} v{variant}: scipy errors {errs} bound {bound:.3e}")
    assert 1e-13 <= bound <= 1e-11


@pytest.mark.parametrize("name,setting", L.STOP_CASES, ids=[f"{n}-{s}" for n, s in L.STOP_CASES])
def test_stop_cases_are_admitted(name, setting):
    b, kw, ref, margins = L.stop_reference(name, setting)
    print(f"{name} {setting}: scipy {(ref[1], ref[2])} margins {margins}")
    assert margins[0] * 1.001 <= 1.0
    assert margins[1] is None or margins[1] >= 1.001
    assert L.stop_bound(name, setting) >= 1e-13


def test_als_reference_is_the_oracle_at_k3():
    from movie_recommender_amd import synth
    from oracle import scipy_als
    uid, iid, r = (np.asarray(a) for a in synth.dense_fixture(40, 45, 3)[:3])
    uid, iid = uid.astype(np.int64), iid.astype(np.int64)
    movies0 = np.random.default_rng(3).uniform(-1, 1, 45 * 3)
    run = L.als_reference(uid, iid, r, 3, 40, 45, movies0, 2)
    movies = movies0
    for it in run:
        users = scipy_als.solve_for_users(movies, uid, iid, r, 40, 3)
        movies = scipy_als.solve_for_movies(users, uid, iid, r, 45, 3)
        assert np.array_equal(users, it["users"]) and np.array_equal(movies, it["movies"])
