"""CPU: the helpers of tests/lsmr_cases.py and every input condition of the
GPU tests of the sparse LSMR, against SciPy itself."""
import math

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse import linalg

import cgls_cases as C
import lsmr_cases as M

SMALL = C.small_cases()


@pytest.fixture(scope="module")
def zoo():
    return C.zoo()


@pytest.mark.parametrize("case", SMALL + ["zoo"], ids=[c.name for c in SMALL] + ["zoo"])
def test_exact_setup_is_what_scipy_returns(case, zoo):
    case = zoo if isinstance(case, str) else case
    b, x0, e, m, S = M.exact_setup(case)
    A = M.csr_of(case)
    alpha = math.sqrt(S) / 2.0 ** m
    for bb, xx in ((b, x0), (e, None)):
        r = linalg.lsmr(A, bb, maxiter=0, x0=xx)
        assert np.array_equal(r[0], x0 if xx is not None else np.zeros(case.cols))
        assert (r[1], r[2]) == (0, 0)
        assert r[3] == 2.0 ** m
        assert r[4] == math.sqrt(S)
        assert r[5] == np.sqrt(alpha * alpha)
        assert r[6] == 1 and r[7] == 0


def test_zero_rhs_quirk_in_scipy():
    """b = 0 with x0 != 0: SciPy returns x = 0 with the setup's norms."""
    case = M.case_by_name("dup_unsorted_40x9")
    A = M.csr_of(case)
    assert case.x0.any() and (A @ case.x0).any()
    r = linalg.lsmr(A, np.zeros(case.rows), x0=case.x0)
    assert not r[0].any() and (r[1], r[2]) == (0, 0)
    u = -(A @ case.x0)
    beta = float(np.sqrt(np.sum(u * u)))     # integer data: exact sums
    g = A.T @ u
    assert r[3] == beta and r[6] == 1 and r[7] == 0
    assert abs(r[4] - math.sqrt(float(np.sum(g * g)))) <= 4e-16 * r[4]
    x, n, _ = M.lsmr_recurrence(A, np.zeros(case.rows), 0.0, case.x0, 5, np.float64)
    assert not x.any() and n["itn"] == 0
    # b = 0 with x0 = 0: the normar == 0 return
    r = linalg.lsmr(A, np.zeros(case.rows))
    assert not r[0].any() and r[1:] == (0, 0, 0, 0, 0, 1, 0)


def test_permutation_case_is_exact_in_scipy():
    rp, ci, vals, rows, cols, b = M.permutation_case()
    A = sp.csr_matrix((vals, ci, rp), shape=(rows, cols))
    for kw in (dict(), dict(atol=0, btol=0, conlim=0)):
        r = linalg.lsmr(A, b, **kw)
        assert (r[1], r[2]) == (1, 1) and np.array_equal(r[0], A.T @ b)
        assert r[3:] == (0, 0, 1, 1, 16)
        assert set(np.unique(r[0])) <= {-1.0, 0.0, 1.0}


def test_fp64_restatement_is_scipy():
    """lsmr_recurrence in fp64 with the tests on gives SciPy's stop and x."""
    case = M.case_by_name("full_block_256x8")
    A = M.csr_of(case)
    b, x0 = M.L.gaussian_rhs(case, 5)
    for kw in (dict(), dict(damp=0.5), dict(conlim=1.3), dict(x0=x0, damp=0.25)):
        ref = linalg.lsmr(A, b, **kw)
        x, n, _ = M.lsmr_recurrence(A, b, kw.get("damp", 0.0), kw.get("x0"), min(A.shape),
                                    np.float64, atol=1e-6, btol=1e-6,
                                    conlim=kw.get("conlim", 1e8), stop=True)
        assert (n["istop"], n["itn"]) == (ref[1], ref[2])
        assert M.rel_max(x, ref[0]) <= 1e-12
        assert M.norm_error(n, M.norms_of(ref)) <= 1e-12


@pytest.mark.parametrize("name,maxiter,variant", M.FIXED_CASES,
                         ids=[f"{n}-it{i}-v{v}" for n, i, v in M.FIXED_CASES])
def test_fixed_iteration_conditions(name, maxiter, variant):
    """SciPy returns (7, maxiter) in three row orders (asserted inside) and
    the bound stays in the range the reference's own error gives."""
    ref, bound, xerrs, nerrs = M.fixed_reference(name, maxiter, variant)
    print(f"{name} it={maxiter} v{variant}: scipy x errors {xerrs} norm errors {nerrs} "
          f"bound {bound:.3e}")
    assert 1e-13 <= bound <= 1e-11


@pytest.mark.parametrize("name,setting", M.STOP_CASES, ids=[f"{n}-{s}" for n, s in M.STOP_CASES])
def test_stop_cases_are_admitted(name, setting):
    b, kw, ref, margins = M.stop_reference(name, setting)
    print(f"{name} {setting}: scipy {(ref[1], ref[2])} margins {margins}")
    assert (ref[1], ref[2]) == M.STOP_EXPECTED[(name, setting)]
    assert margins[0] * 1.001 <= 1.0
    assert margins[1] is None or margins[1] >= 1.001
    assert M.stop_bound(name, setting) >= 1e-13


def test_als_reference_lsmr_is_scipys_lsmr_chained():
    from movie_recommender_amd import synth
    uid, iid, r = (np.asarray(a) for a in synth.dense_fixture(40, 45, 3)[:3])
    uid, iid = uid.astype(np.int64), iid.astype(np.int64)
    movies0 = np.random.default_rng(3).uniform(-1, 1, 45 * 3)
    run = M.als_reference_lsmr(uid, iid, r, 3, 40, 45, movies0, 2)
    users = linalg.lsmr(M.design_users(movies0, uid, iid, 40, 3), r, maxiter=100)[0]
    assert np.array_equal(users, run[0]["users"])
    Am = M.design_movies(users, uid, iid, 45, 3)
    movies = linalg.lsmr(Am, r - users[3::4][uid], maxiter=100)[0]
    assert np.array_equal(movies, run[0]["movies"])
    assert len(run) == 2 and run[1]["error"] < run[0]["error"]
