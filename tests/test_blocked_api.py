"""CPU: the public face of the blocked exact solve (MR_OPT_SOLVE_BLOCKED) --
the option table, mr_solve_plan, and the NumPy restatement of the tiled
factorisation that the GPU tests and the design section describe."""
import ctypes

import numpy as np
import pytest

import blocked_cases as bc

KS = [1, 15, 16, 17, 65, 129, 513]


@pytest.mark.parametrize("K", KS)
def test_restatement_solves_spd_systems(K):
    """Against numpy.linalg.solve to 1e-12 relative.  A = M M^T / K + I has
    cond <= about 5 (M standard normal, K x K), so both solutions carry a few
    hundred ulps at K = 513."""
    rng = np.random.default_rng(K)
    M = rng.normal(0, 1, (K, K))
    A = M @ M.T / K + np.eye(K)
    b = rng.normal(0, 1, K)
    assert np.linalg.cond(A) <= 10.0
    x = bc.blocked_solve(A, b)
    xs = np.linalg.solve(A, b)
    err = np.max(np.abs(x - xs)) / np.max(np.abs(xs))
    print(f"K={K}: relative error {err:.3e}")
    assert err <= 1e-12


def test_restatement_reports_a_non_positive_pivot():
    assert bc.blocked_solve(np.zeros((5, 5)), np.ones(5)) is None
    A = np.eye(20)
    A[17, 17] = -1.0
    assert bc.blocked_solve(A, np.ones(20)) is None


def _plan(k, user_side):
    from movie_recommender_amd import _lib
    out = (ctypes.c_longlong * 3)(-7, -7, -7)
    rc = _lib.lib().mr_solve_plan(k, user_side, out)
    return rc, tuple(out)


@pytest.mark.parametrize("K", KS)
def test_solve_plan_matches_the_formula(K):
    T = -(-K // 16)
    want = (K, T * (T + 1) // 2, T * (T + 1) // 2 * 2048)
    if K > 1:            # K = k + 1 on the user side
        assert _plan(K - 1, 1) == (0, want)
        assert bc.plan(K - 1, True) == want
    if K <= 512:         # K = k on the item side
        assert _plan(K, 0) == (0, want)
        assert bc.plan(K, False) == want


def test_solve_plan_largest_slot():
    rc, (K, tiles, nbytes) = _plan(512, 1)
    assert (rc, K, tiles, nbytes) == (0, 513, 561, 561 * 2048)


@pytest.mark.parametrize("k", [0, -1, 513, 1 << 20])
def test_solve_plan_refuses_k_outside_1_to_512(k):
    for side in (0, 1):
        rc, out = _plan(k, side)
        assert rc == -1 and out == (-7, -7, -7)


def test_solve_plan_refuses_null():
    from movie_recommender_amd import _lib
    assert _lib.lib().mr_solve_plan(64, 1, None) == -1


def test_options_and_symbol():
    from movie_recommender_amd import _lib
    from movie_recommender_amd.engine import OPTIONS
    assert OPTIONS["solve_blocked"] == 9 and OPTIONS["solve_slots"] == 10
    assert sorted(OPTIONS.values()) == list(range(len(OPTIONS)))
    assert "mr_solve_plan" in _lib.SIGNATURES
    assert hasattr(_lib.lib(), "mr_solve_plan")
