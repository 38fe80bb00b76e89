"""CPU: the non-negative solver's interface exists and fails cleanly without
a GPU, and the NumPy restatement the GPU tests compare against
(nnls_cases.nnls_bpp) is pinned to scipy.optimize.nnls."""
import ctypes
import os

import numpy as np
import pytest
import scipy.linalg
import scipy.optimize

import nnls_cases as nc


# ---------------------------------------------------------------------------
# the restatement against SciPy's active-set NNLS
# ---------------------------------------------------------------------------
def scipy_reference(G, c, k):
    """argmin 1/2 x^T G x - c^T x, x[:k] >= 0, a coordinate beyond k free: the
    free coordinate is eliminated by its Schur complement and SciPy solves
    min |L^T x - L^-1 c| with G = L L^T on the rest."""
    K = len(c)
    if K > k:
        g, gam = G[:k, k], G[k, k]
        Gr = G[:k, :k] - np.outer(g, g) / gam
        cr = c[:k] - g * c[k] / gam
    else:
        Gr, cr = G, c
    L = np.linalg.cholesky(Gr)
    x, _ = scipy.optimize.nnls(L.T, scipy.linalg.solve_triangular(L, cr, lower=True),
                               maxiter=30 * k)
    if K > k:
        x = np.append(x, (c[k] - g @ x) / gam)
    return x


@pytest.mark.parametrize("free_last", [False, True])
@pytest.mark.parametrize("K", [3, 17, 65, 129])
def test_restatement_matches_scipy(K, free_last):
    """200 random PD systems in all (25 per case), warm and cold starts."""
    rng = np.random.default_rng(1000 * K + free_last)
    k = K - 1 if free_last else K
    worst = 0.0
    for _ in range(25):
        A = rng.normal(size=(K + 8, K))
        G = A.T @ A / len(A) + 0.1 * np.eye(K)
        c = rng.normal(size=K)
        ref = scipy_reference(G, c, k)
        assert np.all(ref[:k] >= 0)
        for warm in (True, False):
            x, rounds = nc.nnls_bpp(G, c, k, rng.uniform(-1, 1, K), warm=warm)
            assert rounds > 0
            err = np.max(np.abs(x - ref)) / max(1.0, np.max(np.abs(ref)))
            worst = max(worst, err)
            assert np.all(x[:k] >= 0)
    print(f"K={K} free_last={free_last}: worst {worst:.2e}")
    assert worst <= 1e-10, worst


def test_restatement_rules():
    """Non-PD keeps max(previous, 0) and the free coordinate; the cap clamps."""
    prev = np.array([0.5, -0.25, 0.75])
    x, r = nc.nnls_bpp(np.zeros((3, 3)), np.zeros(3), 2, prev)
    assert r == 0 and np.array_equal(x, [0.5, 0.0, 0.75])
    x, r = nc.nnls_bpp(np.zeros((3, 3)), np.zeros(3), 2, prev, warm=False)
    assert r == 0 and np.array_equal(x, [0.5, 0.0, 0.75])
    G = np.array([[1.0, 2.0], [2.0, 1.0]])   # indefinite, positive diagonal
    x, r = nc.nnls_bpp(G, np.ones(2), 2, np.array([1.0, 1.0]))
    assert r == 0 and np.array_equal(x, [1.0, 1.0])
    G = np.array([[2.0, 1.0], [1.0, 2.0]])
    x, r = nc.nnls_bpp(G, np.array([1.0, -1.0]), 2, np.array([1.0, 1.0]), max_rounds=1)
    assert r == -1 and np.array_equal(x, [1.0, 0.0])   # solve gives (1, -1): clamped
    x, r = nc.nnls_bpp(G, np.array([1.0, -1.0]), 2, np.array([1.0, 1.0]))
    assert r == 2 and np.allclose(x, [0.5, 0.0]) and not np.signbit(x[1])


@pytest.mark.parametrize("mode", ["explicit", "implicit"])
@pytest.mark.parametrize("k", [20, 64])
def test_rounds_survive_another_summation_order(k, mode):
    """What test_gpu_nnls.py allows the GPU: the rounds of at least 95 % of the
    entities equal the restatement's.  The restatement against itself with the
    free set in descending order (every sum taken in another order) stays
    inside that cap on the fixtures' fp32-rounded normal equations."""
    u, i, r, U0, V0, nU, nI = nc.fixture(k)
    U = nc.zero_bias(U0, k) if mode == "implicit" else U0
    for side in ("users", "items"):
        G, c = nc.normal64(side, mode, u, i, r, U, V0, k, nU, nI)
        G = G.astype(np.float32).astype(np.float64)
        c = c.astype(np.float32).astype(np.float64)
        prev = nc.prev_of(side, U, V0, k, nU, nI)
        x1, r1 = nc.solve_side(G, c, k, prev)
        x2, r2 = nc.solve_side(G, c, k, prev, flip=True)
        assert np.mean(r1 == r2) >= 0.95, (side, np.mean(r1 == r2))
        assert np.max(np.abs(x1 - x2)) <= 1e-10 * max(1.0, np.max(np.abs(x1)))
        assert np.all(r1 >= 0) and r1.max() >= 2


# ---------------------------------------------------------------------------
# the interface
# ---------------------------------------------------------------------------
def test_solver_table_and_methods():
    from movie_recommender_amd.engine import SOLVERS, AlsContext
    assert SOLVERS == {"cg": 0, "cholesky": 1, "nnls": 2}
    for name in ("set_nnls", "nnls_stats", "nnls_rounds"):
        assert callable(getattr(AlsContext, name))


def test_header_declares_the_solver():
    from conftest import ROOT
    src = open(os.path.join(ROOT, "include", "mr_als.h")).read()
    assert "MR_SOLVER_NNLS = 2" in src
    assert "int mr_als_set_nnls(mr_als* ctx, int max_rounds, int warm_start);" in src
    assert "int mr_als_nnls_stats(mr_als* ctx, int side, long long out[4]);" in src
    assert "int mr_als_nnls_rounds(mr_als* ctx, int side, int* rounds);" in src


def test_symbols_exist_and_reject_null_context():
    from movie_recommender_amd import _lib
    L = _lib.lib()
    out = (ctypes.c_longlong * 4)()
    rounds = (ctypes.c_int * 4)()
    calls = {"mr_als_set_nnls": lambda: L.mr_als_set_nnls(None, 0, 1),
             "mr_als_nnls_stats": lambda: L.mr_als_nnls_stats(None, 0, out),
             "mr_als_nnls_rounds": lambda: L.mr_als_nnls_rounds(None, 0, rounds)}
    for name, call in calls.items():
        assert hasattr(L, name) and name in _lib.SIGNATURES
        # a message from this very call: set a different one first
        assert L.mr_set_gram_chunk(1) == -1 and "chunk" in _lib.last_error()
        assert call() == -1
        msg = _lib.last_error()
        assert msg and "chunk" not in msg and name in msg, msg
    assert L.mr_als_set_solver(None, 2, 0.0) == -1
    assert L.mr_set_gram_chunk(2048) == 0


def test_no_gpu_means_clean_error():
    """Without a device the NNLS context fails as every other one does."""
    from movie_recommender_amd import _lib
    from movie_recommender_amd.engine import AlsContext
    if _lib.lib().mr_device_count() > 0:
        return   # with a device: test_gpu_nnls.py
    u = np.zeros(4, np.int32)
    with pytest.raises(RuntimeError):
        AlsContext(u, u, np.ones(4), 2, 1, 1, solver="nnls")
