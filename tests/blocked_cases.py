"""Shared by test_blocked_api.py and test_gpu_blocked_solve.py: the common
90-user x 70-item fixture (restated from test_gpu_regularized.fixture: 6,000
draws de-duplicated, zipf item ids, the last 2 users and the last item without
ratings, fp32-rounded uniform(-1, 1) factors) and an fp64 NumPy restatement of
the blocked solve of csrc/cholesky.hip: a left-looking Cholesky factorisation
by 16 x 16 tiles with the rhs as one more row, padding coordinates with a
unit diagonal, the diagonal tiles applied through their inverses, and the
back substitution over the tile columns in reverse."""
import functools

import numpy as np

NU, NI = 90, 70
TILE = 16


@functools.lru_cache(maxsize=None)
def fixture(k):
    rng = np.random.default_rng(100 + k)
    n = 6000
    u = rng.integers(0, NU - 2, n).astype(np.int32)       # last 2 users: no ratings
    i = (rng.zipf(1.3, n) % (NI - 1)).astype(np.int32)    # heavy items, last item empty
    key = np.unique(u.astype(np.int64) * NI + i)
    u = (key // NI).astype(np.int32)
    i = (key % NI).astype(np.int32)
    r = rng.normal(0, 1, len(u))
    U0 = rng.uniform(-1, 1, NU * (k + 1)).astype(np.float32).astype(np.float64)
    V0 = rng.uniform(-1, 1, NI * k).astype(np.float32).astype(np.float64)
    for a in (u, i, r, U0, V0):
        a.setflags(write=False)
    return u, i, r, U0, V0


def counts(u, i):
    return {"users": np.bincount(u, minlength=NU), "items": np.bincount(i, minlength=NI)}


def plan(k, user_side):
    """(K, tiles, bytes_per_slot) of mr_solve_plan, restated."""
    K = k + (1 if user_side else 0)
    T = -(-K // TILE)
    tiles = T * (T + 1) // 2
    return K, tiles, tiles * TILE * TILE * 8


def blocked_solve(A, b):
    """x with A x = b (A symmetric positive definite, K x K fp64), or None when
    a pivot is not positive.  Tile column j, left-looking:
      A_ij = A_ij - sum_{m<j} L_im L_jm^T  (i >= j, and the rhs as a last row),
      L_jj = chol(A_jj), W_j = L_jj^-1, L_ij = A_ij W_j^T, z_j = W_j (rhs row);
    then x_j = W_j^T (z_j - sum_{i>j} L_ij^T x_i) for j = T-1 ... 0."""
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    K = A.shape[0]
    T = -(-K // TILE)
    n = T * TILE
    P = np.eye(n)
    P[:K, :K] = A
    c = np.zeros(n)
    c[:K] = b
    L = np.zeros((n, n))
    W = np.zeros((T, TILE, TILE))
    z = np.zeros(n)
    sl = [slice(TILE * t, TILE * (t + 1)) for t in range(T)]
    for j in range(T):
        D = P[sl[j], sl[j]].copy()
        for m in range(j):
            D -= L[sl[j], sl[m]] @ L[sl[j], sl[m]].T
        Ljj = np.zeros((TILE, TILE))
        for q in range(TILE):            # the 16 x 16 factor, right-looking
            d = D[q, q]
            if not d > 0.0:
                return None
            Ljj[q:, q] = D[q:, q] / np.sqrt(d)
            D[q + 1:, q + 1:] -= np.outer(Ljj[q + 1:, q], Ljj[q + 1:, q])
        Wj = np.zeros((TILE, TILE))
        for r in range(TILE):            # row r of W: L^T y = e_r
            y = np.zeros(TILE)
            for q in range(TILE - 1, -1, -1):
                y[q] = ((1.0 if q == r else 0.0) - Ljj[q + 1:, q] @ y[q + 1:]) / Ljj[q, q]
            Wj[r] = y
        W[j] = Wj
        for i in range(j + 1, T):
            Aij = P[sl[i], sl[j]].copy()
            for m in range(j):
                Aij -= L[sl[i], sl[m]] @ L[sl[j], sl[m]].T
            L[sl[i], sl[j]] = Aij @ Wj.T
        rhs = c[sl[j]].copy()
        for m in range(j):
            rhs -= L[sl[j], sl[m]] @ z[sl[m]]
        z[sl[j]] = Wj @ rhs
    x = np.zeros(n)
    for j in range(T - 1, -1, -1):
        v = z[sl[j]].copy()
        for i in range(j + 1, T):
            v -= L[sl[i], sl[j]].T @ x[sl[i]]
        x[sl[j]] = W[j].T @ v
    assert np.all(x[K:] == 0.0)          # the padding solves to zero
    return x[:K]
