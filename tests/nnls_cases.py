"""Shared by the NNLS tests: an fp64 NumPy restatement of the solver's rule
(block principal pivoting with the backup rule and a free last coordinate),
the fixtures, and fp64 normal equations of both modes for CPU-only checks.

The rule (include/mr_als.h, DESIGN.md "Non-negative factors"): minimise
1/2 x^T G x - c^T x with x_j >= 0 on the first k coordinates; a coordinate
beyond k (the user bias) is free.  F starts as {j < k : previous x_j > 0}
(warm) or empty (cold).  A round solves G_FF x_F = c_F by Cholesky (the free
coordinate always in F), forms y = G x - c outside F, and collects V = {j in F
: x_j < 0} + {j not in F : y_j < 0}.  V empty: converged.  |V| < ninf: ninf =
|V|, p = 3, exchange all of V; else p >= 1: p -= 1, exchange all of V; else
exchange only max(V).  A diagonal entry <= 0 before the first round or a
pivot <= 0 in any round: the entity keeps max(previous x, 0) on the
constrained coordinates and its previous free coordinate (rounds 0).  At the
round cap the last x is clamped at 0 on the constrained coordinates
(rounds -cap).
"""
import functools

import numpy as np
import scipy.linalg

LAM = 0.05
ALPHA = 8.0
KS_SMALL = [5, 20, 40, 64]
K_LARGE = 128
SHAPES = {"small": (90, 70, 6000), "large": (48, 300, 9000)}


def default_cap(k):
    return 4 * (k + 1)


def nnls_bpp(G, c, k, x_prev, warm=True, ridge=0.0, max_rounds=0, flip=False):
    """(x, rounds) for one entity: G (K, K), c (K,), K = k or k + 1.  rounds
    as the engine reports them: r > 0 converged, -r stopped at the cap, 0 not
    positive definite.  ``flip`` runs the same rule with the free set's
    coordinates in descending order (another summation order)."""
    G = np.array(G, np.float64)
    c = np.asarray(c, np.float64)
    K = len(c)
    G[np.diag_indices(K)] += ridge
    cap = max_rounds if max_rounds > 0 else default_cap(k)
    x_prev = np.asarray(x_prev, np.float64)

    def keep_previous():
        x = x_prev.copy()
        x[:k] = np.maximum(x[:k], 0.0)
        return x, 0

    if not np.all(np.diag(G) > 0.0):
        return keep_previous()
    free = np.zeros(K, bool)
    free[k:] = True
    if warm:
        free[:k] = x_prev[:k] > 0.0
    ninf, p, rounds = K + 1, 3, 0
    while True:
        F = np.flatnonzero(free)
        if flip:
            F = F[::-1]
        val = np.zeros(K)
        if len(F):
            try:
                L = np.linalg.cholesky(G[np.ix_(F, F)])
            except np.linalg.LinAlgError:
                return keep_previous()
            z = scipy.linalg.solve_triangular(L, c[F], lower=True)
            val[F] = scipy.linalg.solve_triangular(L.T, z, lower=False)
        A = np.flatnonzero(~free)
        val[A] = G[np.ix_(A, F)] @ val[F] - c[A]
        rounds += 1
        V = np.flatnonzero(val[:k] < 0.0)
        if len(V) == 0:
            status = rounds
            break
        if rounds >= cap:
            status = -rounds
            break
        if len(V) < ninf:
            ninf, p = len(V), 3
        elif p >= 1:
            p -= 1
        else:
            V = V[-1:]
        free[V] = ~free[V]
    x = np.where(free, val, 0.0)
    x[:k] = np.maximum(x[:k], 0.0)
    return x, status


def solve_side(G, c, k, X_prev, **kw):
    """nnls_bpp over a stack of entities: (x[E, K], rounds[E])."""
    xs, rs = zip(*(nnls_bpp(G[e], c[e], k, X_prev[e], **kw) for e in range(len(c))))
    return np.stack(xs), np.array(rs, np.int32)


# ---------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture(k, shape="small"):
    """The recipe of test_gpu_implicit.py's fixture: zipf item ids (a few
    heavy items), the last 2 users and the last item empty, r in {0.5, ..., 5},
    fp32-rounded uniform(-1, 1) factors (U0 with a bias column: implicit runs
    zero it).  small: 90 x 70, 6,000 draws; large: 48 x 300, 9,000 draws."""
    nU, nI, n = SHAPES[shape]
    rng = np.random.default_rng(300 + k)
    u = rng.integers(0, nU - 2, n).astype(np.int32)
    i = (rng.zipf(1.3, n) % (nI - 1)).astype(np.int32)
    key = np.unique(u.astype(np.int64) * nI + i)
    u = (key // nI).astype(np.int32)
    i = (key % nI).astype(np.int32)
    r = rng.integers(1, 11, len(u)) * 0.5
    U0 = rng.uniform(-1, 1, nU * (k + 1)).astype(np.float32).astype(np.float64)
    V0 = rng.uniform(-1, 1, nI * k).astype(np.float32).astype(np.float64)
    for a in (u, i, r, U0, V0):
        a.setflags(write=False)
    return u, i, r, U0, V0, nU, nI


def shape_of(k):
    return "large" if k == K_LARGE else "small"


def zero_bias(U0, k):
    U = np.array(U0, np.float64).reshape(-1, k + 1)
    U[:, k] = 0.0
    return U.reshape(-1)


# ---------------------------------------------------------------------------
# fp64 normal equations of one side, as the engine defines them (CPU checks)
# ---------------------------------------------------------------------------
def normal64(side, mode, u, i, r, U, V, k, nU, nI, lam=LAM):
    """(G[E, K, K], c[E, K]): mode "explicit" (weighted lambda, user bias row /
    column last) or "implicit" (alpha = ALPHA, constant lambda, bias row e_k,
    rhs 0)."""
    Uf = np.asarray(U, np.float64).reshape(nU, k + 1)
    Vf = np.asarray(V, np.float64).reshape(nI, k)
    user = side == "users"
    K = k + 1 if user else k
    E = nU if user else nI
    G = np.zeros((E, K, K))
    c = np.zeros((E, K))
    ent, oth = (u, i) if user else (i, u)
    opp = Vf if user else Uf[:, :k]
    cnt = np.bincount(ent, minlength=E)
    if mode == "implicit":
        G[:, :k, :k] = opp.T @ opp
    for e, j, rv in zip(ent, oth, r):
        a = np.zeros(K)
        a[:k] = opp[j]
        if mode == "implicit":
            w = ALPHA * rv
            G[e] += w * np.outer(a, a)
            c[e] += (1.0 + w) * a
        else:
            if user:
                a[k] = 1.0
            G[e] += np.outer(a, a)
            c[e] += (rv if user else rv - Uf[j, k]) * a
    for e in range(E):
        G[e, np.arange(k), np.arange(k)] += lam * (cnt[e] if mode == "explicit" else 1.0)
    if mode == "implicit" and user:
        G[:, k, k] = 1.0
    return G, c


def prev_of(side, U, V, k, nU, nI):
    return (np.asarray(U, np.float64).reshape(nU, k + 1) if side == "users"
            else np.asarray(V, np.float64).reshape(nI, k))
