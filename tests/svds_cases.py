"""The truncated SVD's procedure restated in NumPy, the named test matrices
and the bounds that both the restatement and the device must meet.

``restate`` is ``mr_lsqr_svds`` (``csrc/svds.hip``, ``csrc/svds_host.h``) step
for step -- thick-restart Golub-Kahan-Lanczos, CGS2 against the whole basis,
the same convergence, restart and breakdown rules, the same splitmix64 stream
-- with ``numpy.linalg.svd`` for the projected matrix.  Two points where the
procedure is more specific than its one-line description:

* a breakdown is ``alpha`` or ``beta`` <= mn eps max(largest Ritz value seen,
  largest entry of B so far): before the first sweep ends no Ritz value is
  known, and every entry of B is a lower bound of sigma_1;
* a sweep with ncv == min(M, N) is the whole factorisation.  When the right
  basis is exhausted (j + 1 == N) beta is a recorded 0, so B's SVD is A's;
  for ncv == M < N the left basis spans everything and A = Q [B | beta e]
  P[:, :ncv + 1]^T exactly, so the SVD of that ncv x (ncv + 1) matrix is
  taken instead of B's and every pair counts as converged.

``admit`` asserts a case's relative gap (sigma_k - sigma_{k+1}) / sigma_1 >=
1e-4; every named case passes it (test_svds_api.py), none is dropped.
"""
import functools
import math

import numpy as np
import scipy.sparse as sp

EPS = float(np.finfo(np.float64).eps)
HALF_STARS = np.arange(1, 11) * 0.5
MIN_GAP = 1e-4
MASK = (1 << 64) - 1


class Rng:
    """splitmix64 mapped to (-1, 1), as ``SvdsRng``."""

    def __init__(self, seed):
        self.s = int(seed) & MASK

    def next(self):
        self.s = (self.s + 0x9E3779B97F4A7C15) & MASK
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
        z ^= z >> 31
        return (float(z >> 11) + 0.5) * (1.0 / 4503599627370496.0) - 1.0

    def fill(self, n):
        return np.array([self.next() for _ in range(n)], np.float64)


def default_ncv(k, mn):
    return min(mn, max(2 * k + 1, 20))


def cgs2(basis, w):
    """w orthogonalised against the columns of ``basis`` by classical
    Gram-Schmidt applied twice; returns (w, summed coefficients)."""
    h = np.zeros(basis.shape[1])
    for _ in range(2):
        c = basis.T @ w
        w = w - basis @ c
        h += c
    return w, h


def restate(A, k, ncv=None, tol=0.0, maxiter=None, v0=None, seed=0):
    A = sp.csr_matrix(A) if sp.issparse(A) else np.asarray(A, np.float64)
    M, N = A.shape
    mn = min(M, N)
    assert 1 <= k <= mn
    ncv = default_ncv(k, mn) if ncv is None else ncv
    assert k < ncv <= mn or ncv == k == mn
    maxiter = 10 * mn if maxiter is None else maxiter
    At = A.T.tocsr() if sp.issparse(A) else A.T
    rng = Rng(seed)
    P = np.zeros((N, ncv + 1))
    Q = np.zeros((M, ncv))
    B = np.zeros((ncv, ncv))
    p0 = np.asarray(v0, np.float64).copy() if v0 is not None else rng.fill(N)
    P[:, 0] = p0 / np.sqrt(np.sum(p0 * p0))
    sigma1 = bmax = beta_last = 0.0
    l = restarts = spmv = 0

    def replacement(basis, j, n):
        if j >= n:
            return np.zeros(n)
        while True:
            w, _ = cgs2(basis[:, :j], rng.fill(n))
            nrm = np.sqrt(np.sum(w * w))
            if nrm > 0:
                return w / nrm

    while True:
        for j in range(l, ncv):
            q, _ = cgs2(Q[:, :j], np.asarray(A @ P[:, j]).ravel())
            spmv += 1
            alpha = np.sqrt(np.sum(q * q))
            if alpha == 0.0 or alpha <= mn * EPS * max(sigma1, bmax):
                alpha = 0.0
                Q[:, j] = replacement(Q, j, M)
            else:
                Q[:, j] = q * (1.0 / alpha)
            B[j, j] = alpha
            bmax = max(bmax, alpha)
            z, _ = cgs2(P[:, :j + 1], np.asarray(At @ Q[:, j]).ravel())
            spmv += 1
            beta = np.sqrt(np.sum(z * z))
            if j + 1 >= N or beta == 0.0 or beta <= mn * EPS * max(sigma1, bmax):
                beta = 0.0
                P[:, j + 1] = replacement(P, j + 1, N)
            else:
                P[:, j + 1] = z * (1.0 / beta)
            if j + 1 < ncv:
                B[j, j + 1] = beta
            else:
                beta_last = beta
            bmax = max(bmax, beta)
        vcols = ncv
        if ncv == M and M < N and beta_last != 0.0:
            Baug = np.concatenate([B, np.zeros((ncv, 1))], axis=1)
            Baug[ncv - 1, ncv] = beta_last
            X, sig, Yt = np.linalg.svd(Baug, full_matrices=False)
            beta_last, vcols = 0.0, ncv + 1
        else:
            X, sig, Yt = np.linalg.svd(B)
        Y = Yt.T
        sigma1 = max(sigma1, sig[0])
        thr = tol * sigma1 if tol > 0 else 8 * ncv * EPS * sigma1
        resid = np.abs(beta_last * X[ncv - 1, :])
        nconv = 0
        while nconv < ncv and resid[nconv] <= thr:
            nconv += 1
        if nconv >= k or ncv == mn or restarts >= maxiter:
            break
        keep = min(ncv - 1, max(k + nconv, k + (ncv - k) // 2))
        Pn = P[:, :ncv] @ Y[:, :keep]
        P[:, keep] = P[:, ncv]
        P[:, :keep] = Pn
        Q[:, :keep] = Q @ X[:, :keep]
        B[:] = 0.0
        B[np.arange(keep), np.arange(keep)] = sig[:keep]
        B[:keep, keep] = beta_last * X[ncv - 1, :keep]
        l = keep
        restarts += 1
    return dict(s=sig[:k].copy(), U=Q @ X[:, :k], Vt=(P[:, :vcols] @ Y[:, :k]).T,
                converged=nconv >= k, nconv=min(nconv, k), restarts=restarts, spmv=spmv,
                resid=resid[:k].copy(), thr=thr, ncv=ncv, anorm=sigma1)


# ---------------------------------------------------------------------------
# matrices
# ---------------------------------------------------------------------------
def random_sparse(m, n, density, seed):
    """m x n CSR with half-star values and no empty structure rules."""
    rng = np.random.default_rng(seed)
    mask = rng.random((m, n)) < density
    vals = rng.choice(HALF_STARS, size=(m, n))
    return sp.csr_matrix(np.where(mask, vals, 0.0))


def rank3_50x40():
    rng = np.random.default_rng(7)
    return sp.csr_matrix((rng.integers(-3, 4, (50, 3)) @ rng.integers(-3, 4, (3, 40)))
                         .astype(np.float64))


@functools.lru_cache(maxsize=None)
def matrix(name):
    import cgls_cases as C
    table = {"r90x70": (90, 70, 0.15, 1), "r70x90": (70, 90, 0.15, 2),
             "r257x65": (257, 65, 0.1, 3), "r64x257": (64, 257, 0.1, 4),
             "r300x200": (300, 200, 0.05, 5), "r1000x400": (1000, 400, 0.02, 6),
             "r33x5": (33, 5, 0.4, 7), "r40x30": (40, 30, 0.3, 8)}
    if name in table:
        return random_sparse(*table[name])
    for c in C.small_cases():
        if c.name == name:
            return sp.csr_matrix((c.vals, c.ci, c.rp), shape=(c.rows, c.cols))
    raise KeyError(name)


# (matrix, k, ncv): ncv in {k + 1, 2k + 1, mn} -- many restarts, the default
# rule, no restart; k = mn - 1 and k = mn at 40 x 30
NAMED = [
    ("r90x70", 5, 6), ("r90x70", 5, 11), ("r90x70", 5, 70),
    ("r70x90", 3, 4), ("r70x90", 3, 7), ("r70x90", 3, 70),
    ("r257x65", 1, 2), ("r257x65", 16, 33),
    ("r64x257", 8, 17), ("r64x257", 8, 64),
    ("r300x200", 10, 11), ("r300x200", 29, 59),
    ("r1000x400", 10, 21), ("r1000x400", 6, None),
    ("r33x5", 2, 3), ("r33x5", 2, 5), ("r33x5", 4, 5), ("r33x5", 5, 5),
    ("r40x30", 29, 30), ("r40x30", 30, 30),
    ("dup_unsorted_40x9", 3, 7), ("dense_col_2500x6", 2, 5), ("one_by_one", 1, 1),
    ("full_block_256x8", 4, 9),
]


def case_id(case):
    name, k, ncv = case
    return f"{name}-k{k}-ncv{ncv}"


@functools.lru_cache(maxsize=None)
def dense_svd(name):
    """(U, s, Vt) of the named matrix by numpy.linalg.svd, computed once."""
    return np.linalg.svd(matrix(name).toarray(), full_matrices=False)


@functools.lru_cache(maxsize=None)
def reference(case):
    """The restatement's result on a named case, computed once and shared."""
    name, k, ncv = case
    return restate(matrix(name), k, ncv)


def gap_of(s_all, k):
    nxt = s_all[k] if k < len(s_all) else 0.0
    return (s_all[k - 1] - nxt) / s_all[0]


def admit(case):
    name, k, _ = case
    gap = gap_of(dense_svd(name)[1], k)
    assert gap >= MIN_GAP, f"{case_id(case)}: relative gap {gap:.3g} below {MIN_GAP}"
    return gap


# ---------------------------------------------------------------------------
# the bounds
# ---------------------------------------------------------------------------
# residual and orthonormality allowance over max(thr, the restatement's own
# figure): covers the device reductions' different summation order; not
# derived.  Worst measured ratio of the device's true residual to max(thr,
# the restatement's): 1.39 (r300x200, k = 10, ncv = 11, 502 restarts); 1.18
# next; below 1.0 wherever ncv >= 2k + 1 ("Truncated SVD").
RESID_FACTOR = 4.0


def true_residuals(A, U, s, Vt):
    """max over the pairs of |A v - s u| and |A^T u - s v| (absolute)."""
    A = np.asarray(A.toarray() if sp.issparse(A) else A)
    r1 = np.sqrt(np.sum((A @ Vt.T - U * s[None, :]) ** 2, axis=0))
    r2 = np.sqrt(np.sum((A.T @ U - Vt.T * s[None, :]) ** 2, axis=0))
    return np.maximum(r1, r2)


def ortho_defect(U, Vt):
    k = U.shape[1]
    return max(np.max(np.abs(U.T @ U - np.eye(k))), np.max(np.abs(Vt @ Vt.T - np.eye(k))))


def check_triplets(A, k, ncv, thr, U, s, Vt, svd, ref=None, subspace=True, log=None):
    """The four bounds on descending (U, s, Vt) against ``svd`` = numpy's
    (U, s, Vt) of A.  ``ref``: the restatement's result, whose own residual and
    orthonormality widen bounds 2 and 3 (the device's rule); None for the
    restatement itself.  Returns the measured figures."""
    M, N = A.shape
    _, s_np, Vt_np = svd
    sigma1 = s_np[0] if len(s_np) else 0.0
    res = true_residuals(A, U, s, Vt)
    fig = {"value_err": float(np.max(np.abs(s - s_np[:k]))), "residual": float(res.max()),
           "ortho": float(ortho_defect(U, Vt)), "thr": float(thr)}
    res_lim = RESID_FACTOR * thr
    orth_lim = 64 * EPS * math.sqrt(ncv)
    if ref is not None:
        ref_res = float(true_residuals(A, ref["U"], ref["s"], ref["Vt"]).max())
        res_lim = max(res_lim, RESID_FACTOR * ref_res)
        orth_lim = max(orth_lim, RESID_FACTOR * float(ortho_defect(ref["U"], ref["Vt"])))
        fig["ref_residual"] = ref_res
    fig["residual_over_limit"] = fig["residual"] / res_lim if res_lim > 0 else 0.0
    if log is not None:
        log(fig)
    # 1. Ritz values of the augmented symmetric matrix, plus numpy's own rounding
    assert fig["value_err"] <= math.sqrt(2) * fig["residual"] + 4 * math.sqrt(M + N) * EPS * sigma1, fig
    # 2. residuals
    assert fig["residual"] <= res_lim, fig
    # 3. orthonormality
    assert fig["ortho"] <= orth_lim, fig
    # 4. subspace (Wedin): sin(theta) <= 4 residual / gap
    if subspace and sigma1 > 0:
        gap = gap_of(s_np, k) * sigma1
        Vk = Vt_np[:k].T
        sin_t = float(np.linalg.norm(Vt.T - Vk @ (Vk.T @ Vt.T), 2))
        fig["sin_theta"] = sin_t
        assert sin_t <= 4 * fig["residual"] / gap, fig
    return fig
