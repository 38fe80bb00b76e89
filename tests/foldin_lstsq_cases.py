"""Least-squares fold-in cases whose answer is known exactly, for
``MovieTable.fold_in`` (``fold_in_kernel`` / ``fold_in_svd_kernel``), which
stands in for ``numpy.linalg.lstsq([V_m, 1], ratings, rcond=None)``.

Construction.  Factor rows are dyadic rationals (small integers / 64), so
``A = [F, 1]``, a dyadic ``x0`` and ``b = A x0`` are all exact in fp64.  The
ratings are ``b + e`` with a residual ``e`` that is exactly orthogonal to
range(A): a movie listed m times gets residuals that sum to zero over its m
identical rows, hence ``A^T e = 0``.  (A movie listed twice is legal in the
reference: every listed rating becomes a row.)

* Full-rank A: ``x0`` is *the* least-squares solution.  Near-collinearity is
  exact as well: ``F[:, 1] = F[:, 0] + s * noise`` with ``s = m / 2^q``.
* Rank-deficient A: ``x0 = A^T w`` with a small dyadic ``w`` lies in the row
  space, so it is exactly the minimum-norm least-squares solution.

Every builder checks its own exactness in integer arithmetic on the scaled
data (``check_exact``): the fp64 arrays equal the integers they were made
from, ``A x0 == b - e`` and ``A^T e == 0``.

``reference(case)`` is what the tolerances are measured against, all from
NumPy on the CPU and none of it from the code under test: lstsq's answer, rank
and error against ``x0``, the kept singular values, and the pivot ratio of a
plain Cholesky of ``A^T A`` (the quantity the GPU compares with
``cond_limit``)."""
import functools
import os
import re

import numpy as np

EPS = 2.0 ** -52
# cond_limit of rec_fold_in (csrc/serving.hip): a user whose Cholesky pivot
# ratio min(d) / max(d) is below it goes to the Jacobi SVD.
# test_serving_foldin_cases.py checks this against the source.
COND_LIMIT = 1e-6
# what mr_serving.h / DESIGN.md promise of the Cholesky path against lstsq
CHOLESKY_TOL = 1e-8
SIZES = (1, 3, 11, 15, 16, 63, 64, 100, 128)
LADDER_SHAPES = ((11, 40), (100, 301))
LONG_M = 3000                      # one long list at k = 11 and at k = 128


def source_cond_limit():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                        "movie_recommender_amd", "csrc", "serving.hip")
    with open(path) as f:
        m = re.findall(r"const double cond_limit = ([0-9.eE+-]+);", f.read())
    assert len(m) == 1, m
    return float(m[0])


class Case:
    """One rating list.  ``F_int / 2^ea`` are the table rows (n x k), ``rows``
    the table row of each list entry, ``x0_int / 2^ex`` the answer and
    ``r_int / 2^(ea + ex)`` the ratings; ``e_int`` is the residual on the
    ratings' scale.  The float arrays are what the GPU and lstsq see."""

    def __init__(self, name, k, kind, rank, F_int, ea, rows, x0_int, ex, e_int):
        self.name, self.k, self.K, self.kind, self.rank = name, k, k + 1, kind, rank
        self.F_int, self.ea, self.rows = F_int, ea, np.asarray(rows, np.int64)
        self.x0_int, self.ex, self.e_int = x0_int, ex, e_int
        self.M = len(self.rows)
        A_int = self.A_int()
        self.r_int = A_int.dot(x0_int) + e_int
        self.F = np.ldexp(F_int.astype(np.float64), -ea)
        self.x0 = np.ldexp(x0_int.astype(np.float64), -ex)
        self.ratings = np.ldexp(self.r_int.astype(np.float64), -(ea + ex))
        self.check_exact()

    def A_int(self):
        """The list's M x K matrix as Python integers, scale 2^ea."""
        one = np.full((self.M, 1), 1 << self.ea, dtype=object)
        return np.concatenate([self.F_int[self.rows], one], axis=1)

    def A(self):
        return np.c_[self.F[self.rows], np.ones(self.M)]

    def check_exact(self):
        lim = 1 << 53
        for v_int, v, sc in ((self.F_int, self.F, self.ea), (self.x0_int, self.x0, self.ex),
                             (self.r_int, self.ratings, self.ea + self.ex)):
            assert all(abs(int(x)) < lim for x in v_int.ravel()), self.name
            back = np.ldexp(v, sc)
            assert np.all(back == np.floor(back)), self.name
            assert [int(x) for x in back.ravel()] == [int(x) for x in v_int.ravel()], self.name
        A_int = self.A_int()
        assert np.all(A_int.dot(self.x0_int) == self.r_int - self.e_int), self.name
        assert np.all(A_int.T.dot(self.e_int) == 0), self.name
        assert self.M >= self.K and self.rows.max() < len(self.F_int), self.name
        assert np.any(self.e_int != 0) or self.M == len(set(self.rows.tolist())), self.name


def _obj(a):
    return np.asarray(a, dtype=np.int64).astype(object)


def _rows(rs, n, k):
    """n table rows, scale 64: noise in [-16, 16] / 64 plus 1.0 in column
    i mod (k + 1) (none when that is k): any K of them and the ones column are
    well conditioned, also when M = K."""
    F = rs.randint(-16, 17, (n, k)).astype(np.int64)
    for i in range(n):
        if i % (k + 1) < k:
            F[i, i % (k + 1)] += 64
    return F


def _listing(rs, n, M):
    """M list entries over n table rows, every row at least once, shuffled;
    the extra entries are repeats."""
    rows = np.concatenate([np.arange(n), rs.randint(0, n, M - n)]).astype(np.int64)
    return rs.permutation(rows)


def _residual(rs, rows, scale_bits):
    """Residual with A^T e = 0: over the m entries of one table row,
    d * (2 j - (m - 1)), j = 0 .. m-1, with d in {1/2, 1, 3/2}; scale
    2^scale_bits (>= 1)."""
    e = np.zeros(len(rows), dtype=object)
    for row in np.unique(rows):
        at = np.flatnonzero(rows == row)
        m = len(at)
        if m > 1:
            d = int(rs.randint(1, 4)) << (scale_bits - 1)
            for j, i in enumerate(at):
                e[i] = d * (2 * j - (m - 1))
    return e


def _n_rows(k, M):
    """Table rows for a full-rank list of M: all distinct at M = K, one repeat
    at K + 1, a quarter repeats on longer lists."""
    K = k + 1
    return M - min(M - K, max(1, M // 4)) if M > K else M


def full_rank_case(k, M, seed, s=None):
    """Full column rank.  ``s = (m, q)``: column 1 = column 0 + m / 2^q * noise
    (k >= 2), with integer x0 so that the ratings stay within 53 bits."""
    rs = np.random.RandomState(seed)
    n = _n_rows(k, M)
    F = _obj(_rows(rs, n, k))
    ea = 6
    if s is None:
        x0, ex = _obj(rs.randint(-16, 17, k + 1)), 3
        name = f"full k{k} M{M}"
    else:
        m, q = s
        noise = _obj(rs.randint(-16, 17, n))
        noise[noise == 0] = 1
        F = F * (1 << q)
        F[:, 1] = F[:, 0] + m * noise
        ea += q
        x0, ex = _obj(rs.randint(-3, 4, k + 1)), 0
        name = f"ladder k{k} M{M} s={m}/2^{q}"
    rows = _listing(rs, n, M)
    e = _residual(rs, rows, ea + ex)
    return Case(name, k, "full", k + 1, F, ea, rows, x0, ex, e)


def deficient_case(k, M, kind, seed):
    """Rank-deficient lists.  kind:
    a  fewer distinct rows than K (K - 1 of them, repeats fill the list)
    b  a constant factor column (collinear with the intercept)
    c  two equal columns and an all-zero column: deficit 2 (k >= 3)
    d  deficit 3 (k >= 3): an equal pair, a column that is the sum of two
       others and a constant column; at k < 6 three constant columns"""
    rs = np.random.RandomState(seed)
    K = k + 1
    if kind == "a":
        n, rank = K - 1, K - 1
    else:
        n = _n_rows(k, M)
        rank = K - {"b": 1, "c": 2, "d": 3}[kind]
    F = _rows(rs, n, k)
    if kind == "b":
        F[:, k // 2] = 32
    elif kind == "c":
        z = (1, k - 1)[seed % 2]             # the zero column: early or last
        F[:, 2 if z == 1 else 1] = F[:, 0]
        F[:, z] = 0
    elif kind == "d":
        if k >= 6:
            F[:, 1] = F[:, 0]
            F[:, 3] = F[:, 2] + F[:, 4]
            F[:, 5] = -48
        else:
            F[:, 0], F[:, 1], F[:, 2] = 32, 16, -48
    F = _obj(F)
    rows = _listing(rs, n, M)
    ea, ew = 6, 2
    # x0 = A^T w, w nonzero on a few list entries
    w = np.zeros(M, dtype=object)
    for i in rs.choice(M, min(M, 6), replace=False):
        w[i] = int(rs.randint(-4, 5))
    if not np.any(w != 0):
        w[0] = 3
    A_int = np.concatenate([F[rows], np.full((M, 1), 1 << ea, dtype=object)], axis=1)
    x0, ex = A_int.T.dot(w), ea + ew
    e = _residual(rs, rows, ea + ex)
    tag = f"def-c{z}" if kind == "c" else f"def-{kind}"
    return Case(f"{tag} k{k} M{M}", k, kind, rank, F, ea, rows, x0, ex, e)


# ---------------------------------------------------------------------------
# the reference side
# ---------------------------------------------------------------------------
def pivot_ratio(A):
    """min / max of the Cholesky pivots of A^T A (before the square root), by
    NumPy; 0.0 when the factorisation meets a non-positive pivot."""
    try:
        d = np.diag(np.linalg.cholesky(A.T @ A)) ** 2
    except np.linalg.LinAlgError:
        return 0.0
    return float(d.min() / d.max())


def rel_err(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def reference(case):
    """lstsq on the case and the numbers the tolerances are made of (cached on
    the case)."""
    if getattr(case, "_ref", None) is None:
        A = case.A()
        x, _, rank, sv = np.linalg.lstsq(A, case.ratings, rcond=None)
        cut = EPS * max(case.M, case.K) * sv[0]
        kept = sv[sv > cut]
        ratio = pivot_ratio(A)
        e_ref = rel_err(x, case.x0)
        cond_eff = float(kept[0] / kept[-1])
        if case.rank < case.K or ratio < COND_LIMIT / 100:
            must = 2
        elif ratio > COND_LIMIT * 100:
            must = 1
        else:
            must = 0
        jac = 16 * max(e_ref, case.K * EPS * cond_eff)
        tol = {2: jac, 1: CHOLESKY_TOL, 0: max(CHOLESKY_TOL, jac)}[must]
        case._ref = dict(x=x, rank=int(rank), sv=sv, cut=cut, kept=kept, ratio=ratio,
                         e_ref=e_ref, cond_eff=cond_eff, must=must, jacobi_tol=jac, tol=tol)
    return case._ref


# ---------------------------------------------------------------------------
# the case lists
# ---------------------------------------------------------------------------
def list_lengths(k):
    K = k + 1
    return [K, K + 1] + [m for m in (32, 33, 64) if m > K + 1] + [301]


def _dyadic_s(s):
    """s rounded to m / 2^q with m in 4 .. 7."""
    q = 0
    while s * (1 << q) < 4:
        q += 1
    m = int(round(s * (1 << q)))
    return (m, q) if m <= 7 else (4, q - 1)


@functools.lru_cache(maxsize=None)
def ladder(k, M):
    """Full-rank conditioning ladder: the pivot ratio goes as s^2, measured
    once at s = 2^-8; the rungs aim at pivot ratios from 3e-2 (cond about 10)
    to 3e-19 (cond 5e9 .. 1e10; beyond, the smallest singular value would come
    within 1e3 of lstsq's cut-off at M = 301), four of them within a factor of
    5 of COND_LIMIT."""
    seed = 7000 + k
    c = pivot_ratio(full_rank_case(k, M, seed, (4, 10)).A()) * 2.0 ** 16
    targets = [None, COND_LIMIT * 3e3, 1e-3, COND_LIMIT * 300, COND_LIMIT * 4, COND_LIMIT * 2,
               COND_LIMIT / 2, COND_LIMIT / 4, COND_LIMIT / 300, COND_LIMIT * 1e-5, 1e-16, 3e-19]
    out = []
    for t in targets:
        s = (4, 2) if t is None else _dyadic_s(min(1.0, (t / c) ** 0.5))
        out.append(full_rank_case(k, M, seed, s))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def cases_for(k):
    """Every known-answer case of one k: full rank at each list length,
    the rank-deficient kinds, the long lists and the ladder."""
    K = k + 1
    out = [full_rank_case(k, M, 100 * k + i) for i, M in enumerate(list_lengths(k))]
    mid = 33 if K <= 33 else K + 1
    spec = [("a", K), ("a", 301), ("b", K), ("b", 301)]
    if k >= 3:
        spec += [("c", K + 1), ("c", mid), ("d", 301)]
    if k in (11, 128):
        out.append(full_rank_case(k, LONG_M, 100 * k + 50))
        spec.append(("b" if k == 11 else "a", LONG_M))
    out += [deficient_case(k, M, kind, 100 * k + 60 + i) for i, (kind, M) in enumerate(spec)]
    for lk, lM in LADDER_SHAPES:
        if lk == k:
            out += list(ladder(lk, lM))
    return tuple(out)


def batch_cases(k, pattern, lengths, seed):
    """Users for the batch tests: 'J' a rank-deficient list (kinds a, b, c, d
    in turn), 'C' a well-conditioned one, list lengths cycling through
    ``lengths``."""
    kinds = "abcd" if k >= 3 else "ab"
    out = []
    for i, p in enumerate(pattern):
        M = lengths[i % len(lengths)]
        if p == "J":
            out.append(deficient_case(k, M, kinds[i % len(kinds)], seed + i))
        else:
            out.append(full_rank_case(k, M, seed + i))
    return out


def sweep_factors(d, k, s, lv):
    """Factors (40 x k) of list s at level lv of tests/golden/foldin_sweep.npz."""
    V = d[f"V0_k{k}"][s].copy()
    V[:, 1] = d[f"col1_k{k}"][s, lv]
    return V


def build_table(cases):
    """One movie table holding the rows of all ``cases`` (same k):
    ``(V flat, als_ids, medians, lists)`` with movie ids that are not the ALS
    ids, and ``lists[i]`` the ``[(movie_id, rating)]`` of ``cases[i]``."""
    k = cases[0].k
    base, V, lists = 0, [], []
    for c in cases:
        assert c.k == k
        V.append(c.F)
        lists.append([(int(1000 + 3 * (base + r)), float(x)) for r, x in zip(c.rows, c.ratings)])
        base += len(c.F)
    als_ids = {1000 + 3 * j: j for j in range(base)}
    med = {m: 3.0 for m in als_ids}
    return np.concatenate(V).reshape(-1), als_ids, med, lists
