"""General sparse least-squares cases whose first CG steps are known exactly,
for the CSR-stream SpMV (``csr_spmv_kernel``) behind ``mr_cg_solve`` and
``cg_least_squares_from_python``.  No GPU import here: everything is NumPy /
SciPy on the CPU and none of it comes from the code under test.

Exact data.  Every matrix value is +-1 and ``b``, ``x0`` are drawn from
{-1, 0, 1}, so ``A x0``, ``A^T b``, ``r0 = A^T A x0 - A^T b``, ``p0 = -r0``,
``rr0 = r0.r0`` and, in iteration 0, ``t = A p0``, ``q = A^T t`` and ``pAp =
p0.q`` are integers (computed here in int64).  While the sum of the absolute
terms of a dot product stays below 2^53 every partial sum of it is an integer
fp64 holds exactly, so any summation order gives the same bits: the device's
per-thread, per-block and partials reductions need no tolerance.  ``Case``
asserts this for every row sum and, as the issue of these tests states it,
``sum r0_j^2 < 2^52`` and ``sum |p0_j q_j| < 2^52`` -- conditions on the
inputs, checked on the CPU, not measurements.

``restate(case, max_it)`` gives the solve after 0 and 1 iterations as
``oracle/als_oracle.py:cg_normal`` and the device's ``cg_finalize`` /
``cgls_update_kernel`` state it: ``alpha = fl(rr0) / fl(pAp)``, ``x1 = x0 +
alpha p0`` and ``r1 = r0 + alpha q`` elementwise in fp64 with multiply and add
each rounded (the device computes ``1.0 * x + alpha * p`` with contraction
off), ``rr1 = fsum(r1^2)``.

``block_lists`` restates the row blocks: the device orders A's rows by a
stable sort of each row's first listed column (an empty row's key is
``cols``), and the host cuts both the permuted A and its transpose greedily
into blocks of at most ``max_nnz`` non-zeros and ``max_rows`` rows, a longer
row being a block of its own.

``zoo()`` is the one large case: P (R x 4096) holds two copies of an edge
section -- rows and row runs at every limit of the kernel, each run closed by
a row above the tile, so that the greedy cut yields the runs as blocks -- and
a pipeline section of >= 4200 random blocks, and the matrix is ``A =
blockdiag(P, P^T)`` (P^T's columns after P's), so that ``A^T = blockdiag(P^T,
P)`` and P's row shapes pass through the kernels of A and of A^T both.
"""
import copy
import functools
import math

import numpy as np
import scipy.sparse as sp

from oracle import als_oracle as O

TILE = 2048          # kSpTile: a block's non-zero limit (mr_cg_stats.block_max_nnz)
MAX_ROWS = 256       # kSpMaxRows (mr_cg_stats.block_max_rows)
MAX_PARTS = 2048     # kMaxParts: the SpMV grid's upper limit
ZOO_COLS = 4096
PIPE_BLOCKS = 4200


class Case:
    """A CSR matrix (int32 ``rp``, ``ci``; ``vals`` = +-1) with exact ``b``,
    ``x0``; the integer setup and iteration-0 quantities are attributes."""

    def __init__(self, name, rows, cols, rp, ci, vals, b, x0):
        self.name = name
        self.rows, self.cols = int(rows), int(cols)
        self.rp = np.ascontiguousarray(rp, np.int32)
        self.ci = np.ascontiguousarray(ci, np.int32)
        self.vals = np.ascontiguousarray(vals, np.float64)
        assert len(self.rp) == self.rows + 1 and self.rp[0] == 0
        assert len(self.ci) == len(self.vals) == self.rp[-1]
        assert np.all(np.abs(self.vals) == 1.0)
        self.set_rhs(b, x0)

    @functools.cached_property
    def A(self):
        # duplicates stay listed: a matvec adds every listed entry, as the
        # reference's and the device's row loops do
        return sp.csr_matrix((self.vals.astype(np.int64), self.ci.astype(np.int64),
                              self.rp.astype(np.int64)), shape=(self.rows, self.cols))

    @functools.cached_property
    def At(self):
        return self.A.T.tocsr()

    def set_rhs(self, b, x0):
        """Take (b, x0), compute the integer quantities and assert the
        exactness conditions."""
        self.b = np.ascontiguousarray(b, np.float64)
        self.x0 = np.ascontiguousarray(x0, np.float64)
        assert self.b.shape == (self.rows,) and self.x0.shape == (self.cols,)
        assert np.all(np.isin(self.b, (-1.0, 0.0, 1.0)))
        assert np.all(np.isin(self.x0, (-1.0, 0.0, 1.0)))
        A, At = self.A, self.At
        absA, absAt = abs(A), abs(At)

        def mv(M, absM, v):
            # every row sum's absolute terms stay below 2^53 (float screen
            # first, so that the int64 sums cannot have wrapped)
            if len(v) and M.shape[0]:
                assert float(np.max(absM.astype(np.float64) @ np.abs(v).astype(np.float64),
                                    initial=0.0)) < 2.0 ** 52
            return M @ v

        bi, xi = self.b.astype(np.int64), self.x0.astype(np.int64)
        self.b2 = mv(At, absAt, bi)
        self.r0 = mv(At, absAt, mv(A, absA, xi)) - self.b2
        self.p0 = -self.r0
        self.t0 = mv(A, absA, self.p0)
        self.q0 = mv(At, absAt, self.t0)
        rf, pf, qf = (a.astype(np.float64) for a in (self.r0, self.p0, self.q0))
        assert float(np.sum(rf * rf)) < 2.0 ** 51 and float(np.sum(np.abs(pf * qf))) < 2.0 ** 51
        self.rr0 = int(np.sum(self.r0 * self.r0))
        self.pAp = int(np.sum(self.p0 * self.q0))
        self.abs_pq = int(np.sum(np.abs(self.p0 * self.q0)))
        # the two conditions of the exact tiers
        assert self.rr0 < 2 ** 52, self.rr0
        assert self.abs_pq < 2 ** 52, self.abs_pq
        return self


def restate(case, max_it):
    """(iterations, x, final_rr) after max_it = 0 or 1, restating cg_normal
    and the device's finalize rules on the exact quantities."""
    assert max_it in (0, 1)
    if max_it == 0 or case.rr0 < 1e-6:
        return 0, case.x0.copy(), float(case.rr0)
    alpha = np.float64(case.rr0) / np.float64(case.pAp)
    x1 = case.x0 + alpha * case.p0.astype(np.float64)
    r1 = case.r0.astype(np.float64) + alpha * case.q0.astype(np.float64)
    return 1, x1, math.fsum(r1 * r1)


def oracle(case, max_it, min_dec=0.01, reverse_rows=False):
    """The existing fp64 oracle on the case; with reverse_rows on the same
    system listed bottom-up (another summation order in A^T's products)."""
    rp, ci, vals, b = case.rp, case.ci, case.vals, case.b
    if reverse_rows:
        M = case.A[::-1].tocsr()
        rp, ci, vals, b = M.indptr, M.indices, M.data.astype(np.float64), b[::-1]
    return O.cg_least_squares(rp, ci, vals, case.cols, b, case.x0, min_dec, max_it)


def cg_longdouble(case, max_it, min_dec=0.01):
    """cg_normal with every product and sum in np.longdouble: (x, iterations)."""
    ld = np.longdouble
    A = sp.csr_matrix((case.vals.astype(ld), case.ci.astype(np.int64), case.rp.astype(np.int64)),
                      shape=(case.rows, case.cols))
    At = A.T.tocsr()
    x = case.x0.astype(ld)
    r = At @ (A @ x) - At @ case.b.astype(ld)
    p = -r
    rr = np.dot(r, r)
    it = fails = 0
    while it < max_it:
        if rr < 1e-6:
            break
        Ap = At @ (A @ p)
        alpha = rr / np.dot(p, Ap)
        x = x + alpha * p
        r = r + alpha * Ap
        rr2 = np.dot(r, r)
        beta = rr2 / rr
        fails = fails + 1 if beta > 1 - min_dec else 0
        if fails >= 2:
            break
        p = -r + beta * p
        rr = rr2
        it += 1
    return x, it


def tolerance_from_reference(case, max_it):
    """The bound for the device's x after max_it iterations, from the
    reference alone: 20 x the larger relative error of the fp64 oracle in two
    summation orders (rows as given, rows reversed) against the longdouble
    restatement, 1e-13 at the least.  Returns (x_longdouble as fp64, oracle
    iterations, tolerance, (error as given, error reversed))."""
    xl, itl = cg_longdouble(case, max_it)
    xo, ito, _ = oracle(case, max_it)
    xr, itr, _ = oracle(case, max_it, reverse_rows=True)
    assert ito == itr == itl, (ito, itr, itl)
    scale = max(float(np.max(np.abs(xl), initial=0.0)), 1e-300)
    errs = tuple(float(np.max(np.abs(v.astype(np.longdouble) - xl), initial=0.0)) / scale
                 for v in (xo, xr))
    return xl.astype(np.float64), ito, max(1e-13, 20 * max(errs)), errs


# ---------------------------------------------------------------------------
# row blocks
# ---------------------------------------------------------------------------
def device_row_order(case):
    """The device's row permutation: a stable sort by first listed column,
    empty rows (key = cols) last."""
    key = np.full(case.rows, case.cols, np.int64)
    ne = case.rp[1:] > case.rp[:-1]
    key[ne] = case.ci[case.rp[:-1][ne]]
    return np.argsort(key, kind="stable")


def cut_blocks(lengths, max_nnz=TILE, max_rows=MAX_ROWS):
    """Greedy row blocks of a matrix with the given row lengths: a list of
    (first row, rows, first non-zero, non-zeros)."""
    off = np.concatenate([[0], np.cumsum(np.asarray(lengths, np.int64))])
    rows = len(off) - 1
    out = []
    r = 0
    while r < rows:
        s = r
        if off[s + 1] - off[s] > max_nnz:
            r = s + 1
        else:   # the last row whose end stays within max_nnz of the block's start
            r = min(s + max_rows, int(np.searchsorted(off, off[s] + max_nnz, side="right")) - 1)
        out.append((s, r - s, int(off[s]), int(off[r] - off[s])))
    return out


def row_lengths(case):
    """Row lengths of the device's A (rows in its order) and of its transpose."""
    la = np.diff(case.rp.astype(np.int64))[device_row_order(case)]
    lt = np.bincount(case.ci, minlength=case.cols).astype(np.int64)
    return la, lt


def block_lists(case, max_nnz=TILE, max_rows=MAX_ROWS):
    """(blocks of the permuted A, blocks of its transpose), each a list of
    (first row, rows, first non-zero, non-zeros)."""
    la, lt = row_lengths(case)
    return cut_blocks(la, max_nnz, max_rows), cut_blocks(lt, max_nnz, max_rows)


def with_rhs(case, b, x0):
    """The same matrix with another exact (b, x0)."""
    return copy.copy(case).set_rhs(b, x0)


# ---------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------
def _pm1(rng, n):
    return rng.integers(0, 2, n) * 2.0 - 1.0


def _tern(rng, n):
    return rng.integers(-1, 2, n).astype(np.float64)


def _from_rows(name, rows_cols, cols, seed):
    """A case from a list of per-row column-id lists (listed order kept)."""
    rng = np.random.default_rng(seed)
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows_cols])]).astype(np.int64)
    ci = np.concatenate([np.asarray(r, np.int64) for r in rows_cols] + [np.zeros(0, np.int64)])
    return Case(name, len(rows_cols), cols, rp, ci, _pm1(rng, len(ci)),
                _tern(rng, len(rows_cols)), _tern(rng, cols))


def degenerate_cases():
    """No rows, no columns, neither, and rows without a non-zero: the oracle
    gives 0 iterations, rr = 0 and x untouched."""
    return [_from_rows("rows0", [], 5, 1), _from_rows("cols0", [[], [], []], 0, 2),
            _from_rows("rows0_cols0", [], 0, 3), _from_rows("all_empty_300x7", [[]] * 300, 7, 4)]


def small_cases():
    rng = np.random.default_rng(11)
    out = []
    # duplicate and unsorted column ids within rows
    rows = [list(rng.integers(0, 9, int(n))) for n in rng.integers(1, 14, 40)]
    rows[3] = [5, 5, 5, 2, 2, 8, 0, 5]
    rows[7] = [8, 7, 6, 5, 4, 3, 2, 1, 0]
    out.append(_from_rows("dup_unsorted_40x9", rows, 9, 12))
    # one dense column: A^T holds one row above the tile
    rows = [[2] + list(rng.choice([0, 1, 3, 4, 5], int(rng.integers(0, 3)), replace=False))
            for _ in range(2500)]
    out.append(_from_rows("dense_col_2500x6", rows, 6, 13))
    c = Case("one_by_one", 1, 1, [0, 1], [0], [1.0], [1.0], [-1.0])
    out.append(c)
    # exactly one full block: 256 rows x 8 = 2048 non-zeros
    rows = [sorted(rng.choice(64, 8, replace=False)) for _ in range(256)]
    out.append(_from_rows("full_block_256x8", rows, 64, 14))
    return out


# The edge section, run by run (rows x length).  A row above the tile closes
# every run, so the greedy cut starts each run on a fresh block.
EDGE_RUNS = [
    [1], [2], [15], [16], [17], [2047], [2048], [2049], [4000], [2305],
    [1024, 1024], [1000, 1048], [1000, 1000], [400] * 5,
    [16] * 128, [16] * 129, [8] * 256, [8] * 257, [7] * 256, [9] * 256,
    [1] * 256, [1] * 300, [0] * 3, [1, 0, 0, 5, 0],
    # every row count at which the row-sum group G changes (G = the largest
    # power of two <= 256 / rows, at most 64), with rows on both sides of the
    # 16-terms-per-thread split (length 16 G) in each
    [15] * 128, [15] * 129, [14, 15, 16, 17] * 32 + [15],            # G = 2 | 1
    [32] * 64, [30, 31, 32, 33] * 16 + [31], [31] * 65,              # G = 4 | 2
    [64] * 32, [63, 64, 65, 60] * 8 + [62],                          # G = 8 | 4
    [128] * 16, [127, 128, 129, 100] * 4 + [110],                    # G = 16 | 8
    [256] * 8, [255, 257, 256, 200] * 2 + [210],                     # G = 32 | 16
    [512] * 4, [511, 513, 300, 200, 100],                            # G = 64 | 32
    [1023, 1025], [1025, 1023], [682, 683, 683],                     # G = 64
    [0] * 256, [0] * 600,                                            # whole blocks of empty rows
]
TAIL_RUNS = [[2048], [1], [2049], [2049], [3]]


def _zoo_lengths(rng, pipe_blocks):
    def edge():
        parts = []
        for run in EDGE_RUNS:
            parts.append(np.asarray(run, np.int64))
            parts.append(rng.integers(2049, 2101, 1))
        return parts

    def pipe(n):
        kinds = rng.choice(5, n, p=[0.08, 0.29, 0.29, 0.29, 0.05])
        parts = []
        for k in kinds:
            if k == 0:
                parts.append(rng.integers(2049, 2101, 1))
            elif k == 1:
                parts.append(np.ones(256, np.int64))
            elif k == 2:
                parts.append(rng.integers(0, 9, 256))
            elif k == 3:
                parts.append(rng.integers(100, 701, int(rng.integers(1, 6))))
            else:
                parts.append(np.full(1, 2048, np.int64))
        return parts
    # an edge section first (its blocks are a workgroup's first, loaded into
    # `cur` before the loop) and another in the middle (loaded ahead into `nxt`)
    parts = edge() + pipe(pipe_blocks // 2) + edge() + pipe(pipe_blocks - pipe_blocks // 2)
    parts += [np.asarray(r, np.int64) for r in TAIL_RUNS]
    return np.concatenate(parts).astype(np.int64)


@functools.lru_cache(maxsize=1)
def zoo(seed=5, pipe_blocks=PIPE_BLOCKS):
    rng = np.random.default_rng(seed)
    L = _zoo_lengths(rng, pipe_blocks)
    R = len(L)
    off = np.concatenate([[0], np.cumsum(L)])
    nnz = int(off[-1])
    # row i: its first column i * 64 // R (non-decreasing, so the device's row
    # order keeps P's non-empty rows in place), then L - 1 distinct columns
    # spread over (first, 4095] with a random phase
    row = np.repeat(np.arange(R), L)
    k = np.arange(nnz) - off[row]
    first = row * 64 // R
    span = (ZOO_COLS - 1 - first).astype(np.float64)
    u = rng.random(R)[row]
    rest = first + 1 + np.floor((k - 1 + u) * span / np.maximum(L[row] - 1, 1)).astype(np.int64)
    ci = np.where(k == 0, first, rest)
    assert ci.min() >= 0 and ci.max() < ZOO_COLS
    inner = np.ones(nnz, bool)
    inner[off[:-1][L > 0]] = False
    assert np.all(np.diff(ci)[inner[1:]] > 0)       # distinct, ascending within a row
    P = sp.csr_matrix((_pm1(rng, nnz), ci, off), shape=(R, ZOO_COLS))
    Pt = P.T.tocsr()
    Pt.sort_indices()
    rp = np.concatenate([off, nnz + Pt.indptr[1:].astype(np.int64)])
    cols = np.concatenate([ci, Pt.indices.astype(np.int64) + ZOO_COLS])
    vals = np.concatenate([P.data, Pt.data])
    n = R + ZOO_COLS
    c = Case("zoo", n, n, rp, cols, vals, _tern(rng, n), _tern(rng, n))
    c.p_rows = R
    c.p_lengths = L
    c.rhs2 = (_tern(rng, n), _tern(rng, n))    # another exact (b, x0) for context reuse
    return c
