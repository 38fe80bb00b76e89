"""The CSR-stream SpMV of the general least squares (``csr_spmv_kernel``,
``row_blocks``, ``sort_rows_by_first_col``, ``build_csr``) at its block and
pipeline edges, on the exact cases of tests/cgls_cases.py: integer data whose
setup and first CG iteration have one right answer in fp64 whatever the
summation order, so 0 and 1 iterations are compared bit for bit.

The zoo (631,500 square, 9,062,204 non-zeros, 5,842 row blocks of A and 5,989
of A^T -- more than twice the grid's upper limit of 2,048 workgroups, so every
workgroup's software pipeline advances at least twice) puts rows of 2047 /
2048 / 2049 non-zeros, blocks of exactly 256 rows, 256 rows x 8, every row
count at which the row-sum group changes, the 16-terms split, blocks of empty
rows, odd block offsets and a ragged last block through the kernels of A and
of A^T.  Every case runs on the buffer-load instantiations and again on their
pointer-load twins (``mr_cg_set_gather_path``), which a caller reaches only
with a 4 GiB vector.

Three iterations (the ``SPG_P`` gather, ``update_p = 1``) have no exact
answer; the bound comes from the reference alone (cgls_cases.
tolerance_from_reference).  Measured on the zoo: fp64 oracle against the
longdouble restatement 5.1e-13 .. 5.2e-13 (rows as given) and 3.8e-13 ..
4.0e-13 (rows reversed) by NumPy build, so the bound is 1.02e-11 .. 1.05e-11;
the device is at 1.9e-15 on either gather path."""
import ctypes

import numpy as np
import pytest

import cgls_cases as C

pytestmark = pytest.mark.gpu

PATHS = [0, 1]
PATH_IDS = ["buffer", "pointer"]
SMALL = C.small_cases()
DEGENERATE = C.degenerate_cases()


class Ctx:
    """A device context (include/mr_cg.h) on one gather path."""

    def __init__(self, L, case, path):
        from movie_recommender_amd import _lib
        self._lib, self.L, self.case = _lib, L, case
        self.h = L.mr_cg_create(0, case.rows, case.cols, case.rp.ctypes.data_as(_lib.IP),
                                case.ci.ctypes.data_as(_lib.IP), case.vals.ctypes.data_as(_lib.DP))
        assert self.h, _lib.last_error()
        _lib.check(L.mr_cg_set_gather_path(self.h, path), "mr_cg_set_gather_path")

    def solve(self, case, max_it, min_dec=0.01):
        x = case.x0.copy()
        rr = ctypes.c_double(-1.0)
        it = self.L.mr_cg_solve(self.h, case.b.ctypes.data_as(self._lib.DP),
                                x.ctypes.data_as(self._lib.DP), min_dec, max_it, ctypes.byref(rr))
        assert it >= 0, self._lib.last_error()
        return it, x, rr.value

    def stats(self):
        st = self._lib.MrCgStats()
        self._lib.check(self.L.mr_cg_get_stats(self.h, ctypes.byref(st)), "mr_cg_get_stats")
        return st.as_dict()

    def close(self):
        if self.h:
            self.L.mr_cg_destroy(self.h)
            self.h = None


def _abi(fn, case, max_it):
    from movie_recommender_amd import _lib
    x = case.x0.copy()
    rr = ctypes.c_double(-1.0)
    it = fn(case.rows, case.cols, case.rp.ctypes.data_as(_lib.IP), case.ci.ctypes.data_as(_lib.IP),
            case.vals.ctypes.data_as(_lib.DP), case.rows, case.b.ctypes.data_as(_lib.DP), case.cols,
            x.ctypes.data_as(_lib.DP), 0.01, max_it, ctypes.byref(rr))
    assert it >= 0, _lib.last_error()
    return it, x, rr.value


def _where(x, case):
    """On a wrong x after one iteration: is (x - x0) / p0 one constant?  Then
    the step is along the right p0 with a wrong alpha -- the fault is in A p0
    or A^T t, not in the setup."""
    nz = case.p0 != 0
    bad = int(np.sum(x != C.restate(case, 1)[1]))
    if not nz.any() or np.any(x[~nz] != case.x0[~nz]):
        return f"{bad} wrong entries; x moved where p0 = 0: the setup (r0, p0) is wrong"
    ratio = (x[nz] - case.x0[nz]) / case.p0[nz]
    spread = float(np.max(ratio) - np.min(ratio))
    alpha = case.rr0 / case.pAp
    if spread <= 1e-9 * abs(alpha):
        return (f"{bad} wrong entries; (x - x0) / p0 is constant ({ratio[0]!r}, expected "
                f"{alpha!r}): p0 is right, the fault is in A p0 or A^T t")
    return f"{bad} wrong entries; (x - x0) / p0 is not constant: the setup (r0, p0) is wrong"


def check_exact_tiers(solve, case):
    """max_iteration 0: returns 0, x bit-identical to x0, final_rr == rr0 (the
    three setup SpMVs and the INIT update).  max_iteration 1: returns 1, x ==
    x1 bit for bit, |final_rr - rr1| <= N 2^-53 rr1 (N positive terms: the
    worst case of any summation order)."""
    it, x, rr = solve(case, 0)
    assert it == 0
    assert np.array_equal(x, case.x0)
    assert rr == float(case.rr0), (rr, case.rr0)
    it1, x1, rr1 = C.restate(case, 1)
    it, x, rr = solve(case, 1)
    assert it == it1
    assert np.array_equal(x, x1), _where(x, case)
    print(f"{case.name}: rr1 device {rr!r} restated {rr1!r}", flush=True)
    assert abs(rr - rr1) <= case.cols * 2.0 ** -53 * rr1, (rr, rr1)


# ---------------------------------------------------------------------------
# the zoo
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def zoo_ctxs(gpu):
    z = C.zoo()
    ctxs = [Ctx(gpu, z, p) for p in PATHS]
    yield ctxs
    for c in ctxs:
        c.close()


@pytest.fixture(scope="module")
def zoo_reference3():
    return C.tolerance_from_reference(C.zoo(), 3)


@pytest.mark.parametrize("path", PATHS, ids=PATH_IDS)
def test_zoo_block_counts(zoo_ctxs, path):
    """The library's row blocks are the restated ones, and there are more than
    two per workgroup of the largest grid on both sides: without this the
    pipeline tests below prove nothing."""
    s = zoo_ctxs[path].stats()
    ba, bt = C.block_lists(C.zoo(), s["block_max_nnz"], s["block_max_rows"])
    assert (s["block_max_nnz"], s["block_max_rows"]) == (C.TILE, C.MAX_ROWS)
    assert (s["blocks_a"], s["blocks_at"]) == (len(ba), len(bt))
    assert s["blocks_a"] > 2 * C.MAX_PARTS and s["blocks_at"] > 2 * C.MAX_PARTS
    assert s["nnz"] == len(C.zoo().ci)


@pytest.mark.parametrize("path", PATHS, ids=PATH_IDS)
def test_zoo_exact_setup_and_first_iteration(zoo_ctxs, path):
    check_exact_tiers(zoo_ctxs[path].solve, C.zoo())


@pytest.mark.parametrize("path", PATHS, ids=PATH_IDS)
def test_zoo_context_reuse(gpu, zoo_ctxs, path):
    """Another exact (b, x0) on the used context: exact as the first, and
    three iterations equal a fresh context's bit for bit."""
    z = C.zoo()
    z2 = C.with_rhs(z, *z.rhs2)
    used = zoo_ctxs[path]
    used.solve(z, 3)
    check_exact_tiers(used.solve, z2)
    got = used.solve(z2, 3)
    fresh = Ctx(gpu, z, path)
    try:
        want = fresh.solve(z2, 3)
    finally:
        fresh.close()
    assert got[0] == want[0] == 3 and got[2] == want[2] and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("path", PATHS, ids=PATH_IDS)
def test_zoo_three_iterations(zoo_ctxs, zoo_reference3, path):
    """The SPG_P gather and update_p = 1 against the longdouble restatement,
    within 20 x the fp64 oracle's own error against it (measured: 5.2e-13
    with the rows as given, 4.0e-13 reversed, bound 1.05e-11; device
    1.9e-15)."""
    xl, it_ref, tol, errs = zoo_reference3
    it, x, rr = zoo_ctxs[path].solve(C.zoo(), 3)
    err = float(np.max(np.abs(x - xl)) / np.max(np.abs(xl)))
    print(f"zoo, 3 iterations: oracle errors {errs[0]:.3e} / {errs[1]:.3e}, bound {tol:.3e}, "
          f"device {err:.3e}", flush=True)
    assert it == it_ref
    assert err <= tol, (err, tol)


def test_zoo_pointer_path_is_bit_identical(zoo_ctxs):
    """The same products in the same order: x, the iteration count and
    final_rr after three iterations do not depend on the gather path."""
    a, b = (c.solve(C.zoo(), 3) for c in zoo_ctxs)
    assert a[0] == b[0] and a[2] == b[2] and np.array_equal(a[1], b[1])


# ---------------------------------------------------------------------------
# small cases
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("case", SMALL, ids=[c.name for c in SMALL])
def test_small_cases(gpu, case, path):
    ctx = Ctx(gpu, case, path)
    try:
        s = ctx.stats()
        ba, bt = C.block_lists(case, s["block_max_nnz"], s["block_max_rows"])
        assert (s["blocks_a"], s["blocks_at"]) == (len(ba), len(bt))
        check_exact_tiers(ctx.solve, case)
        xl, it_ref, tol, errs = C.tolerance_from_reference(case, 3)
        it, x, rr = ctx.solve(case, 3)
        assert it == it_ref
        assert np.max(np.abs(x - xl)) <= tol * np.max(np.abs(xl)), (case.name, tol, errs)
        if path:
            other = Ctx(gpu, case, 0)
            try:
                itb, xb, rrb = other.solve(case, 3)
            finally:
                other.close()
            assert it == itb and rr == rrb and np.array_equal(x, xb)
    finally:
        ctx.close()


@pytest.mark.parametrize("case", SMALL, ids=[c.name for c in SMALL])
def test_small_cases_through_reference_abi(gpu, case):
    for fn in (gpu.cg_least_squares_from_python, gpu.cg_least_squares2_from_python):
        check_exact_tiers(lambda c, max_it: _abi(fn, c, max_it), case)


@pytest.mark.parametrize("path", PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("case", DEGENERATE, ids=[c.name for c in DEGENERATE])
def test_degenerate_cases(gpu, case, path):
    """No rows, no columns, no non-zeros: as the oracle, 0 iterations, rr = 0
    and x untouched, whatever max_iteration."""
    ctx = Ctx(gpu, case, path)
    try:
        s = ctx.stats()
        ba, bt = C.block_lists(case, s["block_max_nnz"], s["block_max_rows"])
        assert (s["blocks_a"], s["blocks_at"]) == (len(ba), len(bt))
        for max_it in (0, 1, 3):
            it, x, rr = ctx.solve(case, max_it)
            assert it == 0 and rr == 0.0 and np.array_equal(x, case.x0)
    finally:
        ctx.close()
    if path == 0:
        for max_it in (0, 3):
            it, x, rr = _abi(gpu.cg_least_squares_from_python, case, max_it)
            assert it == 0 and rr == 0.0 and np.array_equal(x, case.x0)


def test_gather_path_rejects_unknown_mode(gpu):
    c = Ctx(gpu, SMALL[2], 0)
    try:
        assert gpu.mr_cg_set_gather_path(c.h, 2) < 0
        assert gpu.mr_cg_set_gather_path(c.h, -1) < 0
        assert gpu.mr_cg_set_gather_path(None, 0) < 0
    finally:
        c.close()
