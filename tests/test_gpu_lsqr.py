"""The general sparse LSQR (``movie_recommender_amd.lsqr``, ``mr_lsqr_*``) on
the device against SciPy's ``lsqr``, on the matrices of tests/cgls_cases.py
(every row length and row count at which the CSR-stream SpMV changes path, on
A and on A^T).  The CPU references, bounds and admission conditions come from
tests/lsqr_cases.py and are computed once per process.

A  exact setup (iter_lim = 0): bit for bit;
B  exact one-step solve on a signed permutation: bit for bit;
C  fixed iteration counts within 20 x SciPy's own error (1e-13 at least);
D  SciPy's (istop, itn) at admitted stops, x bitwise a fixed-count run;
E  reproducibility, structure reuse and the value paths: bitwise.
"""
import math

import numpy as np
import pytest

import cgls_cases as C
import lsqr_cases as L

pytestmark = pytest.mark.gpu

SMALL = C.small_cases()
DEGENERATE = C.degenerate_cases()
ZERO = dict(atol=0.0, btol=0.0, conlim=0.0)


def ctx_of(case, vals=None, path=0):
    from movie_recommender_amd.lsqr import LsqrContext
    c = LsqrContext((case.rp, case.ci, case.vals if vals is None else vals, case.cols))
    c.set_gather_path(path)
    return c


@pytest.fixture(scope="module")
def ctxs(gpu):
    """One context per named matrix (the zoo's is built once)."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = ctx_of(L.case_by_name(name))
        return made[name]
    yield get
    for c in made.values():
        c.close()


def norms_of(res):
    return dict(zip(("istop", "itn") + L.NORM_KEYS, res[1:9]))


# ---------------------------------------------------------------------------
# A: exact setup
# ---------------------------------------------------------------------------
def check_exact_setup(ctx, case):
    b, x0, e, m, S = L.exact_setup(case)
    for bb, xx in ((b, x0), (e, None)):
        x, r = ctx.solve(bb, iter_lim=0, x0=xx)
        assert np.array_equal(x, x0 if xx is not None else np.zeros(case.cols))
        assert (r["istop"], r["itn"]) == (0, 0)
        assert r["r1norm"] == r["r2norm"] == 2.0 ** m, (r, m)
        assert r["arnorm"] == math.sqrt(S), (r["arnorm"], math.sqrt(S))
        assert r["anorm"] == 0.0 and r["acond"] == 0.0 and r["xnorm"] == 0.0
    # residual_l1 on the integer data: |b - A x0| = |e| sums to 4^m exactly
    assert ctx.residual_l1(b, x0) == float(np.sum(np.abs(e.astype(np.int64))))
    xi = case.x0.astype(np.int64)
    want = int(np.sum(np.abs(e.astype(np.int64) + case.A @ xi)))   # b - A 0 = b
    assert ctx.residual_l1(b, np.zeros(case.cols)) == float(want)


@pytest.mark.parametrize("case", SMALL, ids=[c.name for c in SMALL])
@pytest.mark.parametrize("path", [0, 1], ids=["buffer", "pointer"])
def test_exact_setup_small(gpu, case, path):
    with ctx_of(case, path=path) as ctx:
        check_exact_setup(ctx, case)


@pytest.mark.parametrize("path", [0, 1], ids=["buffer", "pointer"])
def test_exact_setup_zoo(gpu, ctxs, path):
    ctx = ctxs("zoo")
    ctx.set_gather_path(path)
    try:
        check_exact_setup(ctx, C.zoo())
    finally:
        ctx.set_gather_path(0)


@pytest.mark.parametrize("case", DEGENERATE, ids=[c.name for c in DEGENERATE])
def test_exact_setup_degenerate(gpu, case):
    with ctx_of(case) as ctx:
        for b in (case.b, np.zeros(case.rows)):
            for x0 in (case.x0, None):
                x, r = ctx.solve(b, iter_lim=0, x0=x0)
                assert np.array_equal(x, case.x0 if x0 is not None else np.zeros(case.cols))
                assert (r["istop"], r["itn"]) == (0, 0)
                assert r["arnorm"] == 0.0
                x, r = ctx.solve(b, x0=x0)   # default limits: the early return
                assert np.array_equal(x, case.x0 if x0 is not None else np.zeros(case.cols))
                assert (r["istop"], r["itn"]) == (0, 0) and r["arnorm"] == 0.0


def test_zero_rhs_returns_x0(gpu, ctxs):
    case = L.case_by_name("dense_col_2500x6")
    x, r = ctxs(case.name).solve(np.zeros(case.rows))
    assert np.array_equal(x, np.zeros(case.cols))
    assert (r["istop"], r["itn"], r["arnorm"], r["r1norm"]) == (0, 0, 0.0, 0.0)


# ---------------------------------------------------------------------------
# B: exact one-step solve
# ---------------------------------------------------------------------------
def test_exact_one_step(gpu):
    from movie_recommender_amd.lsqr import LsqrContext
    from scipy.sparse import linalg
    import scipy.sparse as sp
    rp, ci, vals, rows, cols, b = L.permutation_case()
    A = sp.csr_matrix((vals, ci, rp), shape=(rows, cols))
    want = A.T @ b
    with LsqrContext((rp, ci, vals, cols)) as ctx:
        for bb, kw in ((b, {}), (3.0 * b, dict(iter_lim=5, **ZERO))):
            ref = linalg.lsqr(A, bb, **kw)
            assert (ref[1], ref[2]) == (1, 1)
            scale = 3.0 if kw else 1.0
            assert np.array_equal(ref[0], scale * want)        # SciPy gives exactly this
            x, r = ctx.solve(bb, **kw)
            assert (r["istop"], r["itn"]) == (1, 1), r
            assert np.array_equal(x, scale * want)


# ---------------------------------------------------------------------------
# C: fixed iteration counts
# ---------------------------------------------------------------------------
def check_against(x, r, ref, bound, tag):
    refn = norms_of(ref)
    err = L.rel_max(x, ref[0])
    worst = err
    lines = [f"x {err:.2e}"]
    for key in L.NORM_KEYS:
        d = abs(r[key] - refn[key]) / max(abs(refn[key]), 1e-300)
        worst = max(worst, d)
        lines.append(f"{key} {d:.2e}")
    print(f"{tag}: bound {bound:.2e}; device " + ", ".join(lines), flush=True)
    assert (r["istop"], r["itn"]) == (refn["istop"], refn["itn"]), (r, refn)
    assert err <= bound, (tag, err, bound)
    for key in L.NORM_KEYS:
        assert abs(r[key] - refn[key]) <= bound * abs(refn[key]), (tag, key, r[key], refn[key])


@pytest.mark.parametrize("name,iter_lim,variant", L.FIXED_CASES,
                         ids=[f"{n}-it{i}-{'damp_x0' if v else 'plain'}" for n, i, v in L.FIXED_CASES])
def test_fixed_iterations(gpu, ctxs, name, iter_lim, variant):
    ref, bound, errs = L.fixed_reference(name, iter_lim, variant)
    b, damp, x0 = L.fixed_inputs(name, variant)
    x, r = ctxs(name).solve(b, damp=damp, iter_lim=iter_lim, x0=x0, **ZERO)
    check_against(x, r, ref, bound, f"{name} it={iter_lim} v{variant} scipy {max(errs):.1e}")


# ---------------------------------------------------------------------------
# D: stop rule
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,setting", L.STOP_CASES, ids=[f"{n}-{s}" for n, s in L.STOP_CASES])
def test_stop_rule(gpu, ctxs, name, setting):
    b, kw, ref, margins = L.stop_reference(name, setting)
    ctx = ctxs(name)
    x, r = ctx.solve(b, **kw)
    print(f"{name} {setting}: scipy {(ref[1], ref[2])} margins {margins} device "
          f"{(r['istop'], r['itn'])}", flush=True)
    assert (r["istop"], r["itn"]) == (ref[1], ref[2])
    # a stop changes no arithmetic: the fixed-count run at that itn
    damp = kw.get("damp", 0.0)
    xf, rf = ctx.solve(b, damp=damp, iter_lim=ref[2], **ZERO)
    assert rf["itn"] == ref[2]
    assert np.array_equal(x, xf)
    bound = L.stop_bound(name, setting)
    err = L.rel_max(x, ref[0])
    print(f"{name} {setting}: x error {err:.2e} bound {bound:.2e}", flush=True)
    assert err <= bound


# ---------------------------------------------------------------------------
# E: reproducibility, structure reuse, value paths
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["zoo", "dense_col_2500x6"])
def test_reproducible_and_reused(gpu, ctxs, name):
    case = L.case_by_name(name)
    b, x0 = L.gaussian_rhs(case, 41)
    b2, _ = L.gaussian_rhs(case, 42)
    kw = dict(damp=0.25, iter_lim=6, x0=x0, **ZERO)
    with ctx_of(case) as fresh:
        want = fresh.solve(b, **kw)
    ctx = ctxs(name)

    def same(got):
        assert np.array_equal(got[0], want[0])
        assert got[1] == want[1]
    same(ctx.solve(b, **kw))
    same(ctx.solve(b, **kw))
    ctx.solve(b2, iter_lim=4)
    same(ctx.solve(b, **kw))
    ctx.set_gather_path(1)
    try:
        same(ctx.solve(b, **kw))
    finally:
        ctx.set_gather_path(0)


@pytest.mark.parametrize("name", ["zoo", "dense_col_2500x6"])
def test_value_paths(gpu, name):
    case = L.case_by_name(name)
    rng = np.random.default_rng(51)
    b, _ = L.gaussian_rhs(case, 43)
    v2 = rng.standard_normal(len(case.vals))
    kw = dict(iter_lim=4, **ZERO)
    with ctx_of(case, vals=v2) as c2:
        want = c2.solve(b, **kw)
    table = rng.standard_normal(97)
    index = rng.integers(-1, 97, len(case.vals))
    gathered = np.where(index < 0, 1.0, table[np.maximum(index, 0)])
    with ctx_of(case) as c1:
        c1.set_values(v2)
        got = c1.solve(b, **kw)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1]
        c1.set_values(gathered)
        wg = c1.solve(b, **kw)
        c1.set_values(v2)
        c1.set_value_map(index)
        c1.set_values_from_table(table)
        gg = c1.solve(b, **kw)
        assert np.array_equal(gg[0], wg[0]) and gg[1] == wg[1]
        with pytest.raises(RuntimeError):
            c1.set_values_from_table(table[:int(index.max())])   # one entry short


def test_lsqr_function_matches_scipy_tuple(gpu):
    from movie_recommender_amd.lsqr import lsqr
    from scipy.sparse import linalg
    case = L.case_by_name("full_block_256x8")
    A = L.csr_of(case)
    b, _ = L.gaussian_rhs(case, 44)
    got = lsqr(A, b)
    ref = linalg.lsqr(A, b)
    assert len(got) == 10 and (got[1], got[2]) == (ref[1], ref[2])
    assert L.rel_max(got[0], ref[0]) <= 1e-12
    assert got[9].shape == (case.cols,) and not got[9].any()
