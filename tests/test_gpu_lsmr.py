"""The sparse LSMR (``LsqrContext.solve_lsmr``, ``movie_recommender_amd.lsmr``,
``mr_lsqr_solve_lsmr``) on the device against SciPy's ``lsmr``, on the
matrices of tests/cgls_cases.py and the right-hand sides of
tests/lsqr_cases.py.  The CPU references, bounds and admission conditions
come from tests/lsmr_cases.py and are computed once per process.

A  exact setup (maxiter = 0) and SciPy's zero-b return: bit for bit;
B  exact one-step solve on a signed permutation (the beta == 0 branch): bit
   for bit;
C  fixed iteration counts within 20 x SciPy's own error over x and the five
   norms (1e-13 at least);
D  SciPy's (istop, itn) at admitted stops, x bitwise a fixed-count run;
E  LSQR / LSMR interleaved on one context, value paths, gather paths: bitwise;
F  ``lsmr()`` and ``als_lsmr`` against SciPy's lsmr chained on the CPU.
"""
import math

import numpy as np
import pytest

import cgls_cases as C
import lsmr_cases as M
import lsqr_cases as L

pytestmark = pytest.mark.gpu

SMALL = C.small_cases()
DEGENERATE = C.degenerate_cases()
ZERO = dict(atol=0.0, btol=0.0, conlim=0.0)
EPS = np.finfo(np.float64).eps


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
            made[name] = ctx_of(M.case_by_name(name))
        return made[name]
    yield get
    for c in made.values():
        c.close()


def same(got, want):
    assert np.array_equal(got[0], want[0])
    assert got[1] == want[1], (got[1], want[1])


# ---------------------------------------------------------------------------
# A: exact setup, SciPy's zero-b return
# ---------------------------------------------------------------------------
def check_exact_setup(ctx, case):
    b, x0, e, m, S = M.exact_setup(case)
    alpha = math.sqrt(S) / 2.0 ** m
    for bb, xx in ((b, x0), (e, None)):
        x, r = ctx.solve_lsmr(bb, maxiter=0, x0=xx)
        assert np.array_equal(x, x0 if xx is not None else np.zeros(case.cols))
        assert (r["istop"], r["itn"]) == (0, 0)
        assert r["normr"] == 2.0 ** m, (r, m)
        assert r["normar"] == math.sqrt(S), (r["normar"], math.sqrt(S))
        assert r["norma"] == np.sqrt(alpha * alpha), (r["norma"], alpha)
        assert r["conda"] == 1.0 and r["normx"] == 0.0
    x, r = ctx.solve_lsmr(np.zeros(case.rows))
    assert not x.any()
    assert r == dict(istop=0, itn=0, normr=0.0, normar=0.0, norma=0.0, conda=1.0, normx=0.0)


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
    """No product to take: alpha = 0, so normar == 0 returns x0 untouched
    (before the zero-b rule), with normr = ||b|| on the ternary b."""
    with ctx_of(case) as ctx:
        for b in (case.b, np.zeros(case.rows)):
            for x0 in (case.x0, None):
                for kw in (dict(maxiter=0), dict()):
                    x, r = ctx.solve_lsmr(b, x0=x0, **kw)
                    assert np.array_equal(x, case.x0 if x0 is not None else np.zeros(case.cols))
                    assert (r["istop"], r["itn"]) == (0, 0)
                    assert r["normr"] == math.sqrt(float(np.sum(b * b)))
                    assert r["normar"] == 0.0 and r["norma"] == 0.0
                    assert r["conda"] == 1.0 and r["normx"] == 0.0


def zero_b_expected(case):
    """(normr, normar = norma * normr, the setup's rounding bound) for b = 0,
    x0 = the case's: u = -A x0 and g = A^T A x0 are integers, so beta =
    sqrt(sum u^2) is exact; v = A^T (u / beta) rounds once per scaled entry
    and once per addition, a relative (terms + 2) eps on sum |a| |u| per
    entry, and alpha, alpha * beta, sqrt(alpha^2) add one rounding each."""
    A = L.csr_of(case)
    u = A @ case.x0
    g = A.T @ u
    absg = np.zeros(case.cols)
    np.add.at(absg, case.ci, np.repeat(np.abs(u), np.diff(case.rp)))   # |A|^T |u|, values +-1
    terms = int(np.max(np.bincount(case.ci, minlength=1)))
    ng = math.sqrt(float(np.sum(g * g)))
    tol = ((terms + 2) * float(np.sqrt(np.sum(absg * absg))) / ng + 4) * EPS
    return math.sqrt(float(np.sum(u * u))), ng, tol


@pytest.mark.parametrize("case", SMALL, ids=[c.name for c in SMALL])
def test_zero_rhs_with_x0_returns_zero_like_scipy(gpu, case):
    from scipy.sparse import linalg
    normr, normar, tol = zero_b_expected(case)
    assert normr > 0 and normar > 0
    with ctx_of(case) as ctx:
        for kw in (dict(), dict(maxiter=0)):
            x, r = ctx.solve_lsmr(np.zeros(case.rows), x0=case.x0, **kw)
            assert x.shape == (case.cols,) and not x.any()
            assert (r["istop"], r["itn"]) == (0, 0)
            assert r["normr"] == normr
            assert abs(r["normar"] - normar) <= tol * normar, (r["normar"], normar, tol)
            assert abs(r["norma"] - normar / normr) <= tol * normar / normr
            assert r["conda"] == 1.0 and r["normx"] == 0.0
        if case.name == "dup_unsorted_40x9":
            ref = linalg.lsmr(L.csr_of(case), np.zeros(case.rows), x0=case.x0)
            assert not ref[0].any() and (ref[1], ref[2]) == (0, 0)
            assert r["normr"] == ref[3] and ref[6] == 1 and ref[7] == 0
            assert abs(r["normar"] - ref[4]) <= 2 * tol * ref[4]
            assert abs(r["norma"] - ref[5]) <= 2 * tol * ref[5]
        # the context is left clean: a solve after the zeroed return
        b, x0, e, m, S = M.exact_setup(case)
        x, r = ctx.solve_lsmr(b, maxiter=0, x0=x0)
        assert np.array_equal(x, x0) and r["normr"] == 2.0 ** m


# ---------------------------------------------------------------------------
# B: exact one-step solve
# ---------------------------------------------------------------------------
def test_exact_one_step(gpu):
    from movie_recommender_amd.lsqr import LsqrContext
    from scipy.sparse import linalg
    import scipy.sparse as sp
    rp, ci, vals, rows, cols, b = M.permutation_case()
    A = sp.csr_matrix((vals, ci, rp), shape=(rows, cols))
    want = A.T @ b
    with LsqrContext((rp, ci, vals, cols)) as ctx:
        for kw in ({}, dict(ZERO)):
            ref = linalg.lsmr(A, b, **kw)
            assert (ref[1], ref[2]) == (1, 1) and np.array_equal(ref[0], want)   # SciPy's result
            assert ref[3:] == (0, 0, 1, 1, 16)
            x, r = ctx.solve_lsmr(b, **kw)
            assert np.array_equal(x, want)
            assert r == dict(istop=1, itn=1, normr=0.0, normar=0.0, norma=1.0, conda=1.0,
                             normx=16.0), r


# ---------------------------------------------------------------------------
# C: fixed iteration counts
# ---------------------------------------------------------------------------
def check_against(x, r, ref, bound, tag):
    refn = M.norms_of(ref)
    err = M.rel_max(x, ref[0])
    lines = [f"x {err:.2e}"]
    for key in M.NORM_KEYS:
        d = abs(r[key] - refn[key]) / max(abs(refn[key]), 1e-300)
        lines.append(f"{key} {d:.2e}")
    print(f"{tag}: bound {bound:.2e}; device " + ", ".join(lines), flush=True)
    assert (r["istop"], r["itn"]) == (refn["istop"], refn["itn"]), (r, refn)
    assert err <= bound, (tag, err, bound)
    assert M.norm_error(r, refn) <= bound, (tag, r, refn)


@pytest.mark.parametrize("name,maxiter,variant", M.FIXED_CASES,
                         ids=[f"{n}-it{i}-{'damp_x0' if v else 'plain'}" for n, i, v in M.FIXED_CASES])
def test_fixed_iterations(gpu, ctxs, name, maxiter, variant):
    ref, bound, xerrs, nerrs = M.fixed_reference(name, maxiter, variant)
    b, damp, x0 = M.fixed_inputs(name, variant)
    x, r = ctxs(name).solve_lsmr(b, damp=damp, maxiter=maxiter, x0=x0, **ZERO)
    check_against(x, r, ref, bound, f"{name} it={maxiter} v{variant} scipy x {max(xerrs):.1e} "
                                    f"norms {max(nerrs):.1e}")


# ---------------------------------------------------------------------------
# D: stop rule
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,setting", M.STOP_CASES, ids=[f"{n}-{s}" for n, s in M.STOP_CASES])
def test_stop_rule(gpu, ctxs, name, setting):
    b, kw, ref, margins = M.stop_reference(name, setting)
    ctx = ctxs(name)
    x, r = ctx.solve_lsmr(b, **kw)
    print(f"{name} {setting}: scipy {(ref[1], ref[2])} margins {margins} device "
          f"{(r['istop'], r['itn'])}", flush=True)
    assert (r["istop"], r["itn"]) == (ref[1], ref[2])
    # a stop changes no arithmetic: the fixed-count run at that itn
    xf, rf = ctx.solve_lsmr(b, damp=kw.get("damp", 0.0), maxiter=ref[2], **ZERO)
    assert rf["itn"] == ref[2]
    assert np.array_equal(x, xf)
    assert all(r[k] == rf[k] for k in M.NORM_KEYS), (r, rf)
    check_against(x, r, ref, M.stop_bound(name, setting), f"{name} {setting}")


# ---------------------------------------------------------------------------
# E: interleaving with LSQR, value paths, gather paths
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["zoo", "dense_col_2500x6"])
def test_lsqr_and_lsmr_alternate_on_one_context(gpu, ctxs, name):
    case = M.case_by_name(name)
    b, x0 = L.gaussian_rhs(case, 41)
    b2, _ = L.gaussian_rhs(case, 42)
    kq = dict(damp=0.25, iter_lim=6, x0=x0, **ZERO)
    km = dict(damp=0.25, maxiter=6, x0=x0, **ZERO)
    with ctx_of(case) as fresh:
        want_q = fresh.solve(b, **kq)        # LSQR before any LSMR solve
    with ctx_of(case) as fresh:
        want_m = fresh.solve_lsmr(b, **km)   # LSMR as a context's first solve
    ctx = ctxs(name)
    same(ctx.solve(b, **kq), want_q)
    same(ctx.solve_lsmr(b, **km), want_m)
    same(ctx.solve(b, **kq), want_q)
    ctx.solve_lsmr(b2, maxiter=4)
    same(ctx.solve_lsmr(b, **km), want_m)
    ctx.solve(b2, iter_lim=4)
    same(ctx.solve_lsmr(b, **km), want_m)
    same(ctx.solve(b, **kq), want_q)
    ctx.set_gather_path(1)
    try:
        same(ctx.solve_lsmr(b, **km), want_m)
    finally:
        ctx.set_gather_path(0)


@pytest.mark.parametrize("name", ["zoo", "dense_col_2500x6"])
def test_value_paths(gpu, name):
    case = M.case_by_name(name)
    rng = np.random.default_rng(51)
    b, _ = L.gaussian_rhs(case, 43)
    v2 = rng.standard_normal(len(case.vals))
    kw = dict(maxiter=4, **ZERO)
    with ctx_of(case, vals=v2) as c2:
        want = c2.solve_lsmr(b, **kw)
    table = rng.standard_normal(97)
    index = rng.integers(-1, 97, len(case.vals))
    gathered = np.where(index < 0, 1.0, table[np.maximum(index, 0)])
    with ctx_of(case) as c1:
        c1.set_values(v2)
        same(c1.solve_lsmr(b, **kw), want)
        c1.set_values(gathered)
        wg = c1.solve_lsmr(b, **kw)
        c1.set_values(v2)
        c1.set_value_map(index)
        c1.set_values_from_table(table)
        same(c1.solve_lsmr(b, **kw), wg)
    with ctx_of(case, vals=gathered) as c3:
        same(c3.solve_lsmr(b, **kw), wg)


# ---------------------------------------------------------------------------
# F: lsmr(), als_lsmr
# ---------------------------------------------------------------------------
def test_lsmr_function_matches_scipy_tuple(gpu):
    from movie_recommender_amd.lsmr import lsmr
    from scipy.sparse import linalg
    case = M.case_by_name("dup_unsorted_40x9")
    A = L.csr_of(case)
    b, x0 = L.gaussian_rhs(case, 44)
    ref, bound, _, _ = M.reference_bound(A, b, 0.5, x0, 5)
    got = lsmr(A, b, damp=0.5, x0=x0, maxiter=5, **ZERO)
    assert len(got) == 8 and (got[1], got[2]) == (7, 5)
    assert M.rel_max(got[0], ref[0]) <= bound
    assert M.norm_error(M.norms_of(got), M.norms_of(ref)) <= bound
    # maxiter=None is min(m, n) = 9.  SciPy's defaults stop there with istop 2
    # in three row orders (test2 5.4e-18 against 6.3e-6 the iteration before;
    # normar itself is rounding noise by then, so only x is compared), under
    # 20 x SciPy's own error against longdouble
    refs = M.scipy_orders(A, b, damp=0.5, x0=x0)
    assert {(r[1], r[2]) for r in refs} == {(2, 9)}
    xl = M.lsmr_longdouble(A, b, 0.5, x0, 9)[0]
    bound = max(1e-13, 20 * max(M.rel_max(r[0].astype(np.longdouble), xl) for r in refs))
    got = lsmr(A, b, damp=0.5, x0=x0)
    assert (got[1], got[2]) == (2, 9)
    assert M.rel_max(got[0], refs[0][0]) <= bound
    with ctx_of(case) as ctx:
        x, r = ctx.solve_lsmr(b, damp=0.5, x0=x0, maxiter=9)
    assert np.array_equal(got[0], x) and got[1:] == tuple(r[k] for k in ("istop", "itn") + M.NORM_KEYS)


ALS_FIXTURES = [(40, 45, 3), (120, 90, 10)]
ALS_ITERATIONS = 4


@pytest.mark.parametrize("nu,ni,k", ALS_FIXTURES, ids=[f"{a}x{b}_k{c}" for a, b, c in ALS_FIXTURES])
def test_als_lsmr_follows_the_cpu_path(gpu, nu, ni, k):
    """Bound per iteration: 20 x the CPU path's own largest relative deviation
    among three orders of the rating list (measured: 1.9e-15 at 40x45 k=3,
    2.6e-15 at 120x90 k=10; LSQR's on the same fixtures: 1.4e-15, 2.4e-15),
    1e-13 per chained solve at the least."""
    from movie_recommender_amd import synth
    from movie_recommender_amd.lsmr import als_lsmr
    uid, iid, r = (np.asarray(a) for a in synth.dense_fixture(nu, ni, k)[:3])
    uid, iid, r = uid.astype(np.int64), iid.astype(np.int64), r.astype(np.float64)
    movies0 = np.random.default_rng(100 + k).uniform(-1, 1, ni * k)
    ref, bounds, dev = M.als_bound_lsmr(uid, iid, r, k, nu, ni, movies0, ALS_ITERATIONS)
    errs = [it["error"] for it in ref]
    for a, c in zip(errs, errs[1:]):      # the 1 % rule is not on its threshold
        assert abs(c / a - 0.99) > 1e-6
    seen = []
    users, movies, iterations, errors = als_lsmr(uid, iid, r, k, nu, ni, movies0=movies0,
                                                 max_iterations=ALS_ITERATIONS,
                                                 callback=seen.append)
    n_ref = next((i + 1 for i in range(1, len(errs)) if errs[i] > 0.99 * errs[i - 1]),
                 ALS_ITERATIONS)
    assert iterations == len(seen) == len(errors) == n_ref
    print(f"{nu}x{ni} k={k}: CPU deviation over orders {dev:.2e}")
    for i, (got, want) in enumerate(zip(seen, ref)):
        eu, em = M.rel_max(got["users"], want["users"]), M.rel_max(got["movies"], want["movies"])
        ee = abs(got["error"] - want["error"]) / want["error"]
        print(f"  iteration {i}: users {eu:.2e} movies {em:.2e} error {ee:.2e} "
              f"bound {bounds[i]:.2e}", flush=True)
        assert (got["user_solve"]["istop"], got["user_solve"]["itn"]) == want["user_solve"]
        assert (got["item_solve"]["istop"], got["item_solve"]["itn"]) == want["item_solve"]
        assert eu <= bounds[i] and em <= bounds[i]
        assert ee <= bounds[i]
        assert errors[i] == got["error"]
    assert np.array_equal(users, seen[-1]["users"]) and np.array_equal(movies, seen[-1]["movies"])
