"""Cases and CPU restatements for the sparse LSMR (``mr_lsqr_solve_lsmr``,
``movie_recommender_amd.lsmr``), on the matrices and right-hand sides of
tests/cgls_cases.py and tests/lsqr_cases.py.  No GPU and no product import
here: everything is NumPy / SciPy on the CPU.

Exact setup.  ``lsqr_cases.exact_setup``: beta = 2^m, alpha = sqrt(S) / 2^m,
so normr = 2^m, normar = alpha beta = sqrt(S), normA = sqrt(alpha alpha)
(SciPy takes the sqrt; it is not always alpha to the bit), condA = 1, normx = 0.

Fixed iteration counts.  ``lsmr_recurrence`` restates SciPy's lsmr.py loop in
a dtype; ``reference_bound`` takes 20 x SciPy's own largest relative error
against the np.longdouble restatement over three row orders, 1e-13 at the
least (the rule of ``lsqr_cases.reference_bound``), the error taken over x and
over the five returned norms and the larger used for both: SciPy's LSMR norms
deviate from longdouble by more than its x on some cases.

Stop rule.  ``admit`` asserts SciPy's (istop, itn) agreed over three row
orders and equal to the fp64 restatement's, istop in (1, 2, 3), and the
deciding ratio <= 1 / 1.001 at the stop and >= 1.001 the iteration before.
"""
import functools

import numpy as np
import scipy.sparse as sp
from scipy.sparse import linalg

import lsqr_cases as L
from lsqr_cases import (_sym_ortho, case_by_name, csr_of, design_movies, design_users,  # noqa: F401
                        exact_setup, fixed_inputs, permutation_case, rel_max, row_orders, stop_rhs)

NORM_KEYS = ("normr", "normar", "norma", "conda", "normx")


def lsmr_recurrence(A, b, damp, x0, maxiter, dtype, atol=0.0, btol=0.0, conlim=0.0, stop=False):
    """SciPy's lsmr (lsmr.py:237-449) in `dtype`.  stop=False: exactly maxiter
    iterations, no test.  Returns (x, dict of norms / istop / itn, trace) with
    trace[i] = (test1, rtol, test2, test3, istop) of iteration i + 1."""
    T = dtype
    one = T(1)
    A = sp.csr_matrix((A.data.astype(T), A.indices, A.indptr), shape=A.shape)
    At = A.T.tocsr()
    b = np.asarray(b).astype(T)
    nrm = lambda v: np.sqrt(np.sum(v * v)) if T is np.longdouble else np.linalg.norm(v)
    damp = T(damp)
    ctol = one / T(conlim) if conlim > 0 else T(0)
    atol, btol = T(atol), T(btol)
    u = b
    normb = nrm(b)
    if x0 is None:
        x = np.zeros(A.shape[1], T)
        beta = normb
    else:
        x = np.asarray(x0).astype(T)
        u = u - A @ x
        beta = nrm(u)
    if beta > 0:
        u = (one / beta) * u
        v = At @ u
        alpha = nrm(v)
    else:
        v = np.zeros(A.shape[1], T)
        alpha = T(0)
    if alpha > 0:
        v = (one / alpha) * v
    itn = istop = 0
    zetabar = alpha * beta
    alphabar = alpha
    rho = rhobar = cbar = one
    sbar = T(0)
    h = v.copy()
    hbar = np.zeros(A.shape[1], T)
    betadd = beta
    betad = T(0)
    rhodold = one
    tautildeold = thetatilde = zeta = d = T(0)
    normA2 = alpha * alpha
    maxrbar = T(0)
    minrbar = T(1e+100)
    normA = np.sqrt(normA2)
    condA = one
    normx = T(0)
    normr = beta
    normar = alpha * beta
    trace = []

    def result():
        return x, dict(istop=istop, itn=itn, normr=normr, normar=normar, norma=normA,
                       conda=condA, normx=normx), trace
    if normar == 0:
        return result()
    if normb == 0:
        x[()] = 0
        return result()
    while itn < maxiter:
        itn += 1
        u = A @ v - alpha * u
        beta = nrm(u)
        if beta > 0:
            u = (one / beta) * u
            v = At @ u - beta * v
            alpha = nrm(v)
            if alpha > 0:
                v = (one / alpha) * v
        chat, shat, alphahat = _sym_ortho(alphabar, damp, one)
        rhoold = rho
        c, s, rho = _sym_ortho(alphahat, beta, one)
        thetanew = s * alpha
        alphabar = c * alpha
        rhobarold = rhobar
        zetaold = zeta
        thetabar = sbar * rho
        rhotemp = cbar * rho
        cbar, sbar, rhobar = _sym_ortho(cbar * rho, thetanew, one)
        zeta = cbar * zetabar
        zetabar = -sbar * zetabar
        hbar = hbar * (-(thetabar * rho / (rhoold * rhobarold))) + h
        x = x + (zeta / (rho * rhobar)) * hbar
        h = h * (-(thetanew / rho)) + v
        betaacute = chat * betadd
        betacheck = -shat * betadd
        betahat = c * betaacute
        betadd = -s * betaacute
        thetatildeold = thetatilde
        ctildeold, stildeold, rhotildeold = _sym_ortho(rhodold, thetabar, one)
        thetatilde = stildeold * rhobar
        rhodold = ctildeold * rhobar
        betad = -stildeold * betad + ctildeold * betahat
        tautildeold = (zetaold - thetatildeold * tautildeold) / rhotildeold
        taud = (zeta - thetatilde * tautildeold) / rhodold
        d = d + betacheck * betacheck
        bt = betad - taud
        normr = np.sqrt(d + bt * bt + betadd * betadd)
        normA2 = normA2 + beta * beta
        normA = np.sqrt(normA2)
        normA2 = normA2 + alpha * alpha
        maxrbar = max(maxrbar, rhobarold)
        if itn > 1:
            minrbar = min(minrbar, rhobarold)
        condA = max(maxrbar, rhotemp) / min(minrbar, rhotemp)
        normar = abs(zetabar)
        normx = nrm(x)
        test1 = normr / normb
        test2 = normar / (normA * normr) if (normA * normr) != 0 else T(np.inf)
        test3 = one / condA
        t1 = test1 / (one + normA * normx / normb)
        rtol = btol + atol * normA * normx / normb
        istop = 0
        if itn >= maxiter:
            istop = 7
        if one + test3 <= one:
            istop = 6
        if one + test2 <= one:
            istop = 5
        if one + t1 <= one:
            istop = 4
        if test3 <= ctol:
            istop = 3
        if test2 <= atol:
            istop = 2
        if test1 <= rtol:
            istop = 1
        trace.append((float(test1), float(rtol), float(test2), float(test3), istop))
        if stop and istop != 0:
            break
        if not stop:
            istop = 7 if itn >= maxiter else 0
    return result()


def lsmr_longdouble(A, b, damp, x0, maxiter):
    return lsmr_recurrence(A, b, damp, x0, maxiter, np.longdouble)


def scipy_orders(A, b, **kw):
    """SciPy's lsmr on the rows as given, permuted and reversed."""
    return [linalg.lsmr(A[o].tocsr(), b[o], **kw) for o in row_orders(A.shape[0])]


def norms_of(res):
    """SciPy's 8-tuple as a dict of istop, itn and the five norms."""
    return dict(zip(("istop", "itn") + NORM_KEYS, res[1:8]))


def norm_error(got, want):
    """Largest relative error of the five norms (dicts)."""
    return max(abs(float(got[k]) - float(want[k])) / max(abs(float(want[k])), 1e-300)
               for k in NORM_KEYS)


def reference_bound(A, b, damp, x0, maxiter):
    """(SciPy's result on the rows as given, bound, SciPy's x errors, SciPy's
    norm errors): istop == 7, itn == maxiter is asserted in all three orders;
    the bound is 20 x the larger of the x and the norm errors, 1e-13 at the
    least."""
    xl, nl, _ = lsmr_longdouble(A, b, damp, x0, maxiter)
    res = scipy_orders(A, b, damp=damp, atol=0.0, btol=0.0, conlim=0.0, maxiter=maxiter, x0=x0)
    scale = max(float(np.max(np.abs(xl), initial=0.0)), 1e-300)
    xerrs, nerrs = [], []
    for r in res:
        assert (r[1], r[2]) == (7, maxiter), (r[1], r[2], maxiter)
        xerrs.append(float(np.max(np.abs(r[0].astype(np.longdouble) - xl), initial=0.0)) / scale)
        rn = norms_of(r)
        nerrs.append(max(float(abs(np.longdouble(rn[k]) - nl[k]) / max(abs(nl[k]), 1e-300))
                         for k in NORM_KEYS))
    return res[0], max(1e-13, 20 * max(xerrs + nerrs)), tuple(xerrs), tuple(nerrs)


# ---------------------------------------------------------------------------
# stop rule
# ---------------------------------------------------------------------------
STOP_SETTINGS = {
    "inconsistent": dict(kind="inconsistent", kw={}),
    "consistent": dict(kind="consistent", kw={}),
    "damp": dict(kind="damp", kw=dict(damp=0.5)),
    "tight": dict(kind="tight", kw=dict(atol=1e-12, btol=1e-12)),
    # lsqr_cases' conlim=3.0 never gives istop 3 under LSMR (its condA estimate
    # stays below 2.4 on these matrices): the inconsistent b at two lower limits
    "conlim1.5": dict(kind="inconsistent", kw=dict(conlim=1.5)),
    "conlim1.3": dict(kind="inconsistent", kw=dict(conlim=1.3)),
}
# (case, setting) -> SciPy's (istop, itn), SciPy 1.15
STOP_EXPECTED = {
    ("dense_col_2500x6", "inconsistent"): (2, 4), ("dense_col_2500x6", "consistent"): (1, 5),
    ("dense_col_2500x6", "damp"): (2, 4), ("dense_col_2500x6", "tight"): (2, 6),
    ("full_block_256x8", "inconsistent"): (2, 16), ("full_block_256x8", "consistent"): (1, 16),
    ("full_block_256x8", "damp"): (2, 15), ("full_block_256x8", "tight"): (2, 31),
    ("zoo", "inconsistent"): (2, 29), ("zoo", "consistent"): (1, 36),
    ("zoo", "damp"): (2, 29), ("zoo", "tight"): (2, 70),
    ("dense_col_2500x6", "conlim1.5"): (3, 2), ("zoo", "conlim1.5"): (3, 2),
    ("full_block_256x8", "conlim1.3"): (3, 5),
}
STOP_CASES = list(STOP_EXPECTED)


def stop_rhs_of(case, setting):
    """lsqr_cases.stop_rhs with the LSQR seeds: the consistent b, or the
    Gaussian one (LSQR's "inconsistent")."""
    kind = STOP_SETTINGS[setting]["kind"]
    return stop_rhs(case, "consistent" if kind == "consistent" else "inconsistent")


def admit(A, b, kw, margin=1.001):
    """SciPy's (istop, itn), agreed over three row orders and equal to the
    fp64 restatement's, with the deciding test a factor `margin` inside its
    threshold at the stop and outside it the iteration before."""
    res = scipy_orders(A, b, **kw)
    stops = {(r[1], r[2]) for r in res}
    assert len(stops) == 1, stops
    istop, itn = res[0][1], res[0][2]
    atol, btol = kw.get("atol", 1e-6), kw.get("btol", 1e-6)
    conlim = kw.get("conlim", 1e8)
    _, nr, trace = lsmr_recurrence(A, b, kw.get("damp", 0.0), None, min(A.shape), np.float64,
                                   atol=atol, btol=btol, conlim=conlim, stop=True)
    assert (nr["istop"], nr["itn"]) == (istop, itn), (nr["istop"], nr["itn"], istop, itn)
    assert istop in (1, 2, 3), istop

    def ratio(t):   # deciding quantity / its threshold
        test1, rtol, test2, test3, _ = t
        return {1: test1 / rtol, 2: test2 / atol, 3: test3 * conlim}[istop]
    at = ratio(trace[itn - 1])
    assert at * margin <= 1.0, (istop, itn, at)
    before = None
    if itn >= 2:
        before = ratio(trace[itn - 2])
        assert before >= margin, (istop, itn, before)
        assert trace[itn - 2][4] == 0
    return res[0], (at, before)


# ---------------------------------------------------------------------------
# ALS
# ---------------------------------------------------------------------------
def als_reference_lsmr(uid, iid, r, k, num_users, num_items, movies0, iterations,
                       stop_rule=False, iter_lim=100):
    """``lsqr_cases.als_reference`` with SciPy's lsmr(..., maxiter=iter_lim)."""
    uid, iid = np.asarray(uid, np.int64), np.asarray(iid, np.int64)
    movies = np.asarray(movies0, np.float64).copy()
    out = []
    old = None
    for _ in range(iterations):
        ru = linalg.lsmr(design_users(movies, uid, iid, num_users, k), r, maxiter=iter_lim)
        users = ru[0]
        rhs = r - users[k::k + 1][uid]
        Am = design_movies(users, uid, iid, num_items, k)
        rm = linalg.lsmr(Am, rhs, maxiter=iter_lim)
        movies = rm[0]
        error = float(np.sum(np.abs(rhs - Am @ movies))) / len(r)
        out.append(dict(users=users, movies=movies, error=error, user_solve=(ru[1], ru[2]),
                        item_solve=(rm[1], rm[2])))
        if stop_rule and old is not None and error > 0.99 * old:
            break
        old = error
    return out


def als_bound_lsmr(uid, iid, r, k, num_users, num_items, movies0, iterations):
    """``lsqr_cases.als_bound`` for LSMR: (reference on the list as given,
    per-iteration bounds, the CPU path's spread over three rating orders)."""
    runs = [als_reference_lsmr(uid[o], iid[o], r[o], k, num_users, num_items, movies0, iterations)
            for o in L.als_orders(len(r))]
    base = runs[0]
    dev = 0.0
    for other in runs[1:]:
        for a, c in zip(base, other):
            assert a["user_solve"] == c["user_solve"] and a["item_solve"] == c["item_solve"]
            dev = max(dev, rel_max(c["users"], a["users"]), rel_max(c["movies"], a["movies"]))
    bounds = [max(20 * dev, 1e-13 * 2 * (i + 1)) for i in range(iterations)]
    return base, bounds, dev


# ---------------------------------------------------------------------------
# shared, cached references (computed once per process)
# ---------------------------------------------------------------------------
FIXED_CASES = L.FIXED_CASES


@functools.lru_cache(maxsize=None)
def fixed_reference(name, maxiter, variant):
    b, damp, x0 = fixed_inputs(name, variant)
    return reference_bound(csr_of(case_by_name(name)), b, damp, x0, maxiter)


@functools.lru_cache(maxsize=None)
def stop_reference(name, setting):
    """(b, kwargs, SciPy's result, margins) of a stop case, admitted."""
    case = case_by_name(name)
    b = stop_rhs_of(case, setting)
    kw = dict(STOP_SETTINGS[setting]["kw"])
    res, margins = admit(csr_of(case), b, kw)
    assert (res[1], res[2]) == STOP_EXPECTED[(name, setting)], (name, setting, res[1], res[2])
    return b, kw, res, margins


@functools.lru_cache(maxsize=None)
def stop_bound(name, setting):
    """reference_bound at a stop case's stopping iteration."""
    b, kw, res, _ = stop_reference(name, setting)
    return reference_bound(csr_of(case_by_name(name)), b, kw.get("damp", 0.0), None, res[2])[1]
