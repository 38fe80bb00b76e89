"""Cases and CPU restatements for the general sparse LSQR (``mr_lsqr_*``,
``movie_recommender_amd.lsqr``).  No GPU and no product import here:
everything is NumPy / SciPy on the CPU.

Exact setup (tier A).  On a ``cgls_cases.Case`` (values +-1, x0 from {-1, 0,
1}) take b = A x0 + e with exactly 4^m entries of e equal to +-1: then b - A
x0 = e exactly, beta = 2^m, u = e / 2^m and A^T u are dyadic, and every
summation order gives the same bits while the row sums stay below 2^52 and S
= sum (A^T e)^2 < 2^52 (asserted here); arnorm = alfa beta = sqrt(S).  With
the e drawn here (seed 1) the zoo has m = 5 and S = 15123.

Fixed iteration counts (tier C).  ``lsqr_longdouble`` restates SciPy's
recurrences in np.longdouble with no stopping test; ``reference_bound`` takes
20 x the largest relative max-norm error of SciPy's fp64 lsqr against it over
three row orders (given, permuted, reversed), 1e-13 at the least -- the rule
of ``cgls_cases.tolerance_from_reference``.

Stop rule (tier D).  ``lsqr_recurrence`` restates SciPy's loop in fp64 and records
the three tests per iteration; ``admit`` asserts that the deciding test is a
factor 1.001 inside its threshold where SciPy stops and 1.001 outside it the
iteration before.

ALS (tier F).  ``als_reference`` chains SciPy's lsqr on the two design
matrices as ``oracle/scipy_als.py`` builds them, with the user bias read at
column k (the reference's ``users[3::4]`` is that column at k = 3 only).
"""
import functools

import numpy as np
import scipy.sparse as sp
from scipy.sparse import linalg

import cgls_cases as C

EPS = np.finfo(np.float64).eps
NORM_KEYS = ("r1norm", "r2norm", "anorm", "acond", "arnorm", "xnorm")


# ---------------------------------------------------------------------------
# tier A
# ---------------------------------------------------------------------------
def exact_m(rows):
    m = 0
    while m < 5 and 4 ** (m + 1) <= rows:
        m += 1
    return m


def exact_setup(case, seed=1):
    """(b, x0, e, m, S) of the exact setup on a cgls case; rows >= 1."""
    rng = np.random.default_rng(seed)
    m = exact_m(case.rows)
    e = np.zeros(case.rows)
    pos = rng.choice(case.rows, 4 ** m, replace=False)
    e[pos] = rng.integers(0, 2, 4 ** m) * 2.0 - 1.0
    A, At = case.A, case.At
    xi, ei = case.x0.astype(np.int64), e.astype(np.int64)
    if case.cols:
        assert float(np.max(abs(A).astype(np.float64) @ np.abs(case.x0), initial=0.0)) + 1 < 2.0 ** 52
        assert float(np.max(abs(At).astype(np.float64) @ np.abs(e), initial=0.0)) < 2.0 ** 52
    ax = A @ xi
    g = At @ ei
    gf = g.astype(np.float64)
    assert float(np.sum(gf * gf)) < 2.0 ** 51
    S = int(np.sum(g * g))
    assert S < 2 ** 52
    b = (ax + ei).astype(np.float64)
    return b, case.x0.copy(), e, m, S


def csr_of(case, vals=None):
    v = case.vals if vals is None else vals
    return sp.csr_matrix((np.asarray(v, np.float64), case.ci.astype(np.int64),
                          case.rp.astype(np.int64)), shape=(case.rows, case.cols))


# ---------------------------------------------------------------------------
# tier B
# ---------------------------------------------------------------------------
def permutation_case(seed=3):
    """(rp, ci, vals, rows, cols, b): a signed permutation of 300 with 5 empty
    rows and 7 empty columns appended; b holds 256 entries +-1 on the
    permutation's rows.  beta = 16, alfa = 1, and iteration 1 gives
    uh = A v - alfa u = 0 exactly."""
    rng = np.random.default_rng(seed)
    n = 300
    perm = rng.permutation(n)
    vals = rng.integers(0, 2, n) * 2.0 - 1.0
    rp = np.concatenate([np.arange(n + 1), np.full(5, n)]).astype(np.int32)
    b = np.zeros(n + 5)
    pos = rng.choice(n, 256, replace=False)
    b[pos] = rng.integers(0, 2, 256) * 2.0 - 1.0
    return rp, perm.astype(np.int32), vals, n + 5, n + 7, b


# ---------------------------------------------------------------------------
# tier C
# ---------------------------------------------------------------------------
def _sym_ortho(a, b, one):
    if b == 0:
        return np.sign(a), 0 * one, abs(a)
    if a == 0:
        return 0 * one, np.sign(b), abs(b)
    if abs(b) > abs(a):
        tau = a / b
        s = np.sign(b) / np.sqrt(one + tau * tau)
        return s * tau, s, b / s
    tau = b / a
    c = np.sign(a) / np.sqrt(one + tau * tau)
    return c, c * tau, a / c


def lsqr_recurrence(A, b, damp, x0, iter_lim, dtype, atol=0.0, btol=0.0, conlim=0.0,
                    stop=False):
    """SciPy's lsqr (lsqr.py:355-589) in `dtype`.  stop=False: exactly
    iter_lim iterations, no test.  Returns (x, dict of norms / istop / itn,
    trace) with trace[i] = (test1, rtol, test2, test3, istop) of iteration
    i + 1."""
    T = dtype
    one = T(1)
    A = sp.csr_matrix((A.data.astype(T), A.indices, A.indptr), shape=A.shape)
    At = A.T.tocsr()
    b = np.asarray(b).astype(T)
    nrm = lambda v: np.sqrt(np.sum(v * v)) if T is np.longdouble else np.linalg.norm(v)
    damp = T(damp)
    dampsq = damp * damp
    ctol = T(1) / T(conlim) if conlim > 0 else T(0)
    eps = T(EPS)
    anorm = acond = ddnorm = res2 = xnorm = xxnorm = z = sn2 = T(0)
    cs2 = -one
    itn = istop = 0
    u = b
    bnorm = nrm(b)
    if x0 is None:
        x = np.zeros(A.shape[1], T)
        beta = bnorm
    else:
        x = np.asarray(x0).astype(T)
        u = u - A @ x
        beta = nrm(u)
    if beta > 0:
        u = (one / beta) * u
        v = At @ u
        alfa = nrm(v)
    else:
        v = x.copy()
        alfa = T(0)
    if alfa > 0:
        v = (one / alfa) * v
    w = v.copy()
    rhobar, phibar = alfa, beta
    rnorm = r1norm = r2norm = beta
    arnorm = alfa * beta
    trace = []

    def result():
        return x, dict(istop=istop, itn=itn, r1norm=r1norm, r2norm=r2norm, anorm=anorm,
                       acond=acond, arnorm=arnorm, xnorm=xnorm), trace
    if arnorm == 0:
        return result()
    while itn < iter_lim:
        itn += 1
        u = A @ v - alfa * u
        beta = nrm(u)
        if beta > 0:
            u = (one / beta) * u
            anorm = np.sqrt(anorm * anorm + alfa * alfa + beta * beta + dampsq)
            v = At @ u - beta * v
            alfa = nrm(v)
            if alfa > 0:
                v = (one / alfa) * v
        if damp > 0:
            rhobar1 = np.sqrt(rhobar * rhobar + dampsq)
            cs1 = rhobar / rhobar1
            sn1 = damp / rhobar1
            psi = sn1 * phibar
            phibar = cs1 * phibar
        else:
            rhobar1 = rhobar
            psi = T(0)
        cs, sn, rho = _sym_ortho(rhobar1, beta, one)
        theta = sn * alfa
        rhobar = -cs * alfa
        phi = cs * phibar
        phibar = sn * phibar
        tau = sn * phi
        t1 = phi / rho
        t2 = -theta / rho
        dk = (one / rho) * w
        x = x + t1 * w
        w = v + t2 * w
        dn = nrm(dk)
        ddnorm = ddnorm + dn * dn
        delta = sn2 * rho
        gambar = -cs2 * rho
        rhs = phi - delta * z
        zbar = rhs / gambar
        xnorm = np.sqrt(xxnorm + zbar * zbar)
        gamma = np.sqrt(gambar * gambar + theta * theta)
        cs2 = gambar / gamma
        sn2 = theta / gamma
        z = rhs / gamma
        xxnorm = xxnorm + z * z
        acond = anorm * np.sqrt(ddnorm)
        res1 = phibar * phibar
        res2 = res2 + psi * psi
        rnorm = np.sqrt(res1 + res2)
        arnorm = alfa * abs(tau)
        if damp > 0:
            r1sq = rnorm * rnorm - dampsq * xxnorm
            r1norm = np.sqrt(abs(r1sq))
            if r1sq < 0:
                r1norm = -r1norm
        else:
            r1norm = rnorm
        r2norm = rnorm
        test1 = rnorm / bnorm
        test2 = arnorm / (anorm * rnorm + eps)
        test3 = one / (acond + eps)
        t1 = test1 / (one + anorm * xnorm / bnorm)
        rtol = T(btol) + T(atol) * anorm * xnorm / bnorm
        istop = 0
        if itn >= iter_lim:
            istop = 7
        if one + test3 <= one:
            istop = 6
        if one + test2 <= one:
            istop = 5
        if one + t1 <= one:
            istop = 4
        if test3 <= ctol:
            istop = 3
        if test2 <= T(atol):
            istop = 2
        if test1 <= rtol:
            istop = 1
        trace.append((float(test1), float(rtol), float(test2), float(test3), istop))
        if stop and istop != 0:
            break
        if not stop:
            istop = 7 if itn >= iter_lim else 0
    return result()


def lsqr_longdouble(A, b, damp, x0, iter_lim):
    return lsqr_recurrence(A, b, damp, x0, iter_lim, np.longdouble)


def row_orders(rows, seed=7):
    ident = np.arange(rows)
    return [ident, np.random.default_rng(seed).permutation(rows), ident[::-1]]


def scipy_orders(A, b, **kw):
    """SciPy's lsqr on the rows as given, permuted and reversed."""
    out = []
    for o in row_orders(A.shape[0]):
        out.append(linalg.lsqr(A[o].tocsr(), b[o], **kw))
    return out


def reference_bound(A, b, damp, x0, iter_lim):
    """(SciPy's result on the rows as given, bound, SciPy's errors): the
    condition istop == 7, itn == iter_lim is asserted in all three orders."""
    xl, nl, _ = lsqr_longdouble(A, b, damp, x0, iter_lim)
    res = scipy_orders(A, b, damp=damp, atol=0.0, btol=0.0, conlim=0.0, iter_lim=iter_lim, x0=x0)
    scale = max(float(np.max(np.abs(xl), initial=0.0)), 1e-300)
    errs = []
    for r in res:
        assert (r[1], r[2]) == (7, iter_lim), (r[1], r[2], iter_lim)
        errs.append(float(np.max(np.abs(r[0].astype(np.longdouble) - xl), initial=0.0)) / scale)
    return res[0], max(1e-13, 20 * max(errs)), tuple(errs)


def rel_max(x, ref):
    scale = max(float(np.max(np.abs(ref), initial=0.0)), 1e-300)
    return float(np.max(np.abs(np.asarray(x) - np.asarray(ref)), initial=0.0)) / scale


def gaussian_rhs(case, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(case.rows), rng.standard_normal(case.cols)


# ---------------------------------------------------------------------------
# tier D
# ---------------------------------------------------------------------------
STOP_SETTINGS = {
    "inconsistent": dict(kind="gauss", kw={}),
    "consistent": dict(kind="consistent", kw={}),
    "conlim3": dict(kind="gauss", kw=dict(conlim=3.0)),
    "damp": dict(kind="gauss", kw=dict(damp=0.5)),
    "tight": dict(kind="gauss", kw=dict(atol=1e-12, btol=1e-12)),
}
# (case, setting) -> SciPy's (istop, itn) where the issue lists it
STOP_EXPECTED = {
    ("dense_col_2500x6", "inconsistent"): (2, 4), ("dense_col_2500x6", "consistent"): (1, 5),
    ("full_block_256x8", "inconsistent"): (2, 16), ("full_block_256x8", "consistent"): (1, 16),
    ("full_block_256x8", "tight"): (2, 31),
    ("zoo", "inconsistent"): (2, 31), ("zoo", "consistent"): (1, 35), ("zoo", "conlim3"): (3, 3),
}
STOP_CASES = [(c, s) for c in ("dense_col_2500x6", "full_block_256x8", "zoo")
              for s in ("inconsistent", "consistent", "conlim3", "damp")] + \
             [("full_block_256x8", "tight")]


# the Gaussian b's seed: on the zoo one whose SciPy stop is the listed (2, 31)
# (seeds 3, 5, 6, 7, 9, 10 and 21 stop at 30; the seed is chosen on SciPy alone)
STOP_SEEDS = {"zoo": 1}


def stop_rhs(case, setting):
    consistent = STOP_SETTINGS[setting]["kind"] == "consistent"
    rng = np.random.default_rng(21 if consistent else STOP_SEEDS.get(case.name, 21))
    if STOP_SETTINGS[setting]["kind"] == "consistent":
        return csr_of(case) @ rng.standard_normal(case.cols)
    return rng.standard_normal(case.rows)


def admit(A, b, kw, margin=1.001):
    """SciPy's (istop, itn), agreed over three row orders, with the deciding
    test a factor `margin` inside its threshold at the stop and outside it the
    iteration before (from the fp64 restatement)."""
    res = scipy_orders(A, b, **kw)
    stops = {(r[1], r[2]) for r in res}
    assert len(stops) == 1, stops
    istop, itn = res[0][1], res[0][2]
    atol, btol = kw.get("atol", 1e-6), kw.get("btol", 1e-6)
    conlim = kw.get("conlim", 1e8)
    _, nr, trace = lsqr_recurrence(A, b, kw.get("damp", 0.0), None, 2 * A.shape[1], np.float64,
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
# tier F
# ---------------------------------------------------------------------------
def design_users(movies, uid, iid, num_users, k):
    n = len(uid)
    rows = np.repeat(np.arange(n), k + 1)
    cols = (uid[:, None] * (k + 1) + np.arange(k + 1)[None, :]).ravel()
    data = np.concatenate([movies.reshape(-1, k)[iid], np.ones((n, 1))], axis=1).ravel()
    return sp.coo_matrix((data, (rows, cols)), shape=(n, num_users * (k + 1))).tocsr()


def design_movies(users, uid, iid, num_items, k):
    n = len(uid)
    rows = np.repeat(np.arange(n), k)
    cols = (iid[:, None] * k + np.arange(k)[None, :]).ravel()
    data = users.reshape(-1, k + 1)[uid, :k].ravel()
    return sp.coo_matrix((data, (rows, cols)), shape=(n, num_items * k)).tocsr()


def als_reference(uid, iid, r, k, num_users, num_items, movies0, iterations, stop_rule=False):
    """The reference's loop with SciPy's lsqr; a list of dicts per iteration
    (users, movies, error, user_solve (istop, itn), item_solve).  With
    stop_rule the 1 % rule of fit_to_data ends the loop."""
    uid, iid = np.asarray(uid, np.int64), np.asarray(iid, np.int64)
    movies = np.asarray(movies0, np.float64).copy()
    out = []
    old = None
    for _ in range(iterations):
        ru = linalg.lsqr(design_users(movies, uid, iid, num_users, k), r, iter_lim=100)
        users = ru[0]
        bias = users[k::k + 1]
        rhs = r - bias[uid]
        Am = design_movies(users, uid, iid, num_items, k)
        rm = linalg.lsqr(Am, rhs, iter_lim=100)
        movies = rm[0]
        error = float(np.sum(np.abs(rhs - Am @ movies))) / len(r)
        out.append(dict(users=users, movies=movies, error=error, user_solve=(ru[1], ru[2]),
                        item_solve=(rm[1], rm[2])))
        if stop_rule and old is not None and error > 0.99 * old:
            break
        old = error
    return out


def als_orders(n, seed=9):
    ident = np.arange(n)
    return [ident, np.random.default_rng(seed).permutation(n), ident[::-1]]


def als_bound(uid, iid, r, k, num_users, num_items, movies0, iterations):
    """(reference on the list as given, per-iteration bounds, deviations): 20
    x the reference's largest relative deviation among three orders of the
    rating list, 1e-13 per LSQR solve chained so far at the least.  The
    (istop, itn) of every half-step agree over the orders (asserted)."""
    runs = [als_reference(uid[o], iid[o], r[o], k, num_users, num_items, movies0, iterations)
            for o in als_orders(len(r))]
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
FIXED_ITERS = {"dup_unsorted_40x9": (1, 3), "dense_col_2500x6": (1, 3),
               "full_block_256x8": (1, 3, 30), "zoo": (1, 5, 20)}
FIXED_CASES = [(n, it, var) for n, its in FIXED_ITERS.items() for it in its for var in (0, 1)]


@functools.lru_cache(maxsize=None)
def case_by_name(name):
    if name == "zoo":
        return C.zoo()
    return {c.name: c for c in C.small_cases()}[name]


def fixed_inputs(name, variant):
    """(b, damp, x0) of tier C: Gaussian b; variant 1: damp 0.5, Gaussian x0."""
    case = case_by_name(name)
    b, x0 = gaussian_rhs(case, 31)
    return (b, 0.5, x0) if variant else (b, 0.0, None)


@functools.lru_cache(maxsize=None)
def fixed_reference(name, iter_lim, variant):
    b, damp, x0 = fixed_inputs(name, variant)
    return reference_bound(csr_of(case_by_name(name)), b, damp, x0, iter_lim)


@functools.lru_cache(maxsize=None)
def stop_reference(name, setting):
    """(b, kwargs, SciPy's result, margins) of a tier-D case, admitted."""
    case = case_by_name(name)
    b = stop_rhs(case, setting)
    kw = dict(STOP_SETTINGS[setting]["kw"])
    res, margins = admit(csr_of(case), b, kw)
    if (name, setting) in STOP_EXPECTED:
        assert (res[1], res[2]) == STOP_EXPECTED[(name, setting)], (name, setting, res[1], res[2])
    return b, kw, res, margins


@functools.lru_cache(maxsize=None)
def stop_bound(name, setting):
    """Tier C's bound at a tier-D case's stopping iteration."""
    b, kw, res, _ = stop_reference(name, setting)
    return reference_bound(csr_of(case_by_name(name)), b, kw.get("damp", 0.0), None, res[2])[1]
