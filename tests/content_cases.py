"""Shared helpers for the content-model (tag least squares) tests: the golden
fixture's loader, a NumPy restatement of the model written from its
description (profile, A, LSQR with every stopping test, scores in the defined
order, top-N, agreement), and the acceptance rules both the restatement and
the GPU are held to.

The restatement uses no SciPy and sums in another order than SciPy does: A is
dense, products run over reversed columns / rows through BLAS, norms are
``math.fsum``.
"""
import math

import numpy as np

from conftest import load_golden

MAXF, ROW = 25, 26
EPS = float(np.finfo(np.float64).eps)
FLOOR = 2.0 ** -40          # spread floor of the fixed-iteration rule
FACTOR = 8.0                # ... and its factor over the reference's own spread


# --------------------------------------------------------------------------
# fixture
# --------------------------------------------------------------------------
def _ragged(off, *cols):
    return [tuple(c[off[i]:off[i + 1]] for c in cols) for i in range(len(off) - 1)]


_CACHE = {}


def fixture():
    """content_small.npz decoded once per session (treat as read-only)."""
    if _CACHE:
        return _CACHE
    d = load_golden("content_small.npz")
    d["movie_genres"] = {int(m): set(int(g) for g in gs)
                         for m, (gs,) in zip(d["mg_mid"], _ragged(d["mg_off"], d["mg_gid"]))}
    d["movie_tags"] = {int(m): {int(t): float(v) for t, v in zip(ts, vs)}
                       for m, (ts, vs) in zip(d["mt_mid"],
                                              _ragged(d["mt_off"], d["mt_tid"], d["mt_val"]))}
    d["tag_counts"] = {int(t): int(c) for t, c in zip(d["tc_tid"], d["tc_cnt"])}
    d["med"] = {int(m): float(v) for m, v in zip(d["med_keys"], d["med_vals"])}
    d["lists"] = [[(int(m), float(r)) for m, r in zip(ms, rs)]
                  for ms, rs in _ragged(d["l_off"], d["l_mid"], d["l_r"])]
    d["t_lists"] = [[(int(m), float(r)) for m, r in zip(ms, rs)]
                    for ms, rs in _ragged(d["t_off"], d["t_mid"], d["t_r"])]
    d["names"] = [str(s) for s in d["l_name"]]
    d["profiles"] = [d["profile"][u, :d["p"][u]].tolist() for u in range(len(d["p"]))]
    # traj[u][j - 1] = the reference's x after j iterations, stops disabled
    d["traj"] = [d["traj_x"][a:b].reshape(-1, ROW)
                 for a, b in zip(d["traj_off"][:-1], d["traj_off"][1:])]
    d["recs"] = [[(float(s), int(m)) for s, m in zip(sc, ms)]
                 for sc, ms in _ragged(d["rec_off"], d["rec_score"], d["rec_mid"])]
    _CACHE.update(d)
    return _CACHE


def x_row(xf):
    """(p + 1,) coefficients -> the 26-wide row (zeros past the bias)."""
    out = np.zeros(ROW)
    out[:len(xf)] = np.asarray(xf).reshape(-1)
    return out


# --------------------------------------------------------------------------
# restatement: profile and A
# --------------------------------------------------------------------------
def decide_num_factors(n):
    nf, width, mult = 0, 10, 2
    for _ in range(5):
        if n <= width:
            return nf + n // mult
        nf, n, width, mult = nf + 5, n - width, width * 2, mult * 2
    return nf


def movie_features(m, movie_genres, movie_tags, tag_counts):
    """{feature id: value} of one movie: genres as is with 1.0, tags + 1000."""
    f = {g: 1.0 for g in movie_genres.get(m, ())}
    for t, v in movie_tags.get(m, {}).items():
        f[t + 1000] = v / tag_counts[t]
    return f


def profile_of(lst, movie_genres, movie_tags, tag_counts):
    counts = {}
    for m, _ in lst:
        for f in movie_features(m, movie_genres, movie_tags, tag_counts):
            counts[f] = counts.get(f, 0) + 1
    order = sorted(((c, f) for f, c in counts.items()), reverse=True)
    return [f for _, f in order[:decide_num_factors(len(lst))]]


def system_of(lst, profile, movie_genres, movie_tags, tag_counts, med):
    A = np.zeros((len(lst), len(profile) + 1))
    b = np.zeros(len(lst))
    for i, (m, r) in enumerate(lst):
        f = movie_features(m, movie_genres, movie_tags, tag_counts)
        for j, pid in enumerate(profile):
            A[i, j] = f.get(pid, 0.0)
        A[i, -1] = 1.0
        b[i] = r - med[m]
    return A, b


# --------------------------------------------------------------------------
# restatement: LSQR (Paige & Saunders; damp = 0, x0 = 0)
# --------------------------------------------------------------------------
def _norm(v):
    return math.sqrt(math.fsum(v * v))


def _sym_ortho(a, b):
    if b == 0:
        return float(np.sign(a)), 0.0, abs(a)
    if a == 0:
        return 0.0, float(np.sign(b)), abs(b)
    if abs(b) > abs(a):
        tau = a / b
        s = float(np.sign(b)) / math.sqrt(1 + tau * tau)
        return s * tau, s, b / s
    tau = b / a
    c = float(np.sign(a)) / math.sqrt(1 + tau * tau)
    return c, c * tau, a / c


def lsqr(A, b, atol=1e-6, btol=1e-6, conlim=1e8, iter_lim=1000):
    """Returns (x, istop, itn)."""
    Ar = np.ascontiguousarray(A[:, ::-1])          # products over reversed columns
    Atr = np.ascontiguousarray(A[::-1].T)          # ... and reversed rows
    mv = lambda v: Ar @ v[::-1]                    # noqa: E731
    rmv = lambda u: Atr @ u[::-1]                  # noqa: E731
    n = A.shape[1]
    ctol = 1.0 / conlim if conlim > 0 else 0.0
    anorm = ddnorm = xnorm = xxnorm = z = sn2 = 0.0
    cs2 = -1.0
    x = np.zeros(n)
    bnorm = beta = _norm(b)
    if beta == 0:
        return x, 0, 0
    u = (1 / beta) * b
    v = rmv(u)
    alfa = _norm(v)
    if alfa > 0:
        v = (1 / alfa) * v
    w = v.copy()
    rhobar, phibar = alfa, beta
    if alfa * beta == 0:
        return x, 0, 0
    itn = istop = 0
    while itn < iter_lim:
        itn += 1
        u = mv(v) - alfa * u
        beta = _norm(u)
        if beta > 0:
            u = (1 / beta) * u
            anorm = math.sqrt(anorm ** 2 + alfa ** 2 + beta ** 2)
            v = rmv(u) - beta * v
            alfa = _norm(v)
            if alfa > 0:
                v = (1 / alfa) * v
        cs, sn, rho = _sym_ortho(rhobar, beta)
        theta = sn * alfa
        rhobar = -cs * alfa
        phi = cs * phibar
        phibar = sn * phibar
        tau = sn * phi
        t1, t2 = phi / rho, -theta / rho
        dk = (1 / rho) * w
        x = x + t1 * w
        w = v + t2 * w
        ddnorm += _norm(dk) ** 2
        delta, gambar = sn2 * rho, -cs2 * rho
        rhs = phi - delta * z
        zbar = rhs / gambar
        xnorm = math.sqrt(xxnorm + zbar ** 2)
        gamma = math.sqrt(gambar ** 2 + theta ** 2)
        cs2, sn2, z = gambar / gamma, theta / gamma, rhs / gamma
        xxnorm += z * z
        acond = anorm * math.sqrt(ddnorm)
        rnorm = math.sqrt(phibar ** 2)
        arnorm = alfa * abs(tau)
        test1 = rnorm / bnorm
        test2 = arnorm / (anorm * rnorm + EPS)
        test3 = 1 / (acond + EPS)
        t1 = test1 / (1 + anorm * xnorm / bnorm)
        rtol = btol + atol * anorm * xnorm / bnorm
        if itn >= iter_lim:
            istop = 7
        if 1 + test3 <= 1:
            istop = 6
        if 1 + test2 <= 1:
            istop = 5
        if 1 + t1 <= 1:
            istop = 4
        if test3 <= ctol:
            istop = 3
        if test2 <= atol:
            istop = 2
        if test1 <= rtol:
            istop = 1
        if istop:
            break
    return x, istop, itn


class CpuModel:
    """The restatement's fit of one list: profile, x (p + 1,), itn, istop."""

    def __init__(self, lst, d, **kw):
        g, t, tc, med = d["movie_genres"], d["movie_tags"], d["tag_counts"], d["med"]
        if len(lst) < 2:
            raise ValueError("a rating list needs at least 2 ratings")
        self.profile = profile_of(lst, g, t, tc)
        self.A, self.b = system_of(lst, self.profile, g, t, tc, med)
        self.x, self.istop, self.itn = lsqr(self.A, self.b, **kw)


# --------------------------------------------------------------------------
# restatement: scores, top-N, agreement
# --------------------------------------------------------------------------
def attr_matrix(profile, d):
    """attr[c, j] of every candidate (movie_medians order) for a profile."""
    g, t, tc = d["movie_genres"], d["movie_tags"], d["tag_counts"]
    A = np.zeros((len(d["med_keys"]), len(profile)))
    for c, m in enumerate(d["med_keys"]):
        f = movie_features(int(m), g, t, tc)
        for j, pid in enumerate(profile):
            A[c, j] = f.get(pid, 0.0)
    return A


def exact_scores(profile, x, d, attr=None):
    """s = 0; s += attr_j * x_j (j in profile order); s += bias; s += median."""
    attr = attr_matrix(profile, d) if attr is None else attr
    x = np.asarray(x).reshape(-1)
    s = np.zeros(attr.shape[0])
    for j in range(len(profile)):
        s = s + attr[:, j] * x[j]
    s = s + x[len(profile)]
    return s + d["med_vals"]


def score_bound(profile, x, d, attr=None):
    """(p + 3) 2^-52 (sum_j |attr_j x_j| + |bias| + |median|): any two
    summation orders of the same terms differ by less."""
    attr = attr_matrix(profile, d) if attr is None else attr
    x = np.asarray(x).reshape(-1)
    p = len(profile)
    mag = np.abs(attr * x[None, :p]).sum(axis=1) + abs(x[p]) + np.abs(d["med_vals"])
    return (p + 3) * 2.0 ** -52 * mag


def exact_top_n(scores, mids, excluded, n):
    order = np.lexsort((-mids.astype(np.int64), -scores))
    out = []
    for c in order:
        if int(mids[c]) in excluded:
            continue
        out.append((float(scores[c]), int(mids[c])))
        if len(out) >= n:
            break
    return out


def agreement_counts(actual, pred):
    """Pairs with actual_i > actual_j: (agree when pred_i > pred_j, else
    disagree), over entries with a prediction; agreement None as the
    reference returns it."""
    keep = ~np.isnan(pred)
    a, p = np.asarray(actual)[keep], np.asarray(pred)[keep]
    gt = a[:, None] > a[None, :]
    agree = int(np.sum(gt & (p[:, None] > p[None, :])))
    total = int(np.sum(gt))
    val = agree / total if (len(a) > 1 and total > 0) else None
    return val, agree, total - agree


# --------------------------------------------------------------------------
# acceptance rules (the same for the restatement and the GPU)
# --------------------------------------------------------------------------
def rel_inf(x, xref):
    x, xref = np.asarray(x).reshape(-1), np.asarray(xref).reshape(-1)
    return float(np.max(np.abs(x - xref)) / max(1.0, float(np.max(np.abs(xref)))))


def check_fixed_iteration(errs, spreads, report=None):
    """e_u <= 8 max(s_u, 2^-40) for all but at most 1 list in 10, and no
    e_u above 8 max_u s_u."""
    errs, spreads = np.asarray(errs), np.asarray(spreads)
    bound = FACTOR * np.maximum(spreads, FLOOR)
    over = errs > bound
    cap = FACTOR * max(float(spreads.max()), FLOOR)
    if report is not None:
        report["worst_ratio"] = float(np.max(errs / np.maximum(spreads, FLOOR)))
        report["over"] = int(over.sum())
    assert over.sum() <= len(errs) // 10, (np.nonzero(over)[0], errs[over], bound[over])
    assert errs.max() <= cap, (errs.max(), cap)


def check_stop(itn, istop, d):
    """On stable lists itn / istop equal the reference's but for at most 1 in
    8; every itn lies inside the recorded trajectory."""
    stable = d["stable"].astype(bool)
    miss = stable & ((np.asarray(itn) != d["itn_ref"]) | (np.asarray(istop) != d["istop_ref"]))
    assert miss.sum() <= stable.sum() // 8, (np.nonzero(miss)[0], stable.sum())
    for u, n in enumerate(itn):
        assert 0 <= n <= len(d["traj"][u]), (u, n)
