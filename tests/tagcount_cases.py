"""Shared helpers for the tag-count model tests: the golden fixture's loader, a
NumPy restatement of the model written from its description (profiles, rows,
the two minimum-norm solves with the rank rule, scores in the defined order),
and the acceptance rules both the restatement and the GPU are held to.

The restatement never calls ``lstsq``: it takes ``numpy.linalg.qr`` of A and
the SVD of the small R.  Top-N, agreement counts and the spread rule are those
of ``content_cases``.
"""
import numpy as np

import content_cases as C
from conftest import load_golden

EPS = float(np.finfo(np.float64).eps)
FIT_THRESHOLD = 0.1          # a row enters A0 when tag_dot > 0.1
PREDICT_THRESHOLD = 1e-6     # model 0 scores unless tag_product < 1e-6


# --------------------------------------------------------------------------
# fixture
# --------------------------------------------------------------------------
_CACHE = {}


def movie_data():
    """The movie side: content_small.npz's dictionaries plus genre_counts
    (movies per genre).  Treat as read-only."""
    cf = C.fixture()
    gc = {}
    for m in cf["movie_genres"]:
        for g in cf["movie_genres"][m]:
            gc[g] = gc.get(g, 0) + 1
    return dict(movie_genres=cf["movie_genres"], movie_tags=cf["movie_tags"],
                tag_counts=cf["tag_counts"], genre_counts=gc, med=cf["med"],
                med_keys=cf["med_keys"], med_vals=cf["med_vals"])


def _ragged(off, *cols):
    return [tuple(c[off[i]:off[i + 1]] for c in cols) for i in range(len(off) - 1)]


def fixture():
    """tagcount_small.npz decoded once per session (treat as read-only)."""
    if _CACHE:
        return _CACHE
    d = load_golden("tagcount_small.npz")
    d.update(movie_data())
    assert d["genre_counts"] == {int(g): int(c) for g, c in zip(d["gc_gid"], d["gc_cnt"])}
    d["lists"] = [[(int(m), float(r)) for m, r in zip(ms, rs)]
                  for ms, rs in _ragged(d["l_off"], d["l_mid"], d["l_r"])]
    d["t_lists"] = [[(int(m), float(r)) for m, r in zip(ms, rs)]
                    for ms, rs in _ragged(d["t_off"], d["t_mid"], d["t_r"])]
    d["names"] = [str(s) for s in d["l_name"]]
    # the reference's profiles, keys in insertion order, zero members included
    d["tag_profiles"] = [{int(t): float(v) for t, v in zip(ts, vs)}
                         for ts, vs in _ragged(d["tp_off"], d["tp_tid"], d["tp_val"])]
    d["genre_profiles"] = [{int(g): float(v) for g, v in zip(gs, vs)}
                           for gs, vs in _ragged(d["gp_off"], d["gp_gid"], d["gp_val"])]
    d["rows"] = _ragged(d["l_off"], d["row_td"], d["row_gd"])
    d["recs"] = [[(float(s), int(m)) for s, m in zip(sc, ms)]
                 for sc, ms in _ragged(d["rec_off"], d["rec_score"], d["rec_mid"])]
    d["ref_models"] = [(d["tag_profiles"][u], d["genre_profiles"][u],
                        d["x0_ref"][u] if d["has0"][u] else None,
                        d["x1_ref"][u] if d["has1"][u] else None)
                       for u in range(len(d["lists"]))]
    d["genre_names"] = {f"genre{int(g)}": int(g) for g in d["gc_gid"]}
    d["tag_names"] = {f"tag{int(t)}": int(t) for t in d["tag_counts"]}
    _CACHE.update(d)
    return _CACHE


# --------------------------------------------------------------------------
# restatement: profiles, rows, fit
# --------------------------------------------------------------------------
def profiles_of(lst, d):
    """(tag_profile, genre_profile): dicts in insertion order."""
    tags, genres = d["movie_tags"], d["movie_genres"]
    tp, gp = {}, {}
    for m, r in lst:
        offset = r - 3
        if offset == 0:
            continue
        for t, v in tags.get(m, {}).items():
            tp[t] = tp.get(t, 0) + offset * v
        for g in genres.get(m, ()):
            gp[g] = gp.get(g, 0) + offset
    for t in tp:
        tp[t] = tp[t] / d["tag_counts"][t]
    for g in gp:
        gp[g] = gp[g] / d["genre_counts"][g]
    return tp, gp


def dots_of(m, tp, gp, d):
    """(tag_dot, genre_dot) of movie m: the movie's entries in their own order."""
    td = 0
    for t, v in d["movie_tags"].get(m, {}).items():
        if t in tp:
            td += tp[t] * v
    gd = 0
    for g in d["movie_genres"].get(m, ()):
        if g in gp:
            gd += gp[g]
    return td, gd


def min_norm_solve(A, b):
    """Minimum-norm least squares by QR, then the SVD of R; singular values <=
    eps max(rows, cols) s_max are zero.  Returns (x, rank, singular values)."""
    A, b = np.asarray(A, np.float64), np.asarray(b, np.float64)
    Q, R = np.linalg.qr(A)
    U, s, Vt = np.linalg.svd(R)
    keep = s > EPS * max(A.shape) * s[0]
    c = U.T @ (Q.T @ b)
    return Vt.T[:, keep] @ (c[keep] / s[keep]), int(keep.sum()), s


class CpuModel:
    """The restatement's fit of one list."""

    def __init__(self, lst, d):
        self.tag_profile, self.genre_profile = profiles_of(lst, d)
        self.rows = [dots_of(m, self.tag_profile, self.genre_profile, d) for m, _ in lst]
        b = [r - d["med"][m] for m, r in lst]
        A0 = [[td, gd, 1.0] for td, gd in self.rows if td > FIT_THRESHOLD]
        b0 = [bi for bi, (td, _) in zip(b, self.rows) if td > FIT_THRESHOLD]
        self.n0 = len(A0)
        self.x0 = self.x1 = None
        self.rank0 = self.rank1 = 0
        if len(A0) >= 3:
            self.x0, self.rank0, self.s0 = min_norm_solve(A0, b0)
        if len(lst) >= 2:
            self.x1, self.rank1, self.s1 = min_norm_solve([[gd, 1.0] for _, gd in self.rows], b)


# --------------------------------------------------------------------------
# restatement: scores in the defined order
# --------------------------------------------------------------------------
def exact_scores(model, d):
    """(scores, bound, key) over the candidates in movie_medians order for a
    model (tag_profile, genre_profile, x0 or None, x1 or None).  bound is
    (terms + 1) 2^-52 sum |terms| (0 without a model: the median itself); key
    identifies what the score is a function of (equal keys tie everywhere)."""
    tp, gp, x0, x1 = model
    x0 = None if x0 is None else [float(v) for v in np.asarray(x0).reshape(-1)]
    x1 = None if x1 is None else [float(v) for v in np.asarray(x1).reshape(-1)]
    out, bound, keys = [], [], []
    for m in d["med_keys"]:
        m = int(m)
        med = d["med"][m]
        t, g = dots_of(m, tp, gp, d)
        if not (t < PREDICT_THRESHOLD or x0 is None):
            terms = [t * x0[0], g * x0[1], x0[2], med]
            keys.append((0, t, g, med))
        elif x1 is not None:
            terms = [g * x1[0], x1[1], med]
            keys.append((1, g, med))
        else:
            out.append(med)
            bound.append(0.0)
            keys.append((2, med))
            continue
        s = 0.0
        for v in terms:
            s += v
        out.append(s)
        bound.append((len(terms) + 1) * 2.0 ** -52 * sum(abs(v) for v in terms))
    return np.array(out), np.array(bound), keys


def spread_report(errs, spreads):
    rep = {}
    C.check_fixed_iteration(errs, spreads, rep)
    return rep
