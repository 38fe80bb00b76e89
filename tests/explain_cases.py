"""Explanations (include/mr_explain.h) restated in NumPy, and the fixture of
test_gpu_explain.py.

Fixture, per k from default_rng(1200 + k) -- the recipe of
test_gpu_foldin.py, restated here: a 300-row table, uniform(-1, 1) rounded
through fp32 (|.| of it for the non-negative variant), rows 294 .. 299 zero,
row offsets in {0.25, ..., 2.5}; lists of 0, 1, 2, k - 1, k + 3, 200 and 290
distinct rows with r in {0.5, ..., 5}, and one list of the six zero rows.
k: 1, 5, 20; 67 / 68 straddle the one-pass / two-pass triangle of the build;
128 with the intercept is the LDS maximum K = 129.  Forms: explicit with
intercept and offsets, explicit without either, implicit at alpha = 8.

Targets of an entity: the first row of its own list, the zero row 299, then
rows drawn from default_rng(77 + k).  Target counts Q come from {0, 1, 3, 16,
17, 40}: the kernel solves 16 targets at a time, so 16 / 17 sit on the tile
edge and 40 takes three passes.
"""
import functools

import numpy as np

NI = 300
KS = [1, 5, 20, 67, 68, 128]
FORMS = ["explicit_icpt", "explicit", "implicit"]
REGS = [(0.5, "constant"), (0.05, "weighted")]
ALPHA = 8.0
EPS = np.finfo(np.float64).eps
TILE = 16
QS = [3, 16, 0, 17, 1, 40, 16, 17]   # entity e asks about QS[e] targets
COND_MAX = 1e5


def fixture(k, nonneg_table):
    rng = np.random.default_rng(1200 + k)
    T = rng.uniform(-1, 1, (NI, k)).astype(np.float32).astype(np.float64)
    if nonneg_table: T = np.abs(T)
    T[294:] = 0.0
    offs = rng.integers(1, 11, NI) * 0.25
    lists = []
    for M in sorted(set((0, 1, 2, max(k - 1, 0), k + 3, 200, 290))):
        items = rng.choice(NI, M, replace=False)
        lists.append([(int(i), float(r)) for i, r in zip(items, rng.integers(1, 11, M) * 0.5)])
    lists.append([(int(i), 2.5) for i in range(294, NI)])     # only zero rows
    return T, offs, lists


def targets_of(k, lists):
    rng = np.random.default_rng(77 + k)
    out = []
    for e, lst in enumerate(lists):
        t = ([lst[0][0]] if lst else []) + [NI - 1] + [int(v) for v in rng.integers(0, NI, 40)]
        out.append(t[:QS[e]])
    return out


@functools.lru_cache(maxsize=None)
def case(k, nonneg_table):
    T, offs, lists = fixture(k, nonneg_table)
    T.setflags(write=False)
    offs.setflags(write=False)
    targets = targets_of(k, lists)
    assert {len(t) for t in targets} >= {0, 1, 3, TILE, TILE + 1, 40} or k == 1
    return T, offs, lists, targets


def form_args(form, offs):
    """Keyword arguments of foldin.fold_in / foldin.explain for a form."""
    if form == "implicit":
        return dict(mode="implicit", alpha=ALPHA)
    icpt = form == "explicit_icpt"
    return dict(mode="explicit", intercept=icpt, row_offset=offs if icpt else None)


def bars(T, rows, form):
    """A = [a, 1] with the intercept, a otherwise, for rows of T."""
    A = T[np.asarray(rows, np.int64)].reshape(len(rows), T.shape[1])
    if form == "explicit_icpt":
        A = np.hstack([A, np.ones((len(rows), 1))])
    return A


def system(T, offs, lst, form, reg, mode):
    """(G, A[M, K], coef[M]) of one list in fp64, as include/mr_foldin.h and
    include/mr_explain.h define them; c = A^T coef."""
    k = T.shape[1]
    ids = np.array([i for i, _ in lst], np.int64)
    r = np.array([v for _, v in lst], np.float64)
    A = bars(T, ids, form)
    if form == "implicit":
        w = ALPHA * r
        G = T.T @ T + (A * w[:, None]).T @ A
        coef = 1.0 + w
    else:
        G = A.T @ A
        coef = r - offs[ids] if form == "explicit_icpt" else r
    G[np.arange(k), np.arange(k)] += reg * len(lst) if mode == "weighted" else reg
    return G, A, coef


def reference(T, offs, lst, tg, form, reg, mode):
    """Of one entity with a non-empty list: dict of x*, phi*[Q, M], score*[Q],
    cond_2(G) and the bounds of the issue,
      phi:   8 (K + M) eps cond_2(G) |coef_j| ||G^-1||_2 ||A_t||_2 ||A_j||_2
      score: 8 (K + M) eps cond_2(G) max|x*| ||A_t||_1."""
    G, A, coef = system(T, offs, lst, form, reg, mode)
    K, M = len(G), len(lst)
    At = bars(T, tg, form)
    x = np.linalg.solve(G, A.T @ coef)
    Z = np.linalg.solve(G, At.T) if len(tg) else np.zeros((K, 0))     # [K, Q]
    phi = (A @ Z).T * coef[None, :]
    sv = np.linalg.svd(G, compute_uv=False)
    cond, ginv = sv[0] / sv[-1], 1.0 / sv[-1]
    f = 8 * (K + M) * EPS * cond
    phi_bound = f * ginv * np.linalg.norm(At, axis=1)[:, None] * \
        (np.abs(coef) * np.linalg.norm(A, axis=1))[None, :]
    score_bound = f * np.max(np.abs(x)) * np.sum(np.abs(At), axis=1)
    return dict(x=x, phi=phi, score=At @ x, cond=cond, phi_bound=phi_bound,
                score_bound=score_bound)


def top_of(phi_row, top):
    """The top rule on one target's contributions: (positions, values) of the
    min(top, M) largest, descending, equal values (-0.0 == +0.0) by smaller
    position first -- the stable descending sort."""
    order = np.argsort(-np.asarray(phi_row, np.float64), kind="stable")[:top]
    return order.astype(np.int32), np.asarray(phi_row, np.float64)[order]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)
