"""GPU: the general fold-in (mr_fold_in, foldin.py) and its serving / implicit
faces against fp64 NumPy and the NNLS oracle of nnls_cases.py.

Fixture, per k from default_rng(1200 + k): a 300-row table, uniform(-1, 1)
rounded through fp32 (|.| of it for the non-negative tables), rows 294 .. 299
zero, row offsets in {0.25, ..., 2.5}; lists of 0, 1, 2, k - 1, k + 3, 200 and
290 distinct rows with r in {0.5, ..., 5}, and one list of the six zero rows.
k: 1, 5, 20; 67 / 68 straddle the one-pass / two-pass triangle (K (K + 1) / 2
= 2304 entries at K = 67); 128 with the intercept is the LDS maximum K = 129.
Forms: explicit with intercept and offsets, explicit without either, implicit
at alpha = 8.

Error bound everywhere: the project's 8 (K + M) eps cond_2(G) max|x|
(test_gpu_ranking.test_fold_in_vs_numpy), for the non-negative solve on G_FF of
the oracle's final free set.
"""
import functools

import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu

NI = 300
KS = [1, 5, 20, 67, 68, 128]
FORMS = ["explicit_icpt", "explicit", "implicit"]
REGS = [(0.5, "constant"), (0.05, "weighted")]
ALPHA = 8.0
EPS = np.finfo(np.float64).eps


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


@functools.lru_cache(maxsize=None)
def case(k, nonneg_table):
    T, offs, lists = fixture(k, nonneg_table)
    T.setflags(write=False)
    offs.setflags(write=False)
    return T, offs, lists


def normal(T, offs, lst, form, reg, mode):
    """(G, c) of one list in fp64, as include/mr_foldin.h defines them."""
    k = T.shape[1]
    ids = np.array([i for i, _ in lst], np.int64)
    r = np.array([v for _, v in lst])
    A = T[ids]
    if form == "implicit":
        w = ALPHA * r
        G = T.T @ T + (A * w[:, None]).T @ A
        c = A.T @ (1.0 + w)
    else:
        if form == "explicit_icpt":
            A = np.hstack([A, np.ones((len(lst), 1))])
            r = r - offs[ids]
        G = A.T @ A
        c = A.T @ r
    G[np.arange(k), np.arange(k)] += reg * len(lst) if mode == "weighted" else reg
    return G, c


def call(T, offs, lists, form, reg, mode, **kw):
    from movie_recommender_amd.foldin import fold_in
    if form == "implicit":
        return fold_in(T, lists, "implicit", alpha=ALPHA, reg=reg, reg_mode=mode, **kw)
    icpt = form == "explicit_icpt"
    return fold_in(T, lists, "explicit", intercept=icpt, row_offset=offs if icpt else None,
                   reg=reg, reg_mode=mode, **kw)


def csr_of(lists):
    off = np.zeros(len(lists) + 1, np.int64)
    off[1:] = np.cumsum([len(l) for l in lists])
    return (off, np.array([i for l in lists for i, _ in l], np.int64),
            np.array([r for l in lists for _, r in l]))


def bound_of(G, M, ref):
    if G.size == 0:
        return 0.0
    return 8 * (len(G) + M) * EPS * np.linalg.cond(G) * np.max(np.abs(ref))


def degenerate(offs, lst, form):
    """With an intercept and every r - offset of the list equal to one value
    rho, the minimiser is x[:k] = 0, x[k] = rho and every constrained y_j is
    exactly 0 in exact arithmetic: whether a coordinate enters the free set is
    rounding's choice (the oracle itself takes 1 or 2 rounds with the order of
    its sums).  True of every single-rating list, and of the two-rating list
    of k = 1 (3.5 - 2.5 twice)."""
    return form == "explicit_icpt" and len({r - offs[i] for i, r in lst}) == 1


def is_plus_zero(v):
    return v == 0.0 and not np.signbit(v)


# ---------------------------------------------------------------------------
# 1. the Cholesky solve against NumPy
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nonneg_table", [False, True])
@pytest.mark.parametrize("reg,mode", REGS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("k", KS)
def test_cholesky_vs_numpy(gpu, k, form, reg, mode, nonneg_table):
    T, offs, lists = case(k, nonneg_table)
    K = k + (form == "explicit_icpt")
    X, status, rounds = call(T, offs, lists, form, reg, mode)
    assert X.shape == (len(lists), K)
    X2, status2, rounds2 = call(T, offs, csr_of(lists), form, reg, mode)
    assert np.array_equal(X, X2) and np.array_equal(status, status2) and \
        np.array_equal(rounds, rounds2)                           # CSR input, same bits
    worst = 0.0
    for e, lst in enumerate(lists):
        if len(lst) == 0:
            assert np.all(X[e] == 0.0) and status[e] == 1 and rounds[e] == 0, e
            continue
        assert status[e] == 1 and rounds[e] == 1, (e, status[e], rounds[e])
        if form == "implicit" and all(i >= 294 for i, _ in lst):
            assert np.all(X[e] == 0.0), e
            continue
        G, c = normal(T, offs, lst, form, reg, mode)
        ref = np.linalg.solve(G, c)
        bound = bound_of(G, len(lst), ref)
        err = np.max(np.abs(X[e] - ref))
        worst = max(worst, err / bound if bound else 0.0)
        assert err <= bound, (e, len(lst), err, bound)
    print(f"k={k} {form} reg={reg} {mode} nonneg_table={nonneg_table}: "
          f"worst error / bound {worst:.3e}")


# ---------------------------------------------------------------------------
# 2. the non-negative solve against the oracle
# ---------------------------------------------------------------------------
def check_nnls(T, offs, lists, form, reg, mode, X, status, rounds, max_rounds=0):
    """X / status / rounds of ``lists`` against nnls_cases.nnls_bpp (cold
    start; ``rounds`` None: a face that does not return them); the
    degenerate lists are left to their own test."""
    import nnls_cases
    k = T.shape[1]
    K = k + (form == "explicit_icpt")
    worst, checked = 0.0, 0
    for e, lst in enumerate(lists):
        if len(lst) == 0:
            assert np.all(X[e] == 0.0) and status[e] == 1, e
            assert rounds is None or rounds[e] == 0, e
            continue
        if degenerate(offs, lst, form):
            continue
        G, c = normal(T, offs, lst, form, reg, mode)
        ref, st = nnls_cases.nnls_bpp(G, c, k, np.zeros(K), warm=False, max_rounds=max_rounds)
        want = (1, st) if st > 0 else (-1, -st)
        assert status[e] == want[0], (e, len(lst), status[e], st)
        assert rounds is None or rounds[e] == want[1], (e, len(lst), rounds[e], st)
        assert np.array_equal(X[e, :k] > 0, ref[:k] > 0), (e, len(lst))      # the support
        assert np.all(X[e, :k] >= 0.0), e
        assert all(is_plus_zero(v) for v in X[e, :k][ref[:k] == 0]), e
        F = np.flatnonzero(np.concatenate([ref[:k] > 0, np.ones(K - k, bool)]))
        bound = bound_of(G[np.ix_(F, F)], len(lst), ref)
        err = np.max(np.abs(X[e] - ref))
        worst = max(worst, err / bound if bound else 0.0)
        assert err <= bound, (e, len(lst), err, bound)
        checked += 1
    return worst, checked


@pytest.mark.parametrize("nonneg_table", [False, True])
@pytest.mark.parametrize("reg,mode", REGS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("k", KS)
def test_nnls_vs_oracle(gpu, k, form, reg, mode, nonneg_table):
    T, offs, lists = case(k, nonneg_table)
    X, status, rounds = call(T, offs, lists, form, reg, mode, nonneg=True)
    X2, status2, rounds2 = call(T, offs, csr_of(lists), form, reg, mode, nonneg=True)
    assert np.array_equal(X, X2) and np.array_equal(status, status2) and \
        np.array_equal(rounds, rounds2)
    worst, checked = check_nnls(T, offs, lists, form, reg, mode, X, status, rounds)
    assert checked == sum(len(l) > 0 and not degenerate(offs, l, form) for l in lists)
    assert checked >= len(lists) - (3 if k == 1 else 2)
    print(f"k={k} {form} reg={reg} {mode} nonneg_table={nonneg_table}: rounds "
          f"{rounds.tolist()} worst error / bound {worst:.3e}")


def test_nnls_batch_crosses_the_scratch_chunk(gpu):
    """The non-negative solve keeps G_e in a scratch of at most 256 MiB: 2,000
    slots of [K][K + 1] fp64 at K = 129, so 2,100 entities take two launches
    with the slots reused.  Entity e gets list e mod 8 of the fixture: every
    copy must return the bits of the 8-entity call (checked against the oracle
    by test_nnls_vs_oracle)."""
    k, form, reg, mode, B = 128, "explicit_icpt", 0.05, "weighted", 2100
    T, offs, lists = case(k, True)
    assert (1 << 28) // ((k + 1) * (k + 2) * 8) < B - len(lists)
    X8, status8, rounds8 = call(T, offs, lists, form, reg, mode, nonneg=True)
    pick = np.arange(B) % len(lists)
    X, status, rounds = call(T, offs, [lists[j] for j in pick], form, reg, mode, nonneg=True)
    assert np.array_equal(X, X8[pick]) and np.array_equal(status, status8[pick]) and \
        np.array_equal(rounds, rounds8[pick])


@pytest.mark.parametrize("nonneg_table", [False, True])
@pytest.mark.parametrize("reg,mode", REGS)
@pytest.mark.parametrize("k", KS)
def test_nnls_degenerate_lists_with_intercept(gpu, k, reg, mode, nonneg_table):
    """The lists `degenerate` excludes above (the single-rating list for every
    k): only the solution is held to the bound, x[:k] to 0 and x[k] to r -
    offset; status and non-negativity as everywhere."""
    T, offs, lists = case(k, nonneg_table)
    picked = [l for l in lists if len(l) > 0 and degenerate(offs, l, "explicit_icpt")]
    assert any(len(l) == 1 for l in picked)
    X, status, rounds = call(T, offs, picked, "explicit_icpt", reg, mode, nonneg=True)
    for e, lst in enumerate(picked):
        G, c = normal(T, offs, lst, "explicit_icpt", reg, mode)
        ref = np.zeros(k + 1)
        ref[k] = lst[0][1] - offs[lst[0][0]]
        assert status[e] == 1 and rounds[e] >= 1
        assert np.all(X[e, :k] >= 0.0)
        assert np.max(np.abs(X[e] - ref)) <= bound_of(G, len(lst), ref), (X[e], ref)


# ---------------------------------------------------------------------------
# 3. the implicit form, bit for bit the old entry point
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("reg,mode", [(0.5, "constant"), (0.05, "weighted"), (0.0, "constant")])
@pytest.mark.parametrize("k", [5, 20, 64, 128])
def test_implicit_form_is_bitwise_the_old_entry(gpu, k, reg, mode):
    from movie_recommender_amd import implicit
    from movie_recommender_amd.foldin import fold_in
    import test_gpu_ranking as R
    Y, lists = R.fold_fixture(k)
    Xo, so = implicit.fold_in(Y, lists, R.FOLD_ALPHA, reg, mode)
    X, status, rounds = fold_in(Y, lists, "implicit", alpha=R.FOLD_ALPHA, reg=reg, reg_mode=mode)
    assert np.array_equal(X, Xo) and np.array_equal(status, so)
    assert np.array_equal(rounds, [0 if len(l) == 0 else 1 for l in lists])


# ---------------------------------------------------------------------------
# 4. exact cases
# ---------------------------------------------------------------------------
def test_exact_non_positive_pivot_and_negative_rhs(gpu):
    """T = ones(2, 2), one rating: G = [[1, 1], [1, 1]] + reg I in numbers that
    are exact in binary; with reg = 0 the second pivot is 1 - 1 * 1 = 0."""
    from movie_recommender_amd.foldin import fold_in
    T = np.ones((2, 2))
    for nonneg in (False, True):   # the non-negative solve frees both coordinates in round 1
        X, status, rounds = fold_in(T, [[(0, 2.0)], []], reg=0.0, nonneg=nonneg)
        assert status.tolist() == [0, 1] and rounds.tolist() == [0, 0] and np.all(X == 0.0)
    X, status, rounds = fold_in(T, [[(0, 2.0)]], reg=0.5)
    assert status.tolist() == [1] and rounds.tolist() == [1]
    ref = np.linalg.solve(np.array([[1.5, 1.0], [1.0, 1.5]]), [2.0, 2.0])
    assert np.max(np.abs(X[0] - ref)) <= 1e-14
    X, status, rounds = fold_in(T, [[(0, -2.0)]], reg=0.5, nonneg=True)
    assert status.tolist() == [1] and rounds.tolist() == [1]
    assert all(is_plus_zero(v) for v in X[0])
    # a zero diagonal entry: the zero table without a ridge
    X, status, rounds = fold_in(np.zeros((2, 2)), [[(0, 2.0)]], reg=0.0, nonneg=True)
    assert status.tolist() == [0] and rounds.tolist() == [0] and np.all(X == 0.0)


# ---------------------------------------------------------------------------
# 5. the round cap
# ---------------------------------------------------------------------------
def test_round_cap(gpu):
    import nnls_cases
    k, form, reg, mode = 20, "explicit_icpt", 0.05, "weighted"
    T, offs, lists = case(k, False)
    picked = None
    for lst in lists:
        if len(lst) < 2:
            continue
        G, c = normal(T, offs, lst, form, reg, mode)
        if nnls_cases.nnls_bpp(G, c, k, np.zeros(k + 1), warm=False)[1] > 1:
            picked = lst
            break
    assert picked is not None
    X, status, rounds = call(T, offs, [picked], form, reg, mode, nonneg=True, max_rounds=1)
    assert status.tolist() == [-1] and rounds.tolist() == [1]
    worst, checked = check_nnls(T, offs, [picked], form, reg, mode, X, status, rounds,
                                max_rounds=1)
    assert checked == 1
    assert X[0, k] != 0.0 and np.all(X[0, :k] == 0.0)   # round 1: only the intercept is free


# ---------------------------------------------------------------------------
# 6. against the engine's own half-steps
# ---------------------------------------------------------------------------
ENGINE_TOL = 4 * 1.6645e-07   # 4 x the larger measured value of the docstring below


@pytest.mark.parametrize("k", [10, 20])
def test_fold_in_vs_engine(gpu, k):
    """A training user (item) folded in from its own ratings comes back with
    its own factors.  The fold-in is fp64, so the gap is the engine's fp32
    Gram and fp32 factor storage.  Measured on an MI355X on these fixtures
    (nnls_cases.fixture(k), reg = 0.3 weighted, Cholesky, after iterate(3)):
    the engine's half-step against its fp64 restatement (nnls_cases.normal64
    "explicit" + np.linalg.solve), relative to the largest entry,
        k = 10: users 8.3837e-08, items 1.6247e-07
        k = 20: users 5.2426e-08, items 1.6645e-07
    (the same in two runs).  The tolerance is 4 x the larger of the users /
    items values, 4 x 1.6645e-07 = 6.658e-07, to cover run-to-run placement of
    the slab sums.  The fold-in itself measured 8.384e-08 / 1.625e-07 (k = 10)
    and 5.243e-08 / 1.664e-07 (k = 20) against the engine."""
    from movie_recommender_amd.engine import AlsContext
    from movie_recommender_amd.foldin import fold_in_items, fold_in_users
    import nnls_cases
    u, i, r, U0, V0, nU, nI = nnls_cases.fixture(k)
    r32 = np.asarray(r, np.float32).astype(np.float64)
    with AlsContext(u, i, r, k, nU, nI, solver="cholesky", reg=0.3, reg_mode="weighted") as ctx:
        ctx.set_factors(U0, V0)
        ctx.iterate(3)
        ctx.half_step("users")
        U, V = ctx.get_factors()
        ctx.half_step("items")
        _, V2 = ctx.get_factors()
    U, V, V2 = U.reshape(nU, k + 1), V.reshape(nI, k), V2.reshape(nI, k)
    by_user, by_item = [[] for _ in range(nU)], [[] for _ in range(nI)]
    for uu, ii, rr in zip(u, i, r32):
        by_user[uu].append((int(ii), float(rr)))
        by_item[ii].append((int(uu), float(rr)))
    X, status, _ = fold_in_users(V, by_user, 0.3, "weighted")
    Y, status_i, _ = fold_in_items(U, by_item, 0.3, "weighted")
    assert np.all(status == 1) and np.all(status_i == 1)
    has_u = np.array([len(l) > 0 for l in by_user])
    has_i = np.array([len(l) > 0 for l in by_item])
    assert (~has_u).sum() == 2 and (~has_i).sum() >= 1
    assert np.all(X[~has_u] == 0.0) and np.all(Y[~has_i] == 0.0)
    eu, ei = rel_err(X[has_u], U[has_u]), rel_err(Y[has_i], V2[has_i])
    print(f"k={k}: fold-in vs engine users {eu:.3e} items {ei:.3e} (tolerance {ENGINE_TOL:.1e})")
    assert eu <= ENGINE_TOL and ei <= ENGINE_TOL


# ---------------------------------------------------------------------------
# 7. the serving face
# ---------------------------------------------------------------------------
def test_movie_table_fold_in_ridge(gpu):
    from movie_recommender_amd.serving import MovieTable
    k, n, reg = 8, 40, 0.1
    rng = np.random.default_rng(77)
    V = rng.uniform(-1, 1, (n, k))
    mids = [10 + 7 * j for j in range(n)]                       # non-contiguous movie ids
    perm = rng.permutation(n)
    als_ids = {mids[j]: int(perm[j]) for j in range(n)}
    no_median = [mids[3], mids[17], mids[31]]
    medians = {m: float(rng.integers(4, 9)) * 0.5 for m in mids if m not in no_median}
    medians[5] = 3.0                                            # a median without factors
    unknown = 9999
    usable = [m for m in mids if m not in no_median]

    def ratings(ms):
        return [(m, float(rng.integers(1, 11)) * 0.5) for m in ms]
    lists = [[],
             ratings([unknown, no_median[0]]),                  # nothing usable
             ratings([usable[4], unknown]),
             ratings([usable[9], no_median[1], usable[20]]),
             ratings(list(rng.choice(usable, 30, replace=False)) + [unknown, no_median[2]])]
    with MovieTable(k, V.reshape(-1), als_ids, medians) as table:
        valid, X, status = table.fold_in_ridge(lists, reg)
        assert valid.tolist() == [False, False, True, True, True]
        assert X.shape == (5, k + 1) and np.all(X[:2] == 0.0) and np.all(status == 1)
        for e in (2, 3, 4):
            kept = [(als_ids[m], r - medians[m]) for m, r in lists[e]
                    if m in als_ids and m in medians]
            assert len(kept) == (1, 2, 30)[e - 2]
            A = np.hstack([V[[a for a, _ in kept]], np.ones((len(kept), 1))])
            G = A.T @ A
            G[np.arange(k), np.arange(k)] += reg * len(kept)
            ref = np.linalg.solve(G, A.T @ np.array([r for _, r in kept]))
            assert np.max(np.abs(X[e] - ref)) <= bound_of(G, len(kept), ref), e
        # without the medians: the no-median movie is kept and nothing is subtracted
        valid_raw, X_raw, _ = table.fold_in_ridge(lists, reg, subtract_median=False)
        assert valid_raw.tolist() == [False, True, True, True, True]
        kept = [(als_ids[m], r) for m, r in lists[3] if m in als_ids]
        A = np.hstack([V[[a for a, _ in kept]], np.ones((3, 1))])
        G = A.T @ A
        G[np.arange(k), np.arange(k)] += reg * 3
        ref = np.linalg.solve(G, A.T @ np.array([r for _, r in kept]))
        assert np.max(np.abs(X_raw[3] - ref)) <= bound_of(G, 3, ref)
        # the rows feed scores / top_n unchanged
        sc = table.scores(X[3])[0]
        order = sorted(range(len(sc)), key=lambda c: (sc[c], table.cand_mid[c]), reverse=True)
        top = table.top_n(X[3], None, 10)[0]
        assert len(top) == 10
        assert [m for _, m in top] == [int(table.cand_mid[c]) for c in order[:10]]
        assert [s for s, _ in top] == [sc[c] for c in order[:10]]
        assert not table.fold_in(lists)[0][3]                   # the reference's k + 1 minimum
        with pytest.raises(ValueError):
            table.fold_in_ridge(lists, 0.0)


# ---------------------------------------------------------------------------
# 8. ImplicitModel
# ---------------------------------------------------------------------------
def test_implicit_model_nonneg_and_items(gpu):
    from movie_recommender_amd.implicit import ImplicitModel
    k, reg, mode = 20, 0.5, "constant"
    Y, offs, lists = case(k, True)
    rng = np.random.default_rng(5)
    Xtab = np.abs(rng.uniform(-1, 1, (70, k)))
    item_lists = [[(int(u), float(rng.integers(1, 11)) * 0.5)
                   for u in rng.choice(70, M, replace=False)] for M in (0, 1, 25, 70)]
    with ImplicitModel(Xtab, Y, alpha=ALPHA, reg=reg, reg_mode=mode, nonneg=True) as model:
        X, status = model.fold_in(lists)
        assert X.shape == (len(lists), k) and np.all(X >= 0.0) and np.all(status == 1)
        _, checked = check_nnls(Y, offs, lists, "implicit", reg, mode, X, status, None)
        assert checked == len(lists) - 1
        Yn, status_i = model.fold_in_items(item_lists)
        assert np.all(Yn >= 0.0) and np.all(status_i == 1)
    with ImplicitModel(Xtab, Y, alpha=ALPHA, reg=reg, reg_mode=mode) as model:
        Yn, status_i = model.fold_in_items(item_lists)
        assert Yn.shape == (4, k) and np.all(status_i == 1) and np.all(Yn[0] == 0.0)
        for e, lst in enumerate(item_lists):
            if lst:
                G, c = normal(Xtab, None, lst, "implicit", reg, mode)
                ref = np.linalg.solve(G, c)
                assert np.max(np.abs(Yn[e] - ref)) <= bound_of(G, len(lst), ref), e
