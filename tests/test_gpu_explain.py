"""GPU: explanations (mr_explain, foldin.explain and its faces) against fp64
NumPy (explain_cases.py).

Bounds, from the project's 8 (K + M) eps cond_2(G) max|x| carried through
d(u^T G^-1 v) = -u^T G^-1 dG G^-1 v:
  |phi - phi*|   <= 8 (K + M) eps cond_2(G) |coef_j| ||G^-1||_2 ||A_t||_2 ||A_j||_2
  |score - s*|   <= 8 (K + M) eps cond_2(G) max|x*| ||A_t||_1
  |sum_j phi - score| <= the sum of the entry bounds + the score bound
An entry whose bound is 0 must be exactly 0.  Every system used has cond_2(G)
<= 1e5 (asserted; the largest of the fixture is 4.6e4).
"""
import functools

import numpy as np
import pytest

import explain_cases as C

pytestmark = pytest.mark.gpu

ALL = [(k, form, reg, mode, sign) for k in C.KS for form in C.FORMS for reg, mode in C.REGS
       for sign in (False, True)]
ALL_IDS = [f"k{k}-{form}-{reg}-{mode}-{'abs' if sign else 'signed'}"
           for k, form, reg, mode, sign in ALL]


@functools.lru_cache(maxsize=None)
def run(k, form, reg, mode, sign, top=5, full=True):
    """One mr_explain call on the whole fixture of (k, sign); shared."""
    from movie_recommender_amd.foldin import explain_arrays
    T, offs, lists, targets = C.case(k, sign)
    out = explain_arrays(T, lists, targets, reg=reg, reg_mode=mode, top=top, full=full,
                         **C.form_args(form, offs))
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def refs(k, form, reg, mode, sign):
    T, offs, lists, targets = C.case(k, sign)
    return [C.reference(T, offs, lst, tg, form, reg, mode) if lst else None
            for lst, tg in zip(lists, targets)]


def blocks(out, e):
    """(score[Q], phi[Q, M]) of entity e from the flat arrays."""
    Q = int(out["toff"][e + 1] - out["toff"][e])
    M = int(out["off"][e + 1] - out["off"][e])
    return (out["score"][out["toff"][e]:out["toff"][e + 1]],
            out["phi"][out["poff"][e]:out["poff"][e + 1]].reshape(Q, M))


# ---------------------------------------------------------------------------
# 1. x and status are mr_fold_in's
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k,form,reg,mode,sign", ALL, ids=ALL_IDS)
def test_x_and_status_are_fold_in_bits(gpu, k, form, reg, mode, sign):
    from movie_recommender_amd.foldin import fold_in
    T, offs, lists, targets = C.case(k, sign)
    X, status, _ = fold_in(T, lists, reg=reg, reg_mode=mode, **C.form_args(form, offs))
    out = run(k, form, reg, mode, sign)
    assert out["x"].shape == X.shape
    assert np.array_equal(C.bits(out["x"]), C.bits(X))
    assert np.array_equal(out["status"], status) and np.all(status == 1)


# ---------------------------------------------------------------------------
# 2. contributions against NumPy
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k,form,reg,mode,sign", ALL, ids=ALL_IDS)
def test_contributions_vs_numpy(gpu, k, form, reg, mode, sign):
    T, offs, lists, targets = C.case(k, sign)
    out = run(k, form, reg, mode, sign)
    worst, checked = 0.0, 0
    for e, ref in enumerate(refs(k, form, reg, mode, sign)):
        _, phi = blocks(out, e)
        assert phi.shape == (len(targets[e]), len(lists[e]))
        if ref is None or not targets[e]:
            continue
        assert ref["cond"] <= C.COND_MAX, (e, ref["cond"])
        err, bound = np.abs(phi - ref["phi"]), ref["phi_bound"]
        assert np.all(phi[bound == 0.0] == 0.0), e
        pos = bound > 0.0
        if pos.any():
            worst = max(worst, float(np.max(err[pos] / bound[pos])))
        assert np.all(err <= bound), (e, float(np.max(err - bound)))
        checked += phi.size
    assert checked > 0
    print(f"k={k} {form} reg={reg} {mode} abs={sign}: worst |phi - phi*| / bound {worst:.3e}")


# ---------------------------------------------------------------------------
# 3. scores and the identity
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k,form,reg,mode,sign", ALL, ids=ALL_IDS)
def test_scores_and_identity(gpu, k, form, reg, mode, sign):
    T, offs, lists, targets = C.case(k, sign)
    out = run(k, form, reg, mode, sign)
    worst_s = worst_i = 0.0
    for e, ref in enumerate(refs(k, form, reg, mode, sign)):
        score, phi = blocks(out, e)
        if ref is None:
            assert np.all(score == 0.0), e
            continue
        if not targets[e]:
            continue
        assert ref["cond"] <= C.COND_MAX, (e, ref["cond"])
        es, bs = np.abs(score - ref["score"]), ref["score_bound"]
        assert np.all(es <= bs), (e, es, bs)
        ei, bi = np.abs(phi.sum(axis=1) - score), ref["phi_bound"].sum(axis=1) + bs
        assert np.all(ei <= bi), (e, ei, bi)
        if (bs > 0).any():
            worst_s = max(worst_s, float(np.max(es[bs > 0] / bs[bs > 0])))
        if (bi > 0).any():
            worst_i = max(worst_i, float(np.max(ei[bi > 0] / bi[bi > 0])))
    print(f"k={k} {form} reg={reg} {mode} abs={sign}: worst score error / bound {worst_s:.3e}, "
          f"|sum phi - score| / bound {worst_i:.3e}")


# ---------------------------------------------------------------------------
# 4. top lists are exact
# ---------------------------------------------------------------------------
def check_top(out, top):
    """top_pos / top_val / top_cnt of `out` against the stable descending sort
    of out["phi"], bit for bit."""
    n = 0
    for e in range(len(out["off"]) - 1):
        _, phi = blocks(out, e)
        M = phi.shape[1]
        for q in range(phi.shape[0]):
            t = int(out["toff"][e]) + q
            pos, val = C.top_of(phi[q], top)
            cnt = min(top, M)
            assert out["top_cnt"][t] == cnt, (e, q)
            assert np.array_equal(out["top_pos"][t, :cnt], pos), (e, q)
            assert np.array_equal(C.bits(out["top_val"][t, :cnt]), C.bits(val)), (e, q)
            assert np.all(out["top_pos"][t, cnt:] == -1), (e, q)
            assert np.all(C.bits(out["top_val"][t, cnt:]) == 0), (e, q)
            n += 1
    return n


@pytest.mark.parametrize("top", [1, 5, 64])
@pytest.mark.parametrize("form", C.FORMS)
@pytest.mark.parametrize("k", C.KS)
def test_top_lists_are_the_stable_sort_of_phi(gpu, k, form, top):
    reg, mode = C.REGS[1]
    out = run(k, form, reg, mode, False, top=top)
    M = np.diff(out["off"])
    assert (M[np.diff(out["toff"]) > 0] < top).any()             # a list shorter than top
    assert check_top(out, top) == out["toff"][-1]
    lean = run(k, form, reg, mode, False, top=top, full=False)   # phi not requested
    assert "phi" not in lean
    for name in ("top_pos", "top_cnt", "x", "status"):
        assert np.array_equal(lean[name], out[name]), name
    for name in ("top_val", "score"):
        assert np.array_equal(C.bits(lean[name]), C.bits(out[name])), name


@pytest.mark.parametrize("form", C.FORMS)
def test_ties_go_to_the_smaller_position(gpu, form):
    """A list that holds one row twice with the same r: the two contributions
    are the same bits for every target and the smaller position comes first;
    so do the +0.0 / -0.0 contributions of zero rows."""
    from movie_recommender_amd.foldin import explain_arrays
    k = 5
    T, offs, _, _ = C.case(k, False)
    lists = [[(7, 2.0), (3, 1.5), (7, 2.0), (295, 4.0), (11, 0.5), (3, 1.5), (296, 1.0)]]
    targets = [[7, 3, 20, 299, 150]]
    for top in (1, 3, 64):
        out = explain_arrays(T, lists, targets, reg=0.5, top=top, full=True,
                             **C.form_args(form, offs))
        _, phi = blocks(out, 0)
        assert np.array_equal(C.bits(phi[:, 0]), C.bits(phi[:, 2]))
        assert np.array_equal(C.bits(phi[:, 1]), C.bits(phi[:, 5]))
        assert check_top(out, top) == 5
        for q in range(5):
            pos = out["top_pos"][q, :out["top_cnt"][q]].tolist()
            for a, b in ((0, 2), (1, 5)):
                if phi[q, a] == 0.0:      # a zero-row target: every entry ties, by position
                    continue
                if b in pos:
                    assert a in pos and pos.index(a) + 1 == pos.index(b), (q, pos)
                elif a in pos:
                    assert pos.index(a) == len(pos) - 1, (q, pos)


# ---------------------------------------------------------------------------
# 5. independence and determinism
# ---------------------------------------------------------------------------
def same(a, b):
    return (np.array_equal(C.bits(a.x), C.bits(b.x)) and np.array_equal(a.status, b.status)
            and len(a.score) == len(b.score)
            and all(np.array_equal(C.bits(s), C.bits(t)) for s, t in zip(a.score, b.score))
            and all(np.array_equal(C.bits(s), C.bits(t)) for s, t in zip(a.phi, b.phi))
            and a.top == b.top)


@pytest.mark.parametrize("form", C.FORMS)
@pytest.mark.parametrize("k", [5, 68, 128])
def test_alone_in_a_batch_reversed_and_twice(gpu, k, form):
    from movie_recommender_amd.foldin import Explanation, explain
    T, offs, lists, targets = C.case(k, False)
    kw = dict(reg=0.05, reg_mode="weighted", top=5, full=True, **C.form_args(form, offs))
    batch = explain(T, lists, targets, **kw)
    assert same(batch, explain(T, lists, targets, **kw))                       # two calls
    rev = explain(T, lists[::-1], targets[::-1], **kw)
    back = Explanation(rev.x[::-1], rev.status[::-1], rev.score[::-1], rev.top[::-1],
                       rev.phi[::-1])
    assert same(batch, back)
    for e in range(len(lists)):
        one = explain(T, [lists[e]], [targets[e]], **kw)
        pick = Explanation(batch.x[e:e + 1], batch.status[e:e + 1], batch.score[e:e + 1],
                           batch.top[e:e + 1], batch.phi[e:e + 1])
        assert same(one, pick), e


def test_duplicate_targets_give_the_same_bits(gpu):
    from movie_recommender_amd.foldin import explain
    k = 20
    T, offs, lists, _ = C.case(k, False)
    tg = [5, 17, 5, 299, 17] + [5] * 20       # copies in several groups, waves and passes
    ex = explain(T, [lists[5]], [tg], reg=0.5, top=5, full=True,
                 **C.form_args("explicit_icpt", offs))
    first = {}
    for q, t in enumerate(tg):
        p = first.setdefault(t, q)
        assert C.bits(ex.score[0])[q] == C.bits(ex.score[0])[p]
        assert np.array_equal(C.bits(ex.phi[0][q]), C.bits(ex.phi[0][p]))
        assert ex.top[0][q] == ex.top[0][p]


def test_batch_crosses_the_phi_chunk(gpu):
    """The device phi buffer holds 256 MiB = 33,554,432 doubles.  2,900
    entities with the M = 290 list and 40 targets need 33,640,000, so the call
    takes two launches and the buffer is reused; every copy must return the
    bits of the entity explained alone."""
    from movie_recommender_amd.foldin import explain_arrays
    k, B = 5, 2900
    T, offs, lists, targets = C.case(k, False)
    e = next(i for i, l in enumerate(lists) if len(l) == 290)
    tg = (targets[e] + list(range(40)))[:40]
    assert B * 290 * 40 > (1 << 28) // 8 > (B - 1) * 290 * 40 // 2
    kw = dict(reg=0.05, reg_mode="weighted", top=5, full=True,
              **C.form_args("explicit_icpt", offs))
    one = explain_arrays(T, [lists[e]], [tg], **kw)
    out = explain_arrays(T, [lists[e]] * B, [tg] * B, **kw)
    assert np.array_equal(C.bits(out["phi"]).reshape(B, -1),
                          np.broadcast_to(C.bits(one["phi"]), (B, 290 * 40)))
    for name in ("x", "score", "top_val"):
        assert np.array_equal(C.bits(out[name]).reshape(B, -1),
                              np.broadcast_to(C.bits(one[name]).reshape(1, -1),
                                              (B, one[name].size))), name
    assert np.array_equal(out["top_pos"].reshape(B, -1),
                          np.broadcast_to(one["top_pos"].reshape(1, -1), (B, 40 * 5)))
    assert np.all(out["status"] == 1) and np.all(out["top_cnt"] == 5)


# ---------------------------------------------------------------------------
# 6. edges
# ---------------------------------------------------------------------------
def test_empty_lists_and_no_targets(gpu):
    from movie_recommender_amd.foldin import explain
    T, offs, lists, targets = C.case(5, False)
    kw = dict(reg=0.5, top=5, full=True, **C.form_args("explicit_icpt", offs))
    ex = explain(T, [[], lists[4], []], [[3, 299], [], [1] * 17], **kw)
    assert ex.status.tolist() == [1, 1, 1] and np.all(ex.x[[0, 2]] == 0.0)
    assert np.all(ex.score[0] == 0.0) and np.all(ex.score[2] == 0.0) and ex.score[1].size == 0
    assert ex.top == [[[], []], [], [[]] * 17]
    assert [p.shape for p in ex.phi] == [(2, 0), (0, len(lists[4])), (17, 0)]
    alone = explain(T, [lists[4]], [[]], **kw)
    assert np.array_equal(C.bits(alone.x[0]), C.bits(ex.x[1]))
    none = explain(T, lists, [[] for _ in lists], **kw)                 # Q = 0 everywhere
    full = explain(T, lists, targets, **kw)
    assert np.array_equal(C.bits(none.x), C.bits(full.x)) and np.all(none.status == 1)
    assert all(s.size == 0 for s in none.score) and all(t == [] for t in none.top)


def test_status_zero_is_all_zero(gpu):
    """T = ones(2, 2), one rating, no ridge: G = [[1, 1], [1, 1]] in exact
    binary numbers, the second pivot is 1 - 1 * 1 = 0 (test_gpu_foldin's
    case)."""
    from movie_recommender_amd.foldin import explain_arrays
    T = np.ones((2, 2))
    out = explain_arrays(T, [[(0, 2.0)], [(1, 1.0)], [(0, 2.0)]], [[0, 1, 1], [0], []],
                         reg=0.0, top=4, full=True)
    assert out["status"].tolist() == [0, 0, 0] and np.all(out["x"] == 0.0)
    assert np.all(out["score"] == 0.0) and np.all(out["phi"] == 0.0) and out["phi"].size == 4
    assert np.all(out["top_cnt"] == 0) and np.all(out["top_pos"] == -1)
    assert np.all(C.bits(out["top_val"]) == 0)
    ok = explain_arrays(T, [[(0, 2.0)]], [[0, 1, 1]], reg=0.5, top=4, full=True)
    assert ok["status"].tolist() == [1] and np.all(ok["top_cnt"] == 1)
    ref = C.reference(T, None, [(0, 2.0)], [0, 1, 1], "explicit", 0.5, "constant")
    assert np.all(np.abs(ok["phi"].reshape(3, 1) - ref["phi"]) <= ref["phi_bound"])


@pytest.mark.parametrize("form", ["explicit", "implicit"])
@pytest.mark.parametrize("k", C.KS)
def test_zero_row_target_is_exactly_zero(gpu, k, form):
    T, offs, lists, targets = C.case(k, False)
    out = run(k, form, 0.5, "constant", False)
    seen = 0
    for e, tg in enumerate(targets):
        score, phi = blocks(out, e)
        for q, t in enumerate(tg):
            if t >= 294:
                assert score[q] == 0.0 and np.all(phi[q] == 0.0), (e, q)
                seen += 1
    assert seen >= 5


# ---------------------------------------------------------------------------
# 7. faces
# ---------------------------------------------------------------------------
ENGINE_TOL = 6.66e-07   # the fold-in's tolerance against the engine (test_gpu_foldin.py)


def test_explain_users_and_items_vs_engine(gpu):
    """A training user explained from its own ratings: the scores are the
    engine's predictions V[t] . u[:k] + u[k] for that user (items: U[t, :k] .
    v, the user's bias left to the caller), relative to the largest one."""
    from conftest import rel_err
    from movie_recommender_amd.engine import AlsContext
    from movie_recommender_amd.foldin import (explain_items, explain_users, fold_in_items,
                                              fold_in_users)
    import nnls_cases
    k = 10
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
    rng = np.random.default_rng(9)
    tg_u = [[int(t) for t in rng.integers(0, nI, 6)] for _ in range(nU)]
    tg_i = [[int(t) for t in rng.integers(0, nU, 6)] for _ in range(nI)]
    ex = explain_users(V, by_user, tg_u, 0.3, "weighted", top=3)
    X, status, _ = fold_in_users(V, by_user, 0.3, "weighted")
    assert np.array_equal(C.bits(ex.x), C.bits(X)) and np.array_equal(ex.status, status)
    got = np.array(ex.score)
    pred = np.einsum("uqk,uk->uq", V[np.array(tg_u)], U[:, :k]) + U[:, k:]
    folded = np.einsum("uqk,uk->uq", V[np.array(tg_u)], X[:, :k]) + X[:, k:]
    has = np.array([len(l) > 0 for l in by_user])
    assert np.all(got[~has] == 0.0) and (~has).sum() == 2
    eu = rel_err(got[has], pred[has])
    assert rel_err(got[has], folded[has]) <= 1e-13
    exi = explain_items(U, by_item, tg_i, 0.3, "weighted", top=3)
    Yf, _, _ = fold_in_items(U, by_item, 0.3, "weighted")
    assert np.array_equal(C.bits(exi.x), C.bits(Yf))
    goti = np.array(exi.score)
    hasi = np.array([len(l) > 0 for l in by_item])
    Ut = U[np.array(tg_i)][:, :, :k]
    assert rel_err(goti[hasi], np.einsum("iqk,ik->iq", Ut, Yf)[hasi]) <= 1e-13
    ei = rel_err(goti[hasi], np.einsum("iqk,ik->iq", Ut, V2)[hasi])
    print(f"explain_users vs engine {eu:.3e} (tolerance {ENGINE_TOL:.2e}), explain_items {ei:.3e}")
    assert eu <= ENGINE_TOL
    # a top entry names a rated item, its position and its contribution
    e0 = int(np.flatnonzero(has)[0])
    for per in ex.top[e0]:
        assert len(per) == min(3, len(by_user[e0]))
        for row, pos, val in per:
            assert by_user[e0][pos][0] == row
        assert [v for _, _, v in per] == sorted((v for _, _, v in per), reverse=True)


def test_implicit_model_explain(gpu):
    from movie_recommender_amd.implicit import ImplicitModel
    k, reg, mode = 20, 0.5, "constant"
    Y, offs, lists, targets = C.case(k, True)
    rng = np.random.default_rng(5)
    Xtab = np.abs(rng.uniform(-1, 1, (70, k)))
    item_lists = [[(int(u), float(rng.integers(1, 11)) * 0.5)
                   for u in rng.choice(70, M, replace=False)] for M in (0, 1, 25, 70)]
    item_targets = [[0, 69], [3], [5, 5, 60], list(range(0, 70, 4))]
    with ImplicitModel(Xtab, Y, alpha=C.ALPHA, reg=reg, reg_mode=mode) as model:
        Xn, status = model.fold_in(lists)
        ex = model.explain(lists, targets, top=5, full=True)
        assert np.array_equal(C.bits(ex.x), C.bits(Xn)) and np.array_equal(ex.status, status)
        for e, (lst, tg) in enumerate(zip(lists, targets)):
            if not lst or not tg:
                continue
            ref = C.reference(Y, offs, lst, tg, "implicit", reg, mode)
            assert ref["cond"] <= C.COND_MAX
            bound = ref["phi_bound"].sum(axis=1) + ref["score_bound"]
            assert np.all(np.abs(ex.phi[e].sum(axis=1) - Xn[e] @ Y[tg].T) <= bound), e
        Yn, status_i = model.fold_in_items(item_lists)
        exi = model.explain_items(item_lists, item_targets, top=5, full=True)
        assert np.array_equal(C.bits(exi.x), C.bits(Yn))
        for e, (lst, tg) in enumerate(zip(item_lists, item_targets)):
            if not lst:
                assert np.all(exi.score[e] == 0.0) and exi.top[e] == [[] for _ in tg]
                continue
            ref = C.reference(Xtab, None, lst, tg, "implicit", reg, mode)
            assert ref["cond"] <= C.COND_MAX
            bound = ref["phi_bound"].sum(axis=1) + ref["score_bound"]
            assert np.all(np.abs(exi.phi[e].sum(axis=1) - Yn[e] @ Xtab[tg].T) <= bound), e
    with ImplicitModel(Xtab, Y, alpha=C.ALPHA, reg=reg, reg_mode=mode, nonneg=True) as model:
        with pytest.raises(ValueError, match="nonneg"):
            model.explain(lists, targets)


def test_movie_table_explain_ridge(gpu):
    from movie_recommender_amd.serving import MovieTable
    k, n, reg = 8, 40, 0.1
    rng = np.random.default_rng(77)
    V = rng.uniform(-1, 1, (n, k))
    mids = [10 + 7 * j for j in range(n)]                       # non-contiguous movie ids
    perm = rng.permutation(n)
    als_ids = {mids[j]: int(perm[j]) for j in range(n)}
    no_median = [mids[3], mids[17]]
    medians = {m: float(rng.integers(4, 9)) * 0.5 for m in mids if m not in no_median}
    unknown = 9999
    usable = [m for m in mids if m not in no_median]
    lists = [[],
             [(usable[4], 4.0), (unknown, 3.0), (no_median[0], 2.0)],
             [(m, float(rng.integers(1, 11)) * 0.5) for m in rng.choice(usable, 30, replace=False)]]
    lists[2] = [(int(m), r) for m, r in lists[2]]
    tgs = [[usable[0]], [usable[1], unknown, no_median[1]], [usable[2], 12345, usable[3]]]
    with MovieTable(k, V.reshape(-1), als_ids, medians) as table:
        valid, ex, dropped = table.explain_ridge(lists, tgs, reg, top=4)
        fv, X, _ = table.fold_in_ridge(lists, reg)
        assert valid.tolist() == fv.tolist() == [False, True, True]
        assert dropped == [[], [unknown], [12345]]
        assert [list(d) for d in ex] == [[usable[0]], [usable[1], no_median[1]],
                                         [usable[2], usable[3]]]
        assert ex[0][usable[0]] == (0.0, [])
        score, contrib = ex[1][usable[1]]
        assert [m for m, _ in contrib] == [usable[4]]            # the one usable rating
        rated = {m for m, _ in lists[2]}
        for mid in (usable[2], usable[3]):
            score, contrib = ex[2][mid]
            pred = V[als_ids[mid]] @ X[2, :k] + X[2, k]
            assert abs(score - pred) <= 1e-12 * max(1.0, abs(pred))
            assert len(contrib) == 4 and all(m in rated for m, _ in contrib)
            assert [v for _, v in contrib] == sorted((v for _, v in contrib), reverse=True)
        with pytest.raises(ValueError):
            table.explain_ridge(lists, tgs, 0.0)
        with pytest.raises(ValueError):
            table.explain_ridge(lists, tgs[:2], reg)
