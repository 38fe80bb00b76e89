"""GPU: rank counts (mr_rank_counts), the metrics on them, the implicit
fold-in (mr_implicit_fold_in) and ImplicitModel, against NumPy fp64
restatements that live in this file.

Rank fixture, per k from default_rng(700 + k): 70 users x 300 items (three
user tiles, the last partial; two item tiles, the last partial), factors
uniform(-1, 1) rounded through fp32, Y[294:] = 0 (items nobody rated: their
scores tie), Y[7] = Y[260] = Y[3] (exact copies across the two item tiles),
X[5] = 0 (every score of user 5 ties).  Training (= excluded) pairs: 4,000
draws u in [0, 68), i = zipf(1.3) % 294, de-duplicated, user 2's removed.
Held-out pairs: items outside the user's training set -- user 0 none, user 1
130, users 2 .. 67 1 .. 8 each, users 68 and 69 neither list.
k: 5 (below one 16-factor chunk), 20 (one partial chunk), 64 (four chunks).
"""
import functools

import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu

NU, NI = 70, 300
KS = [5, 20, 64]
EPS = np.finfo(np.float64).eps


# ---------------------------------------------------------------------------
# fixture and the NumPy restatement
# ---------------------------------------------------------------------------
def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def fixture(k, rounded=True):
    rng = np.random.default_rng(700 + k)
    X = rng.uniform(-1, 1, (NU, k))
    Y = rng.uniform(-1, 1, (NI, k))
    if rounded:
        X = X.astype(np.float32).astype(np.float64)
        Y = Y.astype(np.float32).astype(np.float64)
    Y[294:] = 0.0
    Y[7] = Y[3]
    Y[260] = Y[3]
    X[5] = 0.0
    u = rng.integers(0, 68, 4000)
    i = rng.zipf(1.3, 4000) % 294
    key = np.unique(u * NI + i)
    key = key[key // NI != 2]                       # user 2 excludes nothing
    eu, ei = key // NI, key % NI
    tu, ti = [], []
    for usr in range(1, 68):
        n = 130 if usr == 1 else int(rng.integers(1, 9))
        free = np.setdiff1d(np.arange(NI), ei[eu == usr])
        tu += [usr] * n
        ti += list(rng.choice(free, n, replace=False))
    tu, ti = np.array(tu), np.array(ti)
    shuffle = rng.permutation(len(tu))              # any input order
    tu, ti = tu[shuffle], ti[shuffle]
    bias = rng.uniform(-1, 1, NU)
    offset = rng.integers(-4, 5, NI) / 4.0          # coarse: ties survive the offsets
    _freeze(X, Y, eu, ei, tu, ti, bias, offset)
    return X, Y, (tu, ti), (eu, ei), bias, offset


def scores64(X, Y, bias=None, offset=None):
    s = 0
    for j in range(X.shape[1]):
        s = s + X[:, j:j + 1] * Y[None, :, j]
    s = s + (np.zeros(len(X)) if bias is None else bias)[:, None]
    return s + (np.zeros(len(Y)) if offset is None else offset)[None, :]


@functools.lru_cache(maxsize=None)
def reference(k, rounded=True, with_exclude=True, with_offsets=False):
    X, Y, (tu, ti), (eu, ei), bias, offset = fixture(k, rounded)
    S = scores64(X, Y, bias if with_offsets else None, offset if with_offsets else None)
    elig = np.ones((NU, NI), bool)
    if with_exclude:
        elig[eu, ei] = False
    ids = np.arange(NI)
    out = {n: np.zeros(len(tu), np.int32) for n in ("above", "tied", "tied_before")}
    for p, (u, i) in enumerate(zip(tu, ti)):
        m = elig[u] & (ids != i)
        eq = m & (S[u] == S[u, i])
        out["above"][p] = np.sum(m & (S[u] > S[u, i]))
        out["tied"][p] = np.sum(eq)
        out["tied_before"][p] = np.sum(eq & (ids > i))
    out["score"] = S[tu, ti]
    out["n_eligible"] = elig.sum(axis=1).astype(np.int32)
    _freeze(*out.values())
    return out


def assert_counts_equal(got, want):
    for n in ("above", "tied", "tied_before", "n_eligible"):
        assert np.array_equal(got[n], want[n]), n
    assert np.array_equal(got["score"].view(np.int64), want["score"].view(np.int64)), "score bits"


def run_counts(k, rounded=True, with_exclude=True, with_offsets=False):
    from movie_recommender_amd.ranking import rank_counts
    X, Y, test, excl, bias, offset = fixture(k, rounded)
    return rank_counts(X, Y, test, excl if with_exclude else None,
                       bias if with_offsets else None, offset if with_offsets else None)


@pytest.mark.parametrize("k", KS)
def test_fixture_is_not_vacuous(k):
    _, _, (tu, ti), _, _, _ = fixture(k)
    ref, ref_all = reference(k), reference(k, with_exclude=False)
    mixed = int(np.sum((ref["tied_before"] > 0) & (ref["tied_before"] < ref["tied"])))
    changed = int(np.sum(ref["above"] != ref_all["above"]))
    print(f"k={k}: {len(tu)} pairs, tied>0 {int(np.sum(ref['tied'] > 0))}, mixed {mixed}, "
          f"exclusions change above for {changed}, min n_eligible {ref['n_eligible'].min()}")
    assert mixed >= 4
    assert changed > len(tu) / 2
    assert np.bincount(tu, minlength=NU).max() == 130
    assert np.bincount(tu, minlength=NU)[[0, 68, 69]].sum() == 0


# ---------------------------------------------------------------------------
# 1. counts and scores are equal to the restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("with_offsets", [False, True])
@pytest.mark.parametrize("with_exclude", [True, False])
@pytest.mark.parametrize("k", KS)
def test_counts_equal_restatement(gpu, k, with_exclude, with_offsets):
    got = run_counts(k, True, with_exclude, with_offsets)
    assert_counts_equal(got, reference(k, True, with_exclude, with_offsets))
    again = run_counts(k, True, with_exclude, with_offsets)
    for n in ("above", "tied", "tied_before", "n_eligible", "score"):
        assert np.array_equal(got[n], again[n]), n


# ---------------------------------------------------------------------------
# 2. factors that are not fp32 values: an FMA would change the bits
# ---------------------------------------------------------------------------
def test_counts_unrounded_factors(gpu):
    X, Y = fixture(20, False)[:2]
    assert np.any(X != X.astype(np.float32)) and np.any(Y != Y.astype(np.float32))
    for with_offsets in (False, True):
        assert_counts_equal(run_counts(20, False, True, with_offsets),
                            reference(20, False, True, with_offsets))


# ---------------------------------------------------------------------------
# 3. the position in MovieTable's top-N list
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_position_in_top_n_list(gpu, k):
    from movie_recommender_amd.serving import MovieTable
    X, Y, (tu, ti), (eu, ei), _, _ = fixture(k)
    got = run_counts(k)
    off = np.zeros(NU + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(eu, minlength=NU))
    order = np.argsort(eu, kind="stable")
    ids = {i: i for i in range(NI)}
    with MovieTable(k, Y.reshape(-1), ids, dict.fromkeys(ids, 0.0)) as table:
        mids, _, cnt = table.top_n_arrays(np.concatenate([X, np.zeros((NU, 1))], axis=1),
                                          (off, ei[order]), NI)
    assert np.array_equal(cnt, got["n_eligible"])
    pos = got["above"] + got["tied_before"]
    assert np.all(pos < cnt[tu])
    assert np.array_equal(mids[tu, pos], ti)
    assert np.sum(tu == 5) >= 1                      # the all-tied user is covered


# ---------------------------------------------------------------------------
# 4. metrics
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_metrics_on_gpu_counts(gpu, k):
    from movie_recommender_amd.ranking import metrics_from_counts, rank_eval
    X, Y, test, excl, _, _ = fixture(k)
    got = rank_eval(X, Y, test, excl, n=10)
    want = metrics_from_counts(reference(k), test[0], n=10)
    for n in ("mpr", "precision", "recall", "ndcg", "mrr", "hit_rate", "n_dropped", "n_pairs"):
        assert got[n] == want[n], n
    for n, a in want["per_user"].items():
        assert np.array_equal(got["per_user"][n], a), n
    print(f"k={k}: mpr {got['mpr']:.4f} precision {got['precision']:.4f} ndcg {got['ndcg']:.4f}")
    assert 0.4 < got["mpr"] < 0.6                    # random factors


# ---------------------------------------------------------------------------
# 5. refusals through the C ABI
# ---------------------------------------------------------------------------
def raw_counts(L, k, X, Y, toff, titem, eoff, eitem, n_users=NU, n_items=NI):
    from movie_recommender_amd import _lib
    n = max(len(titem), 1)
    out = {name: np.full(n, -7, np.int32) for name in ("above", "tied", "tied_before")}
    out["score"] = np.zeros(n)
    out["n_eligible"] = np.zeros(n_users, np.int32)
    ip, dp, llp = _lib.IP, _lib.DP, _lib.LLP
    rc = L.mr_rank_counts(0, k, n_users, n_items, X.ctypes.data_as(dp), None,
                          Y.ctypes.data_as(dp), None, toff.ctypes.data_as(llp),
                          titem.ctypes.data_as(ip),
                          eoff.ctypes.data_as(llp) if eoff is not None else None,
                          eitem.ctypes.data_as(ip) if eitem is not None else None,
                          out["above"].ctypes.data_as(ip), out["tied"].ctypes.data_as(ip),
                          out["tied_before"].ctypes.data_as(ip), out["score"].ctypes.data_as(dp),
                          out["n_eligible"].ctypes.data_as(ip), None)
    return rc, out


def csr_of(u, i):
    order = np.lexsort((i, u))
    off = np.zeros(NU + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(u, minlength=NU))
    return order, off, np.ascontiguousarray(i[order], np.int32)


def test_refusals_leave_the_library_usable(gpu):
    from movie_recommender_amd import _lib
    k = 20
    X, Y, (tu, ti), (eu, ei), _, _ = fixture(k)
    X, Y = np.ascontiguousarray(X), np.ascontiguousarray(Y)
    torder, toff, titem = csr_of(tu, ti)
    _, eoff, eitem = csr_of(eu, ei)
    want = reference(k)

    def valid_call_is_correct():
        rc, out = raw_counts(gpu, k, X, Y, toff, titem, eoff, eitem)
        assert rc == 0, _lib.last_error()
        for n in ("above", "tied", "tied_before"):
            assert np.array_equal(out[n], want[n][torder]), n
        assert np.array_equal(out["n_eligible"], want["n_eligible"])

    valid_call_is_correct()
    bad_item = titem.copy()
    bad_item[17] = NI
    neg_item = eitem.copy()
    neg_item[3] = -1
    dec_off = toff.copy()
    dec_off[10] = dec_off[9] - 1 if dec_off[9] > 0 else dec_off[11] + 1
    assert np.any(np.diff(dec_off) < 0)
    not_from_zero = eoff.copy()
    not_from_zero[0] = 1
    u_dup = int(np.flatnonzero(np.diff(eoff) >= 2)[0])
    dup = eitem.copy()
    dup[eoff[u_dup] + 1] = dup[eoff[u_dup]]
    u_both = int(np.flatnonzero((np.diff(eoff) >= 1) & (np.diff(toff) >= 1))[0])
    both = titem.copy()
    both[toff[u_both]] = eitem[eoff[u_both]]
    cases = {
        "test id out of range": (k, toff, bad_item, eoff, eitem, "out of range"),
        "excluded id negative": (k, toff, titem, eoff, neg_item, "out of range"),
        "decreasing offsets": (k, dec_off, titem, eoff, eitem, "offsets"),
        "offsets not from 0": (k, toff, titem, not_from_zero, eitem, "offsets"),
        "duplicate exclusion": (k, toff, titem, eoff, dup, "duplicate"),
        "test item excluded": (k, toff, both, eoff, eitem, "also excluded"),
        "k = 0": (0, toff, titem, eoff, eitem, "1..512"),
        "k = 513": (513, toff, titem, eoff, eitem, "1..512"),
    }
    for name, (kk, to, tit, eo, eit, word) in cases.items():
        rc, out = raw_counts(gpu, kk, X, Y, to, tit, eo, eit)
        assert rc == -1, name
        assert word in _lib.last_error(), (name, _lib.last_error())
        assert np.all(out["above"] == -7), name        # a refused call writes nothing
        valid_call_is_correct()


# ---------------------------------------------------------------------------
# the work division: every path of the count kernel gives the same counts
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("tuning", [(0, 1, 0),      # one block walks both item tiles
                                    (0, 1, 64),     # ... and only the users inside the first
                                                    # 64 pair slots of a tile are searched in
                                                    # LDS: user 1 (130 pairs) and those after
                                                    # it take the compare path
                                    (0, 2, -1),     # every user on the compare path
                                    (32, 0, 0)])    # three launches of one user tile each
def test_work_division_paths(gpu, tuning):
    from movie_recommender_amd import _lib
    try:
        _lib.check(gpu.mr_rank_set_tuning(*tuning), "mr_rank_set_tuning")
        for with_exclude in (True, False):
            assert_counts_equal(run_counts(20, True, with_exclude),
                                reference(20, True, with_exclude))
    finally:
        _lib.check(gpu.mr_rank_set_tuning(0, 0, 0), "mr_rank_set_tuning")
    assert gpu.mr_rank_set_tuning(0, 0, 2049) == -1 and gpu.mr_rank_set_tuning(-1, 0, 0) == -1
    assert_counts_equal(run_counts(20), reference(20))


def test_counts_at_k_512(gpu):
    """The largest k (32 chunks of 16 factors), beyond the score table's 128."""
    from movie_recommender_amd.ranking import rank_counts
    rng = np.random.default_rng(512)
    X, Y = rng.uniform(-1, 1, (40, 512)), rng.uniform(-1, 1, (270, 512))
    tu, ti = rng.integers(0, 40, 60), rng.integers(0, 270, 60)
    got = rank_counts(X, Y, (tu, ti))
    S = scores64(X, Y)
    assert np.array_equal(got["score"].view(np.int64), S[tu, ti].view(np.int64))
    assert np.array_equal(got["above"], np.sum(S[tu] > S[tu, ti][:, None], axis=1))
    assert np.all(got["tied"] == 0) and np.all(got["n_eligible"] == 270)


# ---------------------------------------------------------------------------
# 6. fold-in against fp64 NumPy
# ---------------------------------------------------------------------------
FOLD_ALPHA = 8.0


@functools.lru_cache(maxsize=None)
def fold_fixture(k):
    rng = np.random.default_rng(900 + k)
    Y = rng.uniform(-1, 1, (NI, k)).astype(np.float32).astype(np.float64)
    Y[294:] = 0.0
    lists = []
    for M in (0, 1, 2, k - 1, k + 3, 200, 290):
        items = rng.choice(NI, M, replace=False)
        lists.append([(int(i), float(r)) for i, r in zip(items, rng.integers(1, 11, M) * 0.5)])
    lists.append([(int(i), 2.5) for i in range(294, NI)])          # only zero rows
    Y.setflags(write=False)
    return Y, lists


def fold_reference(Y, lst, reg, mode):
    k = Y.shape[1]
    G = Y.T @ Y
    c = np.zeros(k)
    for i, r in lst:
        w = FOLD_ALPHA * r
        G = G + w * np.outer(Y[i], Y[i])
        c = c + (1.0 + w) * Y[i]
    G = G + (reg * len(lst) if mode == "weighted" else reg) * np.eye(k)
    return G, c


@pytest.mark.parametrize("reg,mode", [(0.5, "constant"), (0.05, "weighted"), (0.0, "constant")])
@pytest.mark.parametrize("k", [5, 20, 64, 128])
def test_fold_in_vs_numpy(gpu, k, reg, mode):
    from movie_recommender_amd.implicit import fold_in
    Y, lists = fold_fixture(k)
    X, status = fold_in(Y, lists, FOLD_ALPHA, reg, mode)
    assert X.shape == (len(lists), k) and np.all(status == 1)
    off = np.zeros(len(lists) + 1, np.int64)
    off[1:] = np.cumsum([len(l) for l in lists])
    X2, status2 = fold_in(Y, (off, np.array([i for l in lists for i, _ in l], np.int64),
                              np.array([r for l in lists for _, r in l])), FOLD_ALPHA, reg, mode)
    assert np.array_equal(X, X2) and np.array_equal(status, status2)   # CSR input, same bits
    worst = 0.0
    for u, lst in enumerate(lists):
        if len(lst) == 0 or all(i >= 294 for i, _ in lst):
            assert np.all(X[u] == 0.0), u
            continue
        G, c = fold_reference(Y, lst, reg, mode)
        ref = np.linalg.solve(G, c)
        bound = 8 * (k + len(lst)) * EPS * np.linalg.cond(G) * np.max(np.abs(ref))
        err = np.max(np.abs(X[u] - ref))
        worst = max(worst, err / bound)
        assert err <= bound, (u, len(lst), err, bound)
    print(f"k={k} reg={reg} {mode}: worst error / bound {worst:.3e}")


def test_fold_in_reports_a_non_positive_pivot(gpu):
    """reg = 0 and an item table of rank 1 in numbers that are exact in
    binary: G = 4 [[1, 1], [1, 1]], the first pivot is 4 and the second is
    4 - 2 * 2 = 0 exactly."""
    from movie_recommender_amd.implicit import fold_in
    Y = np.ones((2, 2))
    X, status = fold_in(Y, [[(0, 2.0)], [], [(1, 2.0)]], 1.0, 0.0, "constant")
    assert status.tolist() == [0, 1, 0] and np.all(X == 0.0)
    X, status = fold_in(Y, [[(0, 2.0)]], 1.0, 0.5, "constant")
    assert status.tolist() == [1]
    ref = np.linalg.solve(np.array([[4.5, 4.0], [4.0, 4.5]]), [3.0, 3.0])
    assert np.max(np.abs(X[0] - ref)) <= 1e-14


# ---------------------------------------------------------------------------
# 7. fold-in against the engine's own user half-step
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 20])
def test_fold_in_vs_engine(gpu, k):
    from movie_recommender_amd.engine import AlsContext
    from movie_recommender_amd.implicit import fold_in
    import test_gpu_implicit as T
    u, i, r, U0, V0 = T.fixture(k)
    with AlsContext(u, i, r, k, T.NU, T.NI, solver="cholesky", reg=0.5, reg_mode="constant",
                    implicit_alpha=T.ALPHA) as ctx:
        ctx.set_factors(U0, V0)
        ctx.iterate(3)
        ctx.half_step("users")
        U, V = ctx.get_factors()
    Xe, Ye = T.tables(U, V, k)
    lists = [[] for _ in range(T.NU)]
    for uu, ii, rr in zip(u, i, T.r32_of(r)):
        lists[uu].append((int(ii), float(rr)))
    X, status = fold_in(Ye, lists, T.ALPHA, 0.5, "constant")
    assert np.all(status == 1)
    print(f"k={k}: fold-in vs engine {rel_err(X, Xe):.3e}")
    assert rel_err(X, Xe) < 1e-4
    empty = np.array([len(l) == 0 for l in lists])
    assert empty.sum() == 2 and np.all(X[empty] == 0.0) and np.all(Xe[empty] == 0.0)


# ---------------------------------------------------------------------------
# 8. ImplicitModel end to end
# ---------------------------------------------------------------------------
def test_implicit_model_end_to_end(gpu):
    from movie_recommender_amd.implicit import ImplicitModel, als_implicit
    import test_gpu_implicit as T
    u, i, conf, nU, nI = T.planted()
    k = 8
    held = np.random.default_rng(11).random(len(u)) < 0.2
    tr = ~held
    X, Y, _, _ = als_implicit(u[tr], i[tr], conf[tr], k, nU, nI)
    rs = np.random.RandomState(0)                   # als_implicit's start
    X0 = rs.uniform(-1, 1, nU * (k + 1)).reshape(nU, k + 1)[:, :k]
    Y0 = rs.uniform(-1, 1, nI * k).reshape(nI, k)
    test, excl = (u[held], i[held]), (u[tr], i[tr])
    with ImplicitModel(X, Y) as model, ImplicitModel(X0, Y0) as start:
        ev, ev0 = model.rank_eval(test, excl, n=10), start.rank_eval(test, excl, n=10)
        print(f"mpr {ev['mpr']:.4f} (start {ev0['mpr']:.4f}) ndcg@10 {ev['ndcg']:.4f} "
              f"recall@10 {ev['recall']:.4f}")
        assert ev["mpr"] < 0.5 and ev["mpr"] < ev0["mpr"]
        assert ev["n_dropped"] == 0 and ev["n_pairs"] == int(held.sum())
        usr = int(np.argmax(np.bincount(u[tr], minlength=nU)))
        rated = i[tr][u[tr] == usr]
        x, status = model.fold_in([list(zip(rated.tolist(), conf[tr][u[tr] == usr].tolist()))])
        assert status[0] == 1
        top = model.top_n(x, [set(rated.tolist())], 20)[0]
        assert len(top) == 20 and not set(m for _, m in top) & set(rated.tolist())
        sc = [s for s, _ in top]
        assert sc == sorted(sc, reverse=True)
