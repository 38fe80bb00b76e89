"""GPU: the scoring, exclusion, top-N select and evaluation kernels of
serving.hip at the paths and edges the fixture tests do not reach.

Everything asserted is exact: returned (score, movie id) lists equal
``exact_top_n(exact_scores(...))`` entry for entry, and scores are compared by
their bits.  The one exception is the evaluation's squared error (see
``test_evaluation_long_lists``).  Which path of the select an input takes is
pinned on the CPU by tests/test_serving_select_model.py."""
from fractions import Fraction

import numpy as np
import pytest

from oracle import serving_oracle as O
from serving_cases import (distinct_ids, exact_scores, exact_top_n, select_exclusions,
                           select_inputs, signs_input, synthetic_table, value_table)

pytestmark = pytest.mark.gpu

SELECT_INPUTS = select_inputs()


def bits(a):
    return np.asarray(a, np.float64).view(np.int64)


def movie_table(*args):
    from movie_recommender_amd.serving import MovieTable
    return MovieTable(*args)


def check_top_n(t, X, rated, N, S):
    """top-N of every user row of X against the exact order on S (the exact
    scores of X), ids equal and scores bit-equal."""
    cand = np.asarray(t.cand_mid)
    mids, sc, cnt = t.top_n_arrays(X, rated, N)
    for u in range(len(X)):
        ref = exact_top_n(S[u], cand, set(rated[u]) if rated is not None else set(), N)
        assert cnt[u] == len(ref), (u, N)
        assert mids[u, :cnt[u]].tolist() == [m for _, m in ref], (u, N)
        assert np.array_equal(bits(sc[u, :cnt[u]]), bits([s for s, _ in ref])), (u, N)
    return mids, sc, cnt


# -- 1. select paths ----------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SELECT_INPUTS))
def test_select_paths(gpu, name):
    """Radix levels with elements above, a digit across the key / id boundary,
    the fast path at its capacity, ids up to 2^31 - 2: users 0-2 with no
    exclusions, the head of the order excluded, fewer than N left; user 3
    negated, user 4 halved."""
    inp = SELECT_INPUTS[name]
    X = np.array([[1.0, 0.0]] * 3 + [[-1.0, 0.0], [0.5, 0.0]])
    rated = select_exclusions(inp) + [set(), set()]
    k, V, als_ids, med = value_table(inp["values"], inp["mids"])
    with movie_table(k, V, als_ids, med) as t:
        assert t.cand_mid.tolist() == [int(m) for m in inp["mids"]]
        S = exact_scores(X, V.reshape(-1, 1), t.cand_med)
        assert np.array_equal(bits(S[0]), bits(inp["values"]))
        for N in sorted({inp["N"], 1, 1024}):
            check_top_n(t, X, rated, N, S)
        check_top_n(t, X, None, inp["N"], S)


# -- 2. signs and zeros -------------------------------------------------------
def test_select_signs_and_zeros(gpu):
    """Keys of negative scores, of both zeros, and a range that spans the
    sign: among the zeros the order is by movie id, whatever the zero's sign."""
    inp = signs_input()
    v, mids = inp["values"], np.asarray(inp["mids"])
    X = np.array([[x0, 0.0] for x0, _ in inp["users"]])
    rated = [ex for _, ex in inp["users"]]
    k, V, als_ids, med = value_table(v, mids)
    with movie_table(k, V, als_ids, med) as t:
        S = exact_scores(X, V.reshape(-1, 1), t.cand_med)
        got = {N: check_top_n(t, X, rated, N, S) for N in (375, 400, 1024)}
    zero_ids = np.sort(mids[v == 0])[::-1]
    assert len(zero_ids) == 100
    m, sc, cnt = got[400]
    # user 2 (x0 = 0): only zeros, the 400 largest ids of the whole table
    assert m[2].tolist() == np.sort(mids)[::-1][:400].tolist() and not bits(sc[2]).any()
    # user 3: 350 positives, then the 50 zeros with the largest ids
    assert cnt[3] == 400 and np.all(sc[3, :350] > 0) and not bits(sc[3, 350:]).any()
    assert m[3, 350:].tolist() == zero_ids[:50].tolist()
    assert got[375][0][3, 350:].tolist() == zero_ids[:25].tolist()
    # user 4: 100 positives, all 100 zeros, then the negatives
    assert m[4, 100:200].tolist() == zero_ids.tolist() and np.all(sc[4, 200:] < 0)


# -- 3. row-length and N edges --------------------------------------------------
ROW_LENGTHS = (1, 64, 65, 512, 513, 1536, 1537, 2047, 2048, 2049, 3585, 4097)
EXCL_LENGTHS = (767, 768, 769, 1024, 1025)


@pytest.mark.parametrize("n_cand", ROW_LENGTHS)
def test_select_row_lengths(gpu, n_cand):
    """Rows at the boundaries of the four-deep unrolled passes (512 threads)
    and of the bitonic sizes, N = 1, 400 and 1,024 (more than a short row
    has): distinct scores, all scores equal, a third excluded; and exclusion
    lists (with duplicates) around the exclusion kernel's unrolled trip of
    4 x 256, with distinct and with all-equal scores."""
    rs = np.random.RandomState(n_cand)
    v = (rs.permutation(n_cand) - n_cand // 2) * 0.173 + rs.uniform(0.0, 0.1, n_cand)
    mids = distinct_ids(rs, n_cand, 2 ** 31 - 1)
    X = [[1.0, 0.0], [0.0, 0.0], [1.0, 0.0]]
    rated = [[], [], [int(m) for m in rs.permutation(mids)[:n_cand // 3]]]
    if n_cand >= 2047:
        for L in EXCL_LENGTHS:
            distinct = rs.permutation(mids)[:L - 10]
            lst = [int(m) for m in rs.permutation(np.concatenate([distinct, distinct[:10]]))]
            assert len(lst) == L
            X += [[1.0, 0.0], [0.0, 0.0]]
            rated += [lst, lst]
    X = np.array(X)
    k, V, als_ids, med = value_table(v, mids)
    with movie_table(k, V, als_ids, med) as t:
        S = exact_scores(X, V.reshape(-1, 1), t.cand_med)
        assert np.array_equal(bits(t.scores(X)), bits(S))
        for N in (1, 400, 1024):
            _, _, cnt = check_top_n(t, X, rated, N, S)
            assert cnt[0] == cnt[1] == min(N, n_cand)


def test_top_n_num_results_limits(gpu):
    k, V, als_ids, med = value_table(np.arange(5.0), np.arange(5) + 1)
    with movie_table(k, V, als_ids, med) as t:
        X = np.array([[1.0, 0.0]])
        for n in (0, 1025):
            with pytest.raises(RuntimeError, match="num_results"):
                t.top_n(X, None, n)
        assert t.top_n(X, None, 1024) == [[(4.0 - i, 5 - i) for i in range(5)]]


# -- 4. score tiles -------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 15, 16, 17, 33, 127, 128])
def test_score_tile_edges(gpu, k):
    """Every remainder of the 32-user x 256-candidate x 16-factor tiles, the
    all-off-by-one corners included: the whole score matrix is bit-equal (a
    store past a row's end would land in the next user's row), and the keyed
    variant of the kernel returns the same bits in the exact order."""
    rs = np.random.RandomState(100 + k)
    for n_cand in (1, 63, 255, 256, 257, 513):
        V = rs.normal(0, 0.6, (n_cand, k))
        ids = rs.permutation(np.arange(1, 3 * n_cand + 1))[:n_cand]
        als_ids = {int(m): j for j, m in enumerate(ids)}
        med = {int(m): float(rs.choice(np.arange(1, 11) / 2.0)) for m in rs.permutation(ids)}
        with movie_table(k, V.reshape(-1), als_ids, med) as t:
            cand = t.cand_mid.astype(np.int64)
            Vc = V[t.cand_als]
            for n_users in (1, 31, 32, 33, 65):
                X = rs.normal(0, 0.5, (n_users, k + 1))
                S = exact_scores(X, Vc, t.cand_med)
                assert np.array_equal(bits(t.scores(X)), bits(S)), (n_cand, n_users)
                mids, sc, cnt = t.top_n_arrays(X, None, min(n_cand, 1024))
                assert np.all(cnt == n_cand)
                for u in range(n_users):
                    order = np.lexsort((-cand, -S[u]))
                    assert np.array_equal(mids[u], cand[order]), (n_cand, n_users, u)
                    assert np.array_equal(bits(sc[u]), bits(S[u][order])), (n_cand, n_users, u)


# -- 5. user chunks -------------------------------------------------------------
def test_top_n_over_user_chunks(gpu):
    """More users than one device pass takes: the second chunk's model rows,
    exclusion lists (offsets rebased to the chunk) and output rows.  The
    arrays equal those of the two chunks run as calls of their own, and eight
    users are checked against the exact order."""
    k, n_cand, N = 2, 32768, 10
    rs = np.random.RandomState(41)
    V = rs.normal(0, 0.6, (n_cand, k))
    ids = distinct_ids(rs, n_cand, 2 ** 31 - 1)
    als_ids = {int(m): j for j, m in enumerate(ids)}
    med = {int(m): float(h) for m, h in zip(ids, rs.choice(np.arange(1, 11) / 2.0, n_cand))}
    with movie_table(k, V.reshape(-1), als_ids, med) as t:
        B = t.user_chunk
        assert B * n_cand * 8 <= 1 << 30          # the key scratch this test asks for
        n = B + 37
        assert n > B
        X = rs.normal(0, 0.5, (n, k + 1))
        # 0-5 exclusions per user, a quarter of them no candidates' ids; empty
        # lists at both ends of the first chunk; a long one opens the second
        lens = rs.randint(0, 6, n)
        lens[[0, B - 2]] = 0
        lens[B - 1] = 5
        lens[B] = 2000
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        ex = ids[rs.randint(0, n_cand, off[-1])]
        ex[rs.rand(len(ex)) < 0.25] = 2 ** 31 - 1
        cand = np.asarray(t.cand_mid)
        users = [0, B - 1, B, n - 1] + sorted(rs.choice(n, 4, replace=False).tolist())
        S8 = exact_scores(X[users], V[t.cand_als], t.cand_med)
        # the top ten of the second chunk's first user are among its exclusions
        lead = exact_top_n(S8[2], cand, set(), N)
        ex[off[B]:off[B] + N] = [m for _, m in lead]
        full = t.top_n_arrays(X, (off, ex), N)
        first = t.top_n_arrays(X[:B], (off[:B + 1], ex[:off[B]]), N)
        second = t.top_n_arrays(X[B:], (off[B:] - off[B], ex[off[B]:]), N)
    for a, b, c in zip(full, first, second):
        if a.dtype == np.float64:
            a, b, c = bits(a), bits(b), bits(c)
        assert np.array_equal(a, np.concatenate([b, c]))
    mids, sc, cnt = full
    assert np.all(cnt == N)
    for i, u in enumerate(users):
        ref = exact_top_n(S8[i], cand, set(ex[off[u]:off[u + 1]].tolist()), N)
        assert mids[u].tolist() == [m for _, m in ref], u
        assert np.array_equal(bits(sc[u]), bits([s for s, _ in ref])), u
    assert not set(mids[B].tolist()) & set(m for _, m in lead)


def test_scores_over_user_chunks(gpu):
    """``scores`` of more users than one device pass takes, seven base rows
    tiled: every row on either side of the boundary has its base row's bits."""
    k = 2
    V, als_ids, med = synthetic_table(k, 10, 0, seed=6, ties=1)
    rs = np.random.RandomState(8)
    X7 = rs.normal(0, 0.5, (7, k + 1))
    with movie_table(k, V, als_ids, med) as t:
        B = t.user_chunk
        n = B + 9
        assert n > B and n * 10 * 8 < 200 << 20
        base = t.scores(X7)
        assert np.array_equal(bits(base), bits(exact_scores(X7, V.reshape(-1, k)[t.cand_als],
                                                            t.cand_med)))
        big = t.scores(np.tile(X7, (n // 7 + 1, 1))[:n])
    assert big.shape == (n, 10)
    for r in range(7):
        assert np.all(big[r::7].view(np.int64) == bits(base[r])[None, :]), r


# -- 6. evaluation ----------------------------------------------------------------
def test_evaluation_long_lists(gpu):
    """Predictions made in the evaluation kernel on lists up to and beyond its
    1,024-rating pair chunk, mixed with ratings of movies that have no
    prediction.  pred, the pair counts, n_pred and the agreement are exact.
    sse is a sum of n positive terms accumulated with fma and reduced by a
    tree, any order of which is within n * 2^-52 relative of the exact sum
    (n - 1 roundings of at most 2^-53 each, first order, doubled); the exact
    sum of the squares is formed in rational arithmetic."""
    k = 5
    V, als_ids, med = synthetic_table(k, 3000, 300, seed=17, ties=50)
    rs = np.random.RandomState(18)
    cands = np.array([m for m in med if m in als_ids])
    others = np.concatenate([[m for m in med if m not in als_ids],
                             10 ** 7 + np.arange(3000)])
    half = np.arange(1, 11) / 2.0

    def mixed(n, p_other=1.0 / 7.0):
        other = rs.rand(n) < p_other
        m = np.where(other, rs.permutation(others)[:n], rs.permutation(cands)[:n])
        return [(int(a), float(r)) for a, r in zip(m, rs.choice(half, n))]

    lists = [mixed(0), mixed(1, 0.0), mixed(2, 0.0)] + [mixed(n) for n in (1023, 1024, 1025, 2500)]
    lists.append(mixed(1030, 1.0))                                  # nothing predictable
    one = mixed(1500, 1.0)
    one[1200] = (int(cands[5]), 4.0)                                # exactly one predictable
    lists.append(one)
    lists.append([(m, 3.5) for m, _ in mixed(1100)])                # all actual ratings equal
    U = rs.normal(0, 0.5, (6, k + 1))
    rows = rs.randint(0, 6, len(lists))
    with movie_table(k, V, als_ids, med) as t:
        res = t.evaluate(U.reshape(-1), rows, lists)
    pos = 0
    for i, l in enumerate(lists):
        p = np.array([np.nan if (s := O.predict(U[rows[i]], m, med, V, als_ids)) is None else s
                      for m, _ in l], np.float64).reshape(-1)
        a = np.array([r for _, r in l], np.float64)
        got = res["pred"][pos:pos + len(l)]
        pos += len(l)
        ok = ~np.isnan(p)
        assert np.array_equal(np.isnan(got), ~ok), i
        assert np.array_equal(bits(got[ok]), bits(p[ok])), i
        agree, dis = O.ranking_agreement_counts(a[ok], p[ok])
        assert (res["n_agree"][i], res["n_disagree"][i], res["n_pred"][i]) == \
            (agree, dis, int(ok.sum())), i
        if ok.sum() > 1 and agree + dis > 0:
            assert res["agreement"][i] == agree / (agree + dis), i
        else:
            assert np.isnan(res["agreement"][i]), i
        exact = sum(Fraction(float(d)) ** 2 for d in p[ok] - a[ok])
        sse = float(res["sse"][i])
        print(f"list {i}: n={len(l)} n_pred={int(ok.sum())} sse={sse!r} "
              f"rel_err={float(abs(Fraction(sse) - exact) / exact) if exact else 0.0:.3e}")
        assert abs(Fraction(sse) - exact) <= int(ok.sum()) * Fraction(1, 2 ** 52) * exact, i
    # the shapes the lists were made for
    npred = res["n_pred"]
    assert npred[0] == 0 and npred[1] == 1 and npred[2] == 2
    assert npred[7] == 0 and npred[8] == 1
    assert all(0 < npred[i] < len(lists[i]) for i in (3, 4, 5, 6, 9))
    assert npred[6] > 1024 and npred[9] > 1 and res["n_agree"][9] == res["n_disagree"][9] == 0
    assert np.isnan(res["agreement"][[0, 1, 7, 8, 9]]).all()
    assert not np.isnan(res["agreement"][[3, 4, 5, 6]]).any()
