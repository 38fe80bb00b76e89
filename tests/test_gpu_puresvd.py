"""GPU: PureSVD -- the truncated SVD of a zero-filled rating matrix as a factor
model on the serving kernels -- against NumPy: the item subspace, the user
factors, the scores in the serving order, the ranking, and ``refit``."""
import math

import numpy as np
import pytest

import svds_cases as S
from movie_recommender_amd.puresvd import PureSVD
from movie_recommender_amd.svds import svds

pytestmark = pytest.mark.gpu

USERS, ITEMS = 60, 45


def ratings(seed=21):
    rng = np.random.default_rng(seed)
    mask = rng.random((USERS, ITEMS)) < 0.3
    uid, iid = np.nonzero(mask)
    order = rng.permutation(len(uid))          # not sorted by user
    uid, iid = uid[order], iid[order]
    r = rng.choice(S.HALF_STARS, len(uid))
    return uid, iid, r


def dense(uid, iid, r):
    R = np.zeros((USERS, ITEMS))
    R[uid, iid] = r
    return R


MOVIE_IDS = [1000 + 7 * i for i in range(ITEMS)]


def serving_scores(X, Qf):
    """s = 0; s += x_i * v_i with separately rounded multiply and add."""
    s = np.zeros((X.shape[0], Qf.shape[0]))
    for i in range(Qf.shape[1]):
        s = s + X[:, i:i + 1] * Qf[:, i][None, :]
    return s


@pytest.mark.parametrize("k", [5, 16])
def test_puresvd_against_numpy(k):
    uid, iid, r = ratings()
    R = dense(uid, iid, r)
    svd = np.linalg.svd(R, full_matrices=False)
    assert S.gap_of(svd[1], k) >= S.MIN_GAP
    with PureSVD(uid, iid, r, USERS, ITEMS, k, movie_ids=MOVIE_IDS) as m:
        Qf = m.item_factors
        assert Qf.shape == (ITEMS, k) and m.singular_values.shape == (k,)
        assert np.all(np.diff(m.singular_values) <= 0)
        # the item factors span numpy's right singular subspace (Wedin, bound 5)
        res = np.sqrt(np.sum((R.T @ (R @ Qf) - Qf * m.singular_values[None, :] ** 2) ** 2, axis=0))
        resid = float(np.max(res / np.maximum(m.singular_values, 1e-300)))
        Vk = svd[2][:k].T
        sin_t = float(np.linalg.norm(Qf - Vk @ (Vk.T @ Qf), 2))
        gap = S.gap_of(svd[1], k) * svd[1][0]
        print("puresvd", k, "residual", resid, "sin", sin_t, "gap", gap)
        assert sin_t <= 4 * resid / gap
        lists = [[(MOVIE_IDS[i], float(R[u, i])) for i in np.nonzero(R[u])[0]]
                 for u in range(0, USERS, 7)] + [[]]
        rows = list(range(0, USERS, 7))
        X = m.user_factors(lists)
        want = R[rows] @ Qf
        assert np.max(np.abs(X[:-1] - want)) <= 1e-13 * np.max(np.abs(want))
        assert np.array_equal(X[-1], np.zeros(k))
        Xb = np.zeros((len(lists), k + 1))
        Xb[:, :k] = X
        sc = m.table().scores(Xb)
        ref = serving_scores(X, Qf)
        assert np.array_equal(sc, ref)
        got = m.recommend(lists, 10)
        for u, lst in enumerate(lists):
            rated = {mid for mid, _ in lst}
            ranked = sorted(((ref[u, i], MOVIE_IDS[i]) for i in range(ITEMS)
                             if MOVIE_IDS[i] not in rated), reverse=True)[:10]
            assert got[u] == ranked, u
        # the empty list scores 0 everywhere: ties by movie id descending
        assert [mid for _, mid in got[-1]] == sorted(MOVIE_IDS, reverse=True)[:10]


def test_refit_equals_a_fresh_model():
    uid, iid, r = ratings()
    r2 = np.random.default_rng(4).permutation(r)
    with PureSVD(uid, iid, r, USERS, ITEMS, 5) as m, PureSVD(uid, iid, r2, USERS, ITEMS, 5) as f:
        first = m.item_factors.copy()
        m.refit(r2)
        assert np.array_equal(m.item_factors, f.item_factors)
        assert np.array_equal(m.singular_values, f.singular_values)
        assert not np.array_equal(first, m.item_factors)
        top = m.recommend([[(3, 4.0), (9, 2.5)]], 5)
        assert top == f.recommend([[(3, 4.0), (9, 2.5)]], 5)


def test_k_above_the_serving_limit_is_refused_by_the_table_only():
    rng = np.random.default_rng(8)
    n = 140
    mask = rng.random((n, n)) < 0.2
    uid, iid = np.nonzero(mask)
    r = rng.choice(S.HALF_STARS, len(uid))
    with PureSVD(uid, iid, r, n, n, 129, ncv=n) as m:
        assert m.item_factors.shape == (n, 129)
        R = np.zeros((n, n))
        R[uid, iid] = r
        s_np = np.linalg.svd(R, compute_uv=False)
        assert np.max(np.abs(m.singular_values - s_np[:129])) <= (
            math.sqrt(2) * 4 * 8 * n * S.EPS * s_np[0] + 4 * math.sqrt(2 * n) * S.EPS * s_np[0])
        with pytest.raises(ValueError, match=r"rec: k must be in 1\.\.128"):
            m.table()
        with pytest.raises(ValueError, match=r"rec: k must be in 1\.\.128"):
            m.recommend([[(0, 1.0)]], 3)
    s = svds((np.arange(n + 1) * 0, np.zeros(0, int), np.zeros(0), n), k=129, ncv=n,
             return_singular_vectors=False)
    assert np.array_equal(s, np.zeros(129))
