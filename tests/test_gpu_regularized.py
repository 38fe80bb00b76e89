"""GPU: regularised ALS -- the ridge pass on the tri16 normal equations, the
regularised CG and Cholesky half-steps, the device objective and held-out
error -- against NumPy restatements composed from oracle.als_oracle.

Common fixture (the one of test_gpu_parity.test_cg_iterations_vs_oracle):
90 users x 70 items, 6,000 draws de-duplicated, the last 2 users and the last
item empty, zipf item ids (a few heavy items), normal ratings, fp32-rounded
uniform(-1, 1) factors.  The k values each pick a layout / kernel path:
5 VALU NB = 1, 20 VALU padded, 40 MFMA NB = 3 (unfolded last diagonal block),
64 MFMA NB = 4, 128 pair-of-waves, 144 streamed large-k.
"""
import functools
import os
import pickle

import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu

NU, NI = 90, 70
MIN_CHUNK = 64   # the smallest Gram chunk the engine accepts (mr_set_gram_chunk)


@functools.lru_cache(maxsize=None)
def fixture(k):
    rng = np.random.default_rng(100 + k)
    n = 6000
    u = rng.integers(0, NU - 2, n).astype(np.int32)       # last 2 users: no ratings
    i = (rng.zipf(1.3, n) % (NI - 1)).astype(np.int32)    # heavy items, last item empty
    key = np.unique(u.astype(np.int64) * NI + i)
    u = (key // NI).astype(np.int32)
    i = (key % NI).astype(np.int32)
    r = rng.normal(0, 1, len(u))
    U0 = rng.uniform(-1, 1, NU * (k + 1)).astype(np.float32).astype(np.float64)
    V0 = rng.uniform(-1, 1, NI * k).astype(np.float32).astype(np.float64)
    for a in (u, i, r, U0, V0):
        a.setflags(write=False)
    return u, i, r, U0, V0


def counts(u, i):
    return {"users": np.bincount(u, minlength=NU), "items": np.bincount(i, minlength=NI)}


def weights(cnt, mode):
    return cnt if mode == "weighted" else np.ones_like(cnt)


def ridge_expected(G0, k, lam, w):
    """G0 (fp32 values held in fp64) with each of the first k diagonal entries
    replaced by np.float32(np.float64(G0_ii) + lam * w_e)."""
    G = G0.copy()
    for d in range(k):
        G[:, d, d] = (G0[:, d, d] + lam * w).astype(np.float32).astype(np.float64)
    return G


def reset_chunk():
    from movie_recommender_amd import _lib
    _lib.check(_lib.lib().mr_set_gram_chunk(2048), "reset chunk")


# ---------------------------------------------------------------------------
# 1. the ridge pass is exact
# ---------------------------------------------------------------------------
def _ridge_case(k, mode, chunk):
    from movie_recommender_amd.engine import AlsContext
    u, i, r, U0, V0 = fixture(k)
    lam = 0.3
    cnt = counts(u, i)
    try:
        with AlsContext(u, i, r, k, NU, NI, gram_chunk=chunk) as ctx:
            ctx.set_factors(U0, V0)
            if chunk is not None:   # the heavy items go through slab_reduce
                assert (ctx.layout("items")[3][3] >= 0).sum() >= 2, "no split item"
            for side, nE in (("users", NU), ("items", NI)):
                ents = np.arange(nE)
                ctx.set_regularization(0.0, mode)
                ctx.build_normal_equations(side)
                G0, c0 = ctx.normal_equations(side, ents)
                ctx.set_regularization(lam, mode)
                ctx.build_normal_equations(side)
                G1, c1 = ctx.normal_equations(side, ents)
                w = weights(cnt[side], mode)
                # c, every off-diagonal entry, the bias row / column / corner:
                # bitwise; every diagonal entry i < k: one rounding
                assert np.array_equal(c1, c0), side
                assert np.array_equal(G1, ridge_expected(G0, k, lam, w)), side
                assert not np.array_equal(G1, G0)
                # an empty entity: untouched when weighted, lam on its diagonal
                # (and nothing else) when constant
                assert cnt[side][-1] == 0 and np.all(G0[-1] == 0)
                want = np.zeros_like(G0[-1])
                if mode == "constant":
                    want[np.arange(k), np.arange(k)] = np.float64(np.float32(lam))
                assert np.array_equal(G1[-1], want), side
    finally:
        if chunk is not None:
            reset_chunk()


@pytest.mark.parametrize("mode", ["weighted", "constant"])
@pytest.mark.parametrize("k", [5, 20, 40, 64, 128, 144])
def test_ridge_pass_exact(gpu, k, mode):
    _ridge_case(k, mode, None)


@pytest.mark.parametrize("mode", ["weighted", "constant"])
def test_ridge_pass_exact_after_slab_reduce(gpu, mode):
    """k = 64 with the smallest Gram chunk the engine accepts (64 ratings;
    mr_set_gram_chunk refuses less), so the heavy items' normal
    equations are summed by slab_reduce before the pass (no user of this
    fixture has more than 64 ratings)."""
    _ridge_case(64, mode, MIN_CHUNK)


# ---------------------------------------------------------------------------
# 2. shard offset
# ---------------------------------------------------------------------------
def test_ridge_pass_on_a_shard(gpu):
    from movie_recommender_amd.engine import AlsContext
    from movie_recommender_amd import distributed
    k = 64
    u, i, r, U0, V0 = fixture(k)
    (u0, u1), (i0, i1), uv, iv, _, _ = distributed.shard_views(u, i, r, NU, NI, 1, 3, k=k)
    assert 0 < u0 < u1 < NU and 0 < i0 < i1 < NI
    with AlsContext(u, i, r, k, NU, NI, reg=0.3, reg_mode="weighted") as full, \
            AlsContext(uv[0], uv[1], uv[2], k, NU, NI, user_range=(u0, u1), item_range=(i0, i1),
                       item_view=iv, reg=0.3, reg_mode="weighted") as shard:
        for ctx in (full, shard):
            ctx.set_factors(U0, V0)
        for side, (a, b) in (("users", (u0, u1)), ("items", (i0, i1))):
            full.build_normal_equations(side)
            shard.build_normal_equations(side)
            Gf, cf = full.normal_equations(side, np.arange(a, b))
            Gs, cs = shard.normal_equations(side, np.arange(b - a))
            assert np.array_equal(Gs, Gf) and np.array_equal(cs, cf), side
            # and they are regularised: the diagonal carries 0.3 n_e
            cnt = counts(u, i)[side][a:b]
            full.set_regularization(0.0, "weighted")
            full.build_normal_equations(side)
            G0, _ = full.normal_equations(side, np.arange(a, b))
            full.set_regularization(0.3, "weighted")
            assert np.array_equal(Gs, ridge_expected(G0, k, 0.3, cnt)), side


# ---------------------------------------------------------------------------
# 3. regularised CG against the oracle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("onepass", [1, 0])
@pytest.mark.parametrize("k", [5, 40, 64, 128, 144])
def test_regularized_cg_vs_oracle(gpu, k, onepass):
    """The body of test_cg_iterations_vs_oracle with lambda = 0.05 weighted and
    fuse_start left at 1: the oracle's fp64 CG runs on the GPU's own
    REGULARISED normal equations, so equal counts, rr, x and r0 also prove
    that the engine took the unfused start (a fused start would have formed
    r0 from the unregularised accumulators).  Tolerances are that test's."""
    from movie_recommender_amd.engine import AlsContext
    from oracle import als_oracle as O
    u, i, r, U0, V0 = fixture(k)
    lam = 0.05
    cnt = counts(u, i)
    with AlsContext(u, i, r, k, NU, NI, reg=lam, reg_mode="weighted") as ctx:
        ctx.set_option("fuse_start", 1)
        ctx.set_option("cg_onepass", onepass)
        for side, nE in (("users", NU), ("items", NI)):
            ctx.set_factors(U0, V0)
            ctx.build_normal_equations(side)
            G, c = ctx.normal_equations(side, np.arange(nE))
            # the G read back is the regularised one
            ctx.set_regularization(0.0, "weighted")
            ctx.build_normal_equations(side)
            G0, _ = ctx.normal_equations(side, np.arange(nE))
            ctx.set_regularization(lam, "weighted")
            assert np.array_equal(G, ridge_expected(G0, k, lam, cnt[side]))
            x0 = (U0 if side == "users" else V0).astype(np.float32)
            r0 = np.einsum("eij,ej->ei", G, x0.astype(np.float64).reshape(nE, -1)).ravel() \
                - c.ravel()
            for m in (0, 1, 2, 4):
                ctx.set_factors(U0, V0)
                its, rr = ctx.half_step(side, 0.01, m)
                U, V = ctx.get_factors()
                if m == 0:
                    rv, pv, _ = ctx.cg_vectors(side)
                    sc = np.max(np.abs(r0))
                    assert np.max(np.abs(rv - r0)) <= 1e-13 * sc, np.max(np.abs(rv - r0)) / sc
                    assert np.array_equal(pv, -rv)
                x = x0.copy()
                ito, rro = O.cg_blocks(G, c, x, 0.01, m)
                got = U if side == "users" else V
                assert its == ito, (side, m, its, ito)
                assert abs(rr - rro) <= 1e-10 * abs(rro), (side, m, rr, rro)
                step = np.max(np.abs(x.astype(np.float64) - x0))
                assert np.max(np.abs(got - x)) <= 1e-9 * step + 2 * np.spacing(np.float32(1)), \
                    (side, m, np.max(np.abs(got - x)), step)


# ---------------------------------------------------------------------------
# 4. resident == launch-per-iteration with lambda > 0
# ---------------------------------------------------------------------------
def test_regularized_resident_equals_per_iteration(gpu):
    from movie_recommender_amd.engine import AlsContext
    k = 64
    u, i, r, U0, V0 = fixture(k)
    outs = []
    for res in (1, 0):
        with AlsContext(u, i, r, k, NU, NI, reg=0.05, reg_mode="weighted", timing=True) as ctx:
            ctx.set_option("cg_resident", res)
            ctx.set_factors(U0, V0)
            ctx.iterate(2)
            outs.append((ctx.get_factors(), ctx.stats()))
    ((Ua, Va), sa), ((Ub, Vb), sb) = outs
    assert sa["kernel_launches"]["resident_users"] > 0
    assert sb["kernel_launches"]["resident_users"] == 0
    assert np.array_equal(Ua, Ub) and np.array_equal(Va, Vb)
    assert (sa["cg_users_total"], sa["cg_items_total"]) == (sb["cg_users_total"],
                                                            sb["cg_items_total"])
    for s in (sa, sb):   # one pass per half-step
        assert s["kernel_launches"]["regularize"] == 4


# ---------------------------------------------------------------------------
# 5. regularised exact solve
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 40, 64, 128])
def test_regularized_exact_solve(gpu, k):
    """After build_normal_equations and one Cholesky half-step every entity's
    x is the fp64 np.linalg.solve of the GPU's own regularised (G, c) to 1e-5
    relative: fp32 storage of x is 6e-8, the fp64 solve error about cond x
    1e-16 with cond <= 1e6 (asserted here on the host).

    The fixture's empty entities (2 users, 1 item) have w_e = 0 in the
    weighted mode: their G stays zero, no solve exists for them and the
    engine counts them as non-PD and keeps their x.  So the check reads:
    every entity WITH ratings is solved (nonpd_* equals the number of empty
    entities exactly) and matches np.linalg.solve; every empty one keeps its
    x bitwise.

    k = 128: every user has fewer than 129 ratings, so every unregularised
    user block is singular (asserted on the host); the same call with
    lambda = 0 reports nonpd_users > 0."""
    from movie_recommender_amd.engine import AlsContext
    u, i, r, U0, V0 = fixture(k)
    cnt = counts(u, i)
    with AlsContext(u, i, r, k, NU, NI, solver="cholesky", reg=0.1, reg_mode="weighted") as ctx:
        for side, nE, K in (("users", NU, k + 1), ("items", NI, k)):
            ctx.set_factors(U0, V0)
            ctx.reset_stats()
            ctx.build_normal_equations(side)
            G, c = ctx.normal_equations(side, np.arange(nE))
            ctx.half_step(side)
            U, V = ctx.get_factors()
            st = ctx.stats()
            x = (U if side == "users" else V).reshape(nE, K)
            x0 = (U0 if side == "users" else V0).reshape(nE, K)
            empty = cnt[side] == 0
            assert st["nonpd_" + side] == int(empty.sum()), (side, st)
            assert np.array_equal(x[empty], x0[empty])
            worst = 0.0
            for e in np.flatnonzero(~empty):
                assert np.linalg.cond(G[e]) <= 1e6, (side, e, np.linalg.cond(G[e]))
                xs = np.linalg.solve(G[e], c[e])
                worst = max(worst, np.max(np.abs(x[e] - xs)) / np.max(np.abs(xs)))
            print(f"k={k} {side}: worst relative error {worst:.3e}")
            assert worst <= 1e-5, (side, worst)
    if k == 128:
        assert cnt["users"].max() < 129
        with AlsContext(u, i, r, k, NU, NI, solver="cholesky") as ctx:
            ctx.set_factors(U0, V0)
            ctx.half_step("users")
            st = ctx.stats()
        print("k=128, lambda=0: nonpd_users", st["nonpd_users"], "of", NU)
        assert st["nonpd_users"] > 0


@pytest.mark.parametrize("k", [10, 64])
def test_regularized_cholesky_loop_vs_oracle(gpu, k):
    """Two exact ALS-WR iterations against the oracle's exact solve on its own
    fp64 normal equations with lambda n_e added to the first k diagonal
    entries; 1e-4 as test_cholesky_mode_vs_oracle holds on this fixture with
    a weaker constant ridge."""
    from movie_recommender_amd.engine import AlsContext
    from movie_recommender_amd import synth
    from oracle import als_oracle as O
    nU, nI, lam = 150, 120, 0.1
    u, i, r, *_ = synth.dense_fixture(nU, nI, k, 0.9, seed=k)
    rng = np.random.RandomState(2)
    U0 = rng.uniform(-1, 1, nU * (k + 1))
    V0 = rng.uniform(-1, 1, nI * k)
    with AlsContext(u, i, r, k, nU, nI, solver="cholesky", reg=lam, reg_mode="weighted") as ctx:
        ctx.set_factors(U0, V0)
        ctx.iterate(2)
        U, V = ctx.get_factors()
        st = ctx.stats()
    assert st["nonpd_users"] == 0 and st["nonpd_items"] == 0
    nu = np.bincount(u, minlength=nU)
    ni = np.bincount(i, minlength=nI)
    Uo, Vo = U0.copy(), V0.copy()
    d = np.arange(k)
    for _ in range(2):
        G, c = O.gram_user(u, i, r, Vo, k, nU)
        G[:, d, d] += lam * nu[:, None]
        assert O.solve_blocks(G, c, Uo) == 0
        G, c = O.gram_item(u, i, r, Uo, k, nI)
        G[:, d, d] += lam * ni[:, None]
        assert O.solve_blocks(G, c, Vo) == 0
    print(f"k={k}: relU {rel_err(U, Uo):.3e} relV {rel_err(V, Vo):.3e}")
    assert rel_err(U, Uo) < 1e-4 and rel_err(V, Vo) < 1e-4


# ---------------------------------------------------------------------------
# 6. objective and held-out error
# ---------------------------------------------------------------------------
def _close(a, b, tol=1e-12):
    return abs(a - b) <= tol * abs(b)


@pytest.mark.parametrize("k", [5, 64, 144])
def test_objective_and_sse(gpu, k):
    """objective() and sse() against NumPy fp64 on the same inputs to 1e-12
    relative: only the summation order differs (6,000 terms x 1e-16).  The
    same inputs are the fp32-rounded factors and, for objective(), the ratings
    as the context holds them -- its CSR stores them in fp32 -- while sse()
    takes the caller's fp64 ratings as they are.

    With the smallest Gram chunk the engine accepts (64) sse() is bitwise the
    default-chunk value (it does not walk the work list).  objective()'s
    training sse walks the users' work list, so where the chunk changes that
    list a user's ratings land in other waves and blocks and the fp64
    partials are added in another order: 1e-12 there (users that really are
    split: test_objective_with_split_users)."""
    from movie_recommender_amd.engine import AlsContext
    from oracle import als_oracle as O
    u, i, r, U0, V0 = fixture(k)
    cnt = counts(u, i)
    pred = O.predict(U0, V0, u, i, k)
    r32 = r.astype(np.float32).astype(np.float64)
    sse_train = float(np.sum((r32 - pred) ** 2))
    sse_host = float(np.sum((r - pred) ** 2))
    Um = U0.reshape(NU, k + 1)[:, :k]
    Vm = V0.reshape(NI, k)
    lam = 0.05
    with AlsContext(u, i, r, k, NU, NI) as ctx:
        ctx.set_factors(U0, V0)
        for mode in ("weighted", "constant"):
            ctx.set_regularization(lam, mode)
            o1, o2 = ctx.objective(), ctx.objective()
            assert o1 == o2                                  # identical bits
            assert o1["n"] == len(u) and o1["lam"] == lam
            pu = float(np.sum(weights(cnt["users"], mode) * np.sum(Um * Um, axis=1)))
            pi = float(np.sum(weights(cnt["items"], mode) * np.sum(Vm * Vm, axis=1)))
            assert _close(o1["sse"], sse_train), (o1["sse"], sse_train)
            assert _close(o1["pen_users"], pu) and _close(o1["pen_items"], pi), (o1, pu, pi)
            assert o1["J"] == o1["sse"] + lam * (o1["pen_users"] + o1["pen_items"])
        s1, s2 = ctx.sse(u, i, r), ctx.sse(u, i, r)
        assert s1 == s2 and s1[1] == len(u)
        assert _close(s1[0], sse_host), (s1, sse_host)
        assert _close(ctx.rmse(u, i, r), np.sqrt(sse_host / len(u)))
        # a held-out set that is not the training set, odd length
        hu, hi, hr = u[::7][:-1].copy(), i[::-1][::7][:-1].copy(), r[::7][:-1] + 0.25
        want = float(np.sum((hr - O.predict(U0, V0, hu, hi, k)) ** 2))
        got = ctx.sse(hu, hi, hr)
        assert got[1] == len(hu) and _close(got[0], want), (got, want)
        assert ctx.sse(hu[:0], hi[:0], hr[:0]) == (0.0, 0)
        # a bad id raises and the context stays usable
        for bu, bi in ((NU, 0), (0, NI), (-1, 0)):
            with pytest.raises(RuntimeError, match="out of range"):
                ctx.sse([0, bu], [0, bi], [1.0, 1.0])
        assert ctx.sse(u, i, r) == s1 and ctx.objective() == o1
    try:
        with AlsContext(u, i, r, k, NU, NI, gram_chunk=MIN_CHUNK, reg=lam,
                        reg_mode="constant") as ctx:
            ctx.set_factors(U0, V0)
            assert ctx.sse(u, i, r) == s1
            o3 = ctx.objective()
            assert o3["n"] == len(u) and _close(o3["sse"], o1["sse"])
            assert o3["pen_users"] == o1["pen_users"] and o3["pen_items"] == o1["pen_items"]
    finally:
        reset_chunk()


def test_objective_with_split_users(gpu):
    """The common fixture with the roles swapped (70 users, the zipf ids: up
    to 88 ratings each; 90 items) at the smallest chunk: the heavy users are
    split across waves of the objective kernel, as in the Gram."""
    from movie_recommender_amd.engine import AlsContext
    from oracle import als_oracle as O
    k = 64
    i, u, r, V0, U0 = fixture(k)          # swapped: users <- items
    nU, nI = NI, NU
    U0 = np.concatenate([U0.reshape(nU, k), np.linspace(-1, 1, nU)[:, None]], axis=1) \
        .astype(np.float32).astype(np.float64).ravel()
    V0 = V0.reshape(nI, k + 1)[:, :k].ravel()
    order = np.argsort(u, kind="stable")
    u, i, r = u[order], i[order], r[order]
    r32 = r.astype(np.float32).astype(np.float64)
    want = float(np.sum((r32 - O.predict(U0, V0, u, i, k)) ** 2))
    pu = float(np.sum(np.bincount(u, minlength=nU) *
                      np.sum(U0.reshape(nU, k + 1)[:, :k] ** 2, axis=1)))
    res = []
    try:
        for chunk in (MIN_CHUNK, None):
            with AlsContext(u, i, r, k, nU, nI, gram_chunk=chunk) as ctx:
                split = int((ctx.layout("users")[3][3] >= 0).sum())
                assert (split >= 4) if chunk else (split == 0), split
                ctx.set_factors(U0, V0)
                o = ctx.objective()
                assert o == ctx.objective()
                assert o["n"] == len(u) and _close(o["sse"], want), (o, want)
                assert _close(o["pen_users"], pu)
                res.append((o, ctx.sse(u, i, r)))
    finally:
        reset_chunk()
    assert res[0][1] == res[1][1]
    assert res[0][0]["pen_users"] == res[1][0]["pen_users"]
    assert res[0][0]["pen_items"] == res[1][0]["pen_items"]


# ---------------------------------------------------------------------------
# 7. monotone objective
# ---------------------------------------------------------------------------
def test_objective_is_monotone_under_exact_half_steps(gpu):
    """Each Cholesky half-step minimises J exactly on its side (fp32 effects
    on a minimiser are second order): over 6 half-steps J never rises by
    more than 1e-6 relative, and ends below its start."""
    from movie_recommender_amd.engine import AlsContext
    from movie_recommender_amd import synth
    k, nU, nI = 10, 150, 120
    u, i, r, *_ = synth.dense_fixture(nU, nI, k, 0.9, seed=k)
    rng = np.random.RandomState(2)
    with AlsContext(u, i, r, k, nU, nI, solver="cholesky", reg=0.1, reg_mode="weighted") as ctx:
        ctx.set_factors(rng.uniform(-1, 1, nU * (k + 1)), rng.uniform(-1, 1, nI * k))
        J = [ctx.objective()["J"]]
        for h in range(6):
            ctx.half_step("users" if h % 2 == 0 else "items")
            J.append(ctx.objective()["J"])
    print("J per half-step:", J)
    for a, b in zip(J, J[1:]):
        assert b <= a * (1 + 1e-6), J
    assert J[-1] < J[0]


# ---------------------------------------------------------------------------
# 8. lambda = 0 is today's engine
# ---------------------------------------------------------------------------
def test_lambda_zero_is_the_unregularised_engine(gpu):
    from movie_recommender_amd.engine import AlsContext
    k = 64
    u, i, r, U0, V0 = fixture(k)
    outs = []
    for call in (False, True):
        with AlsContext(u, i, r, k, NU, NI, timing=True) as ctx:
            if call:
                ctx.set_regularization(0.0, "weighted")
            ctx.set_factors(U0, V0)
            ctx.iterate(2)
            outs.append((ctx.get_factors(), ctx.stats()))
    ((Ua, Va), sa), ((Ub, Vb), sb) = outs
    assert np.array_equal(Ua, Ub) and np.array_equal(Va, Vb)
    for s in (sa, sb):
        assert s["kernel_launches"]["regularize"] == 0
        assert s["kernel_ms"]["regularize"] == 0.0
    assert sa["kernel_launches"] == sb["kernel_launches"]


# ---------------------------------------------------------------------------
# the training driver
# ---------------------------------------------------------------------------
def test_als_train_regularized(gpu, tmp_path):
    """Reads and writes als_train's files, draws U0 then V0 from NumPy's
    global RNG, stops on J's relative decrease, returns J per iteration."""
    from movie_recommender_amd import train
    from movie_recommender_amd.engine import AlsContext
    k = 5
    u, i, r, _, _ = fixture(k)
    d = str(tmp_path)
    for name, obj in ((f"als{k}_movie_ids", list(range(NI))), (f"als{k}_user_ids", list(range(NU))),
                      (f"als{k}_user_ratings_train", [u, i, r])):
        with open(os.path.join(d, name + ".bin"), "wb") as f:
            pickle.dump(obj, f)
    np.random.seed(3)
    out = train.als_train_regularized([k], d, 0.1, max_iterations=4, tol=0.0, verbose=False)
    U, V, its, hist = out[k]
    assert its == 4 and len(hist) == 4 and all(b <= a * (1 + 1e-6) for a, b in zip(hist, hist[1:]))
    np.random.seed(3)
    U0 = np.random.uniform(-1, 1, NU * (k + 1))
    V0 = np.random.uniform(-1, 1, NI * k)
    with AlsContext(u, i, r, k, NU, NI, solver="cholesky", reg=0.1) as ctx:
        ctx.set_factors(U0, V0)
        ctx.iterate(4)
        Ue, Ve = ctx.get_factors()
        assert ctx.objective()["J"] == hist[-1]
    assert np.array_equal(U, Ue) and np.array_equal(V, Ve)
    for name, want in ((f"als{k}_user_factors", U), (f"als{k}_item_factors", V)):
        with open(os.path.join(d, name + ".bin"), "rb") as f:
            assert np.array_equal(pickle.load(f), want)
    # a loose tol stops early
    np.random.seed(3)
    early = train.als_train_regularized([k], d, 0.1, max_iterations=4, tol=0.5, verbose=False)
    assert early[k][2] < 4 and early[k][3] == hist[:early[k][2]]
