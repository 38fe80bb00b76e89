"""GPU: implicit-feedback ALS (confidence 1 + alpha r, preference 1 for stored
pairs and 0 for all others, no user bias) against a NumPy fp64 restatement
that lives in this file.

Fixture: the one of test_gpu_regularized.py with non-negative ratings -- 90
users x 70 items, 6,000 draws de-duplicated, zipf item ids (a few heavy items),
the last 2 users and the last item empty, r in {0.5, 1, ..., 5}, fp32-rounded
uniform(-1, 1) factors.  alpha = 8 makes every w = alpha r and every 1 + w
exact in fp32 and in bf16.  The k values each pick a kernel path: 5 VALU NB = 1,
20 VALU padded, 40 matrix cores NB = 3 (unfolded last diagonal block), 64
NB = 4, 128 NB = 8.
"""
import functools

import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu

NU, NI = 90, 70
ALPHA = 8.0
MIN_CHUNK = 64
KS = [5, 20, 40, 64, 128]


@functools.lru_cache(maxsize=None)
def fixture(k, inexact=False):
    rng = np.random.default_rng(300 + k)
    n = 6000
    u = rng.integers(0, NU - 2, n).astype(np.int32)       # last 2 users: no ratings
    i = (rng.zipf(1.3, n) % (NI - 1)).astype(np.int32)    # heavy items, last item empty
    key = np.unique(u.astype(np.int64) * NI + i)
    u = (key // NI).astype(np.int32)
    i = (key % NI).astype(np.int32)
    r = rng.integers(1, 11, len(u)) * 0.5
    U0 = rng.uniform(-1, 1, NU * (k + 1)).astype(np.float32).astype(np.float64)
    V0 = rng.uniform(-1, 1, NI * k).astype(np.float32).astype(np.float64)
    if inexact:
        r = np.abs(rng.normal(0, 1, len(u)))
    U0.reshape(NU, k + 1)[:, k] = 0.0                      # the mode has no user bias
    for a in (u, i, r, U0, V0):
        a.setflags(write=False)
    return u, i, r, U0, V0


# ---------------------------------------------------------------------------
# the NumPy restatement (fp64)
# ---------------------------------------------------------------------------
def tables(U, V, k, nU=NU, nI=NI):
    return (np.asarray(U, np.float64).reshape(nU, k + 1)[:, :k],
            np.asarray(V, np.float64).reshape(nI, k))


def normal64(side, u, i, r, alpha, X, Y):
    """(G, c, S) of one side: G_e = S + sum w y y^T, c_e = sum (1 + w) y."""
    ent, oth, opp, nE = (u, i, Y, len(X)) if side == "users" else (i, u, X, len(Y))
    S = opp.T @ opp
    G = np.repeat(S[None], nE, axis=0)
    c = np.zeros((nE, opp.shape[1]))
    for e, j, rv in zip(ent, oth, r):
        w = alpha * rv
        G[e] += w * np.outer(opp[j], opp[j])
        c[e] += (1.0 + w) * opp[j]
    return G, c, S


def dense_loss(u, i, r, alpha, X, Y):
    """sum over ALL (u, i) of c_ui (p_ui - x_u . y_i)^2, formed densely."""
    C = np.ones((len(X), len(Y)))
    P = np.zeros((len(X), len(Y)))
    C[u, i] = 1.0 + alpha * r
    P[u, i] = 1.0
    return float(np.sum(C * (P - X @ Y.T) ** 2))


def als64(u, i, r, alpha, lam, X, Y, iterations):
    X, Y = X.copy(), Y.copy()
    k = X.shape[1]
    for _ in range(iterations):
        G, c, _ = normal64("users", u, i, r, alpha, X, Y)
        X = np.stack([np.linalg.solve(G[e] + lam * np.eye(k), c[e]) for e in range(len(X))])
        G, c, _ = normal64("items", u, i, r, alpha, X, Y)
        Y = np.stack([np.linalg.solve(G[e] + lam * np.eye(k), c[e]) for e in range(len(Y))])
    return X, Y


def r32_of(r):
    return np.asarray(r, np.float32).astype(np.float64)   # what the CSR holds


def reset_chunk():
    from movie_recommender_amd import _lib
    _lib.check(_lib.lib().mr_set_gram_chunk(2048), "reset chunk")


def check_normal(ctx, side, u, i, r, alpha, k, U, V):
    """The context's (G, c) of `side` at factors (U, V) against fp64 NumPy:
    the bound test_gram_kernel_vs_numpy holds the explicit Gram to."""
    X, Y = tables(U, V, k)
    nE = NU if side == "users" else NI
    G64, c64, S = normal64(side, u, i, r32_of(r), alpha, X, Y)
    ctx.build_normal_equations(side)
    G, c = ctx.normal_equations(side, np.arange(nE))
    worst_g = worst_c = 0.0
    for e in range(nE):
        worst_g = max(worst_g, np.max(np.abs(G[e, :k, :k] - G64[e])) / np.max(np.abs(G64[e])))
        worst_c = max(worst_c, np.max(np.abs(c[e, :k] - c64[e])) / max(np.max(np.abs(c64[e])), 1))
    print(f"k={k} {side} alpha={alpha}: G {worst_g:.3e} c {worst_c:.3e}")
    assert worst_g < 2e-5 and worst_c < 2e-5, (side, worst_g, worst_c)
    if side == "users":   # bias row and column exactly 0, corner exactly 1, rhs entry 0
        assert np.all(G[:, k, :k] == 0) and np.all(G[:, :k, k] == 0)
        assert np.all(G[:, k, k] == 1) and np.all(c[:, k] == 0)
    cnt = np.bincount(u if side == "users" else i, minlength=nE)
    empty = np.flatnonzero(cnt == 0)
    assert len(empty) == (2 if side == "users" else 1)
    for e in empty:
        assert np.array_equal(G[e], G[empty[0]]) and np.all(c[e] == 0)
        assert np.max(np.abs(G[e, :k, :k] - S)) / np.max(np.abs(S)) < 2e-5
    return G, c, empty, S


# ---------------------------------------------------------------------------
# 1. normal equations against fp64 NumPy
# ---------------------------------------------------------------------------
def _normal_case(k, alpha, inexact, chunk=None):
    from movie_recommender_amd.engine import AlsContext
    u, i, r, U0, V0 = fixture(k, inexact)
    try:
        with AlsContext(u, i, r, k, NU, NI, gram_chunk=chunk, implicit_alpha=alpha) as ctx:
            if chunk is not None:   # the heavy items go through slab_reduce
                _, _, went, wslab = ctx.layout("items")[3]
                assert len(np.unique(went[wslab >= 0])) >= 2, "fewer than 2 split items"
            for side, other in (("users", "items"), ("items", "users")):
                ctx.set_factors(U0, V0)
                G, c, empty, S = check_normal(ctx, side, u, i, r, alpha, k, U0, V0)
                # building twice gives identical bits
                ctx.build_normal_equations(side)
                G2, c2 = ctx.normal_equations(side, np.arange(len(G)))
                assert np.array_equal(G, G2) and np.array_equal(c, c2), side
                # after a half-step changed the opposite table the empty entities
                # hold the NEW S (an add pass that accumulates would not)
                ctx.half_step(other)
                U1, V1 = ctx.get_factors()
                G3, _, _, S3 = check_normal(ctx, side, u, i, r, alpha, k, U1, V1)
                assert np.max(np.abs(S3 - S)) > 1e-3 * np.max(np.abs(S))
                assert not np.array_equal(G3[empty[0]], G[empty[0]])
    finally:
        if chunk is not None:
            reset_chunk()


@pytest.mark.parametrize("k", KS)
def test_normal_equations_vs_numpy(gpu, k):
    _normal_case(k, ALPHA, False)


def test_normal_equations_inexact_weights(gpu):
    """alpha = 1.7, r = |normal(0, 1)|: w and 1 + w round in fp32."""
    _normal_case(64, 1.7, True)


# ---------------------------------------------------------------------------
# 2. split entities
# ---------------------------------------------------------------------------
def test_normal_equations_split_items(gpu):
    """k = 64 at the smallest Gram chunk: the heavy items' partial records are
    summed by slab_reduce before the add pass."""
    _normal_case(64, ALPHA, False, MIN_CHUNK)


# ---------------------------------------------------------------------------
# 3. the ridge composes exactly
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["weighted", "constant"])
@pytest.mark.parametrize("k", [40, 64])
def test_ridge_composes_exactly(gpu, k, mode):
    from movie_recommender_amd.engine import AlsContext
    from test_gpu_regularized import ridge_expected, weights
    u, i, r, U0, V0 = fixture(k)
    lam = 0.3
    cnt = {"users": np.bincount(u, minlength=NU), "items": np.bincount(i, minlength=NI)}
    with AlsContext(u, i, r, k, NU, NI, implicit_alpha=ALPHA) as ctx:
        ctx.set_factors(U0, V0)
        for side, nE in (("users", NU), ("items", NI)):
            ctx.set_regularization(0.0, mode)
            ctx.build_normal_equations(side)
            G0, c0 = ctx.normal_equations(side, np.arange(nE))
            ctx.set_regularization(lam, mode)
            ctx.build_normal_equations(side)
            G1, c1 = ctx.normal_equations(side, np.arange(nE))
            assert np.array_equal(c1, c0), side
            assert np.array_equal(G1, ridge_expected(G0, k, lam, weights(cnt[side], mode))), side
            assert not np.array_equal(G1, G0)


# ---------------------------------------------------------------------------
# 4. exact solve
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_exact_solve(gpu, k):
    """After build_normal_equations and one Cholesky half-step every entity's
    x is the fp64 np.linalg.solve of the GPU's own (G, c) to 1e-5 relative
    (cond <= 1e6 asserted on the host); an entity without ratings comes back
    exactly zero, and so does the whole bias column."""
    from movie_recommender_amd.engine import AlsContext
    u, i, r, U0, V0 = fixture(k)
    cnt = {"users": np.bincount(u, minlength=NU), "items": np.bincount(i, minlength=NI)}
    with AlsContext(u, i, r, k, NU, NI, solver="cholesky", reg=0.5, reg_mode="constant",
                    implicit_alpha=ALPHA) as ctx:
        for side, nE, K in (("users", NU, k + 1), ("items", NI, k)):
            ctx.set_factors(U0, V0)
            ctx.reset_stats()
            ctx.build_normal_equations(side)
            G, c = ctx.normal_equations(side, np.arange(nE))
            ctx.half_step(side)
            U, V = ctx.get_factors()
            st = ctx.stats()
            assert st["nonpd_users"] == 0 and st["nonpd_items"] == 0, st
            x = (U if side == "users" else V).reshape(nE, K)
            empty = cnt[side] == 0
            assert empty.sum() >= 1 and np.all(x[empty] == 0)
            assert np.all(U.reshape(NU, k + 1)[:, k] == 0)
            worst = 0.0
            for e in np.flatnonzero(~empty):
                assert np.linalg.cond(G[e]) <= 1e6, (side, e, np.linalg.cond(G[e]))
                xs = np.linalg.solve(G[e], c[e])
                worst = max(worst, np.max(np.abs(x[e] - xs)) / np.max(np.abs(xs)))
            print(f"k={k} {side}: worst relative error {worst:.3e}")
            assert worst <= 1e-5, (side, worst)


# ---------------------------------------------------------------------------
# 5. CG against the oracle on the GPU's own blocks
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("onepass", [1, 0])
@pytest.mark.parametrize("k", [5, 64, 128])
def test_cg_vs_oracle(gpu, k, onepass):
    """The body and tolerances of test_regularized_cg_vs_oracle: the oracle's
    fp64 CG runs on the GPU's own implicit (G, c), so equal counts, rr, x and
    r0 also prove the unfused start.  The bias entry of r, p, q stays 0."""
    from movie_recommender_amd.engine import AlsContext
    from oracle import als_oracle as O
    u, i, r, U0, V0 = fixture(k)
    with AlsContext(u, i, r, k, NU, NI, reg=0.5, reg_mode="constant",
                    implicit_alpha=ALPHA) as ctx:
        ctx.set_option("fuse_start", 1)
        ctx.set_option("cg_onepass", onepass)
        for side, nE in (("users", NU), ("items", NI)):
            ctx.set_factors(U0, V0)
            ctx.build_normal_equations(side)
            G, c = ctx.normal_equations(side, np.arange(nE))
            x0 = (U0 if side == "users" else V0).astype(np.float32)
            r0 = np.einsum("eij,ej->ei", G, x0.astype(np.float64).reshape(nE, -1)).ravel() \
                - c.ravel()
            for m in (0, 1, 2, 4):
                ctx.set_factors(U0, V0)
                its, rr = ctx.half_step(side, 0.01, m)
                U, V = ctx.get_factors()
                vecs = ctx.cg_vectors(side)
                if side == "users":
                    for v in vecs:
                        assert np.all(v.reshape(NU, k + 1)[:, k] == 0)
                    assert np.all(U.reshape(NU, k + 1)[:, k] == 0)
                if m == 0:
                    rv, pv, _ = vecs
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
# 6. objective
# ---------------------------------------------------------------------------
def _close(a, b, tol):
    return abs(a - b) <= tol * abs(b)


def _check_objective(ctx, u, i, r, k, U, V, nU, nI, mode):
    X, Y = tables(U, V, k, nU, nI)
    o1, o2 = ctx.objective(), ctx.objective()
    assert o1 == o2                                          # identical bits
    want = dense_loss(u, i, r32_of(r), ALPHA, X, Y)
    assert o1["n"] == len(u)
    assert _close(o1["sse"], want, 1e-10), (o1["sse"], want)
    wu = np.bincount(u, minlength=nU) if mode == "weighted" else np.ones(nU)
    wi = np.bincount(i, minlength=nI) if mode == "weighted" else np.ones(nI)
    pu, pi = float(np.sum(wu * np.sum(X * X, axis=1))), float(np.sum(wi * np.sum(Y * Y, axis=1)))
    assert _close(o1["pen_users"], pu, 1e-12) and _close(o1["pen_items"], pi, 1e-12), (o1, pu, pi)
    assert o1["J"] == o1["sse"] + o1["lam"] * (o1["pen_users"] + o1["pen_items"])


@pytest.mark.parametrize("k", [5, 64])
def test_objective_vs_dense_loss(gpu, k):
    """objective()["sse"] is the loss over ALL 90 x 70 pairs, never formed
    densely on the device, against the dense NumPy sum on the same inputs (the
    fp32-rounded factors, the ratings as the CSR holds them) to 1e-10 relative:
    fp64 on both sides, the device form subtracts d^2 per stored pair."""
    from movie_recommender_amd.engine import AlsContext
    u, i, r, U0, V0 = fixture(k)
    with AlsContext(u, i, r, k, NU, NI, solver="cholesky", reg=0.5, reg_mode="constant",
                    implicit_alpha=ALPHA) as ctx:
        ctx.set_factors(U0, V0)
        _check_objective(ctx, u, i, r, k, U0, V0, NU, NI, "constant")
        ctx.set_regularization(0.5, "weighted")
        _check_objective(ctx, u, i, r, k, U0, V0, NU, NI, "weighted")
        ctx.set_regularization(0.5, "constant")
        ctx.iterate(1)
        U, V = ctx.get_factors()
        _check_objective(ctx, u, i, r, k, U, V, NU, NI, "constant")


def test_objective_with_split_users(gpu):
    """The fixture with the roles swapped (70 users with the zipf ids, 90
    items) at the smallest chunk: the heavy users are split across waves."""
    from movie_recommender_amd.engine import AlsContext
    k = 64
    i, u, r, V0, U0 = fixture(k)          # swapped: users <- items
    nU, nI = NI, NU
    U0 = np.concatenate([U0.reshape(nU, k), np.zeros((nU, 1))], axis=1).ravel()
    V0 = V0.reshape(nI, k + 1)[:, :k].ravel()
    order = np.argsort(u, kind="stable")
    u, i, r = u[order], i[order], r[order]
    try:
        with AlsContext(u, i, r, k, nU, nI, gram_chunk=MIN_CHUNK, reg=0.5, reg_mode="constant",
                        implicit_alpha=ALPHA) as ctx:
            assert int((ctx.layout("users")[3][3] >= 0).sum()) >= 4
            ctx.set_factors(U0, V0)
            _check_objective(ctx, u, i, r, k, U0, V0, nU, nI, "constant")
    finally:
        reset_chunk()


# ---------------------------------------------------------------------------
# 7. monotone descent
# ---------------------------------------------------------------------------
def test_objective_is_monotone_under_exact_half_steps(gpu):
    """Each Cholesky half-step minimises J exactly on its side: over 6
    half-steps J never rises by more than 1e-6 relative and ends below its
    start (in fp64 every half-step of this fixture lowers J by >= 1.1 %)."""
    from movie_recommender_amd.engine import AlsContext
    k = 20
    u, i, r, U0, V0 = fixture(k)
    with AlsContext(u, i, r, k, NU, NI, solver="cholesky", reg=0.5, reg_mode="constant",
                    implicit_alpha=ALPHA) as ctx:
        ctx.set_factors(U0, V0)
        J = [ctx.objective()["J"]]
        for h in range(6):
            ctx.half_step("users" if h % 2 == 0 else "items")
            J.append(ctx.objective()["J"])
    print("J per half-step:", J)
    for a, b in zip(J, J[1:]):
        assert b <= a * (1 + 1e-6), J
    assert J[-1] < J[0]


# ---------------------------------------------------------------------------
# 8. the loop against the restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 20])
def test_cholesky_loop_vs_numpy(gpu, k):
    """Three exact iterations against the fp64 NumPy loop: factors to 1e-4
    (the bound of test_regularized_cholesky_loop_vs_oracle), J to 1e-5.  A CPU
    run with 4e-7 relative noise plus fp32 rounding on G, c and x gave 2.6e-5
    on the factors and 3.1e-7 on J at these k; at k = 64 the blocks' condition
    (1e4) takes the factor distance to 2.6e-4, so the loop stops at k = 20."""
    from movie_recommender_amd.engine import AlsContext
    u, i, r, U0, V0 = fixture(k)
    lam = 0.5
    with AlsContext(u, i, r, k, NU, NI, solver="cholesky", reg=lam, reg_mode="constant",
                    implicit_alpha=ALPHA) as ctx:
        ctx.set_factors(U0, V0)
        ctx.iterate(3)
        U, V = ctx.get_factors()
        st = ctx.stats()
        J = ctx.objective()["J"]
    assert st["nonpd_users"] == 0 and st["nonpd_items"] == 0
    X0, Y0 = tables(U0, V0, k)
    Xo, Yo = als64(u, i, r32_of(r), ALPHA, lam, X0, Y0, 3)
    X, Y = tables(U, V, k)
    Jo = dense_loss(u, i, r32_of(r), ALPHA, Xo, Yo) + lam * (np.sum(Xo * Xo) + np.sum(Yo * Yo))
    print(f"k={k}: relX {rel_err(X, Xo):.3e} relY {rel_err(Y, Yo):.3e} J {abs(J - Jo) / Jo:.3e}")
    assert rel_err(X, Xo) < 1e-4 and rel_err(Y, Yo) < 1e-4
    assert abs(J - Jo) <= 1e-5 * Jo
    assert np.all(U.reshape(NU, k + 1)[:, k] == 0)


# ---------------------------------------------------------------------------
# 9. switching the mode off restores the explicit engine
# ---------------------------------------------------------------------------
def test_switching_off_restores_the_explicit_engine(gpu):
    from movie_recommender_amd.engine import AlsContext
    k = 64
    u, i, r, _, V0 = fixture(k)
    U0 = np.random.default_rng(9).uniform(-1, 1, NU * (k + 1))   # with a bias column
    outs = []
    for implicit_first in (True, False):
        with AlsContext(u, i, r, k, NU, NI) as ctx:
            if implicit_first:
                ctx.set_implicit(ALPHA)
                ctx.set_factors(U0, V0)
                ctx.iterate(1)
                ctx.set_implicit(0)
            ctx.set_factors(U0, V0)
            ctx.reset_stats()
            ctx.iterate(1)
            st = ctx.stats()
            outs.append((ctx.get_factors(), (st["cg_users_total"], st["cg_items_total"])))
    ((Ua, Va), ca), ((Ub, Vb), cb) = outs
    assert np.array_equal(Ua, Ub) and np.array_equal(Va, Vb)
    assert ca == cb and ca[0] > 0 and ca[1] > 0
    assert np.any(Ua.reshape(NU, k + 1)[:, k] != 0)   # the bias is back


def test_init_factors_keeps_the_bias_pinned(gpu):
    """The device-side initialiser in implicit mode: the bias column is zero
    after init_factors and after a CG iteration from that start, the factor
    values are the explicit mode's for the same seed, and predict is X.Y."""
    from movie_recommender_amd.engine import AlsContext
    k = 64
    u, i, r, _, _ = fixture(k)
    with AlsContext(u, i, r, k, NU, NI) as ctx:
        ctx.init_factors(3)
        Ue, Ve = ctx.get_factors()
    assert np.any(Ue.reshape(NU, k + 1)[:, k] != 0)
    with AlsContext(u, i, r, k, NU, NI, reg=0.5, reg_mode="constant",
                    implicit_alpha=ALPHA) as ctx:
        ctx.init_factors(3)
        U, V = ctx.get_factors()
        assert np.all(U.reshape(NU, k + 1)[:, k] == 0)
        assert np.array_equal(U.reshape(NU, k + 1)[:, :k], Ue.reshape(NU, k + 1)[:, :k])
        assert np.array_equal(V, Ve)
        ctx.iterate(1)                            # CG, the default solver
        U, V = ctx.get_factors()
        st = ctx.stats()
        assert st["cg_users_total"] > 0 and st["cg_items_total"] > 0
        assert np.all(U.reshape(NU, k + 1)[:, k] == 0)
        for v in ctx.cg_vectors("users"):
            assert np.all(v.reshape(NU, k + 1)[:, k] == 0)
        X, Y = tables(U, V, k)
        want = np.einsum("nj,nj->n", X[u], Y[i])
        got = ctx.predict(u, i)
        assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))


# ---------------------------------------------------------------------------
# 10. refusals leave the context usable
# ---------------------------------------------------------------------------
def test_refusals(gpu):
    from movie_recommender_amd.engine import AlsContext
    from movie_recommender_amd import distributed
    k = 8
    u, i, r, _, _ = fixture(k)
    rneg = r.copy()
    rneg[len(r) // 2] = -0.5
    (u0, u1), (i0, i1), uv, iv, _, _ = distributed.shard_views(u, i, r, NU, NI, 1, 3, k=k)
    cases = {
        "negative": lambda: AlsContext(u, i, rneg, k, NU, NI),
        "shard": lambda: AlsContext(uv[0], uv[1], uv[2], k, NU, NI, user_range=(u0, u1),
                                    item_range=(i0, i1), item_view=iv),
        "k144": lambda: AlsContext(u, i, r, 144, NU, NI),
    }
    for name, make in cases.items():
        with make() as ctx:
            with pytest.raises(RuntimeError, match="implicit"):
                ctx.set_implicit(ALPHA)
            assert ctx.implicit_alpha == 0.0
            ctx.init_factors(1)
            ctx.iterate(1)                # the explicit engine still runs
            assert ctx.stats()["iterations"] == 1
    with pytest.raises(RuntimeError, match="implicit"):
        AlsContext(u, i, rneg, k, NU, NI, implicit_alpha=ALPHA)


# ---------------------------------------------------------------------------
# 11. als_implicit end to end
# ---------------------------------------------------------------------------
def planted():
    rng = np.random.default_rng(7)
    nU, nI = 120, 100
    M = rng.normal(0, 1, (nU, 4)) @ rng.normal(0, 1, (nI, 4)).T
    u, i = np.nonzero(M > np.quantile(M, 0.85))
    conf = rng.integers(1, 4, len(u)).astype(np.float64)
    return u.astype(np.int32), i.astype(np.int32), conf, nU, nI


def test_als_implicit_end_to_end(gpu):
    """Planted rank-4 preferences (the 15 % largest entries of A B^T, 120 x
    100), k = 8, defaults otherwise.  J is non-increasing and the stored pairs
    score higher than the others: the NumPy restatement (als64 from the same
    RandomState(0) start, 15 iterations) separates the two means by 0.820;
    the assertion asks for 0.3."""
    from movie_recommender_amd.implicit import als_implicit
    u, i, conf, nU, nI = planted()
    X, Y, its, hist = als_implicit(u, i, conf, 8, nU, nI)
    assert X.shape == (nU, 8) and Y.shape == (nI, 8)
    assert 1 <= its <= 15 and len(hist) == its
    assert all(b <= a * (1 + 1e-6) for a, b in zip(hist, hist[1:])), hist
    score = X @ Y.T
    seen = np.zeros((nU, nI), bool)
    seen[u, i] = True
    gap = score[seen].mean() - score[~seen].mean()
    print(f"iterations {its}, J {hist[0]:.4f} -> {hist[-1]:.4f}, gap {gap:.3f}")
    assert gap > 0.3, gap
