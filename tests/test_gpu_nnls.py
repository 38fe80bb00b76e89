"""GPU: the non-negative solver (MR_SOLVER_NNLS, csrc/nnls.hip) against the
fp64 NumPy restatement of its rule in nnls_cases.py.

Fixtures (nnls_cases.fixture): the 90 x 70 one of test_gpu_implicit.py for
k in {5, 20, 40, 64} and 48 x 300 for k = 128 (more items than factors, so S
has full rank); explicit runs use weighted lambda = 0.05, implicit runs
alpha = 8 and constant lambda = 0.05.  Every comparison runs the restatement
on the (G, c) read back from the device and the same start, so it checks the
solver alone.

Bound 1: |x_gpu - x_ref|_inf <= 2^-23 max(1, |x_ref|_inf) per entity -- the
fp32 store of x costs 2^-24 relative, the fp64 solve about cond * 2^-53, which
is nothing at the cond <= 1e5 these fixtures have (asserted).  Rounds: equal
for at least 95 % of the entities; a sign decision on a value at fp64 noise
level may differ, and the restatement against itself in another summation
order stays inside that cap (test_nnls_api.py checks that on the CPU).
"""
import functools

import numpy as np
import pytest

import nnls_cases as nc

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
KS = nc.KS_SMALL + [nc.K_LARGE]
MODES = ["explicit", "implicit"]
SIDES = ["users", "items"]


def make_ctx(k, mode, r_shift=0.0, **kw):
    from movie_recommender_amd.engine import AlsContext
    u, i, r, U0, V0, nU, nI = nc.fixture(k, nc.shape_of(k))
    kw.setdefault("solver", "nnls")
    if mode == "implicit":
        kw.update(reg=nc.LAM, reg_mode="constant", implicit_alpha=nc.ALPHA)
    else:
        kw.setdefault("reg", nc.LAM)
        kw.setdefault("reg_mode", "weighted")
    return AlsContext(u, i, r + r_shift, k, nU, nI, **kw)


def start_of(k, mode):
    _, _, _, U0, V0, _, _ = nc.fixture(k, nc.shape_of(k))
    return (nc.zero_bias(U0, k) if mode == "implicit" else np.array(U0)), np.array(V0)


def half_step(ctx, k, mode, side, ridge=0.0, **ref_kw):
    """One half-step of `side` from the fixture's factors: the read-back
    (G, c), the GPU's x and rounds, the restatement's on the same system."""
    _, _, _, _, _, nU, nI = nc.fixture(k, nc.shape_of(k))
    U0, V0 = start_of(k, mode)
    ctx.set_factors(U0, V0)
    st0 = ctx.stats()
    assert ctx.half_step(side)[0] == 0
    E = nU if side == "users" else nI
    G, c = ctx.normal_equations(side, np.arange(E))
    U, V = ctx.get_factors()
    x = U.reshape(nU, k + 1) if side == "users" else V.reshape(nI, k)
    other_same = np.array_equal(V, V0) if side == "users" else np.array_equal(U, U0)
    assert other_same, "the half-step wrote the other side's table"
    prev = nc.prev_of(side, U0, V0, k, nU, nI)
    x_ref, r_ref = nc.solve_side(G, c, k, prev, ridge=ridge, **ref_kw)
    st1 = ctx.stats()
    key = "nonpd_users" if side == "users" else "nonpd_items"
    return {"G": G, "c": c, "x": x, "prev": prev, "rounds": ctx.nnls_rounds(side),
            "stats": ctx.nnls_stats(side), "x_ref": x_ref, "r_ref": r_ref, "k": k,
            "nonpd": st1[key] - st0[key], "ridge": ridge}


@functools.lru_cache(maxsize=None)
def case(k, mode, side):
    with make_ctx(k, mode) as ctx:
        return half_step(ctx, k, mode, side)


def worst_error(d, rows=None):
    """max over entities of |x - x_ref|_inf / max(1, |x_ref|_inf)."""
    x, ref = d["x"], d["x_ref"]
    if rows is not None:
        x, ref = x[rows], ref[rows]
    if len(x) == 0:
        return 0.0
    return float(np.max(np.max(np.abs(x - ref), axis=1) /
                        np.maximum(1.0, np.max(np.abs(ref), axis=1))))


def kkt_violation(d, rows):
    """Worst excess over the bound b_j = 1e-9 |c|_inf + 2^-23 (|G| |x|)_j of
    the KKT conditions at the returned x, over `rows`; <= 0 passes."""
    k, worst = d["k"], -np.inf
    for e in rows:
        G = d["G"][e] + d["ridge"] * np.eye(len(d["c"][e]))
        c, x = d["c"][e], d["x"][e]
        assert np.all(x[:k] >= 0.0)
        g = G @ x - c
        b = 1e-9 * np.max(np.abs(c)) + EPS * (np.abs(G) @ np.abs(x))
        active = np.ones(len(x), bool)
        active[:k] = x[:k] > 0.0            # the bias (index k) is always active
        worst = max(worst, np.max(np.where(active, np.abs(g) - b, -g - b)))
    return worst


# ---------------------------------------------------------------------------
# 1. one half-step against the restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", KS)
def test_half_step_vs_restatement(gpu, k, mode, side):
    d = case(k, mode, side)
    solved = np.flatnonzero(d["r_ref"] != 0)
    cond = max(np.linalg.cond(d["G"][e]) for e in solved)
    err = worst_error(d)
    same = float(np.mean(d["rounds"] == d["r_ref"]))
    print(f"k={k} {mode} {side}: err {err:.3e} (bound {EPS:.3e}) cond {cond:.2e} "
          f"rounds equal {same:.3f} max {d['stats']['rounds_max']} ref max {d['r_ref'].max()}")
    assert cond <= 1e5, cond
    assert err <= EPS, err
    assert same >= 0.95, same
    assert d["stats"]["unconverged"] == 0 and np.all(d["r_ref"] >= 0)
    assert d["stats"]["entities"] == len(d["rounds"])
    assert d["stats"]["rounds_total"] == int(np.sum(np.abs(d["rounds"])))
    assert d["stats"]["rounds_max"] == int(np.max(np.abs(d["rounds"])))
    # only the empty entities of an explicit run (weighted lambda: G = 0) are non-PD
    n_empty = (2 if side == "users" else 1) if mode == "explicit" else 0
    assert int(np.sum(d["rounds"] == 0)) == n_empty == d["nonpd"]
    assert np.array_equal(d["rounds"] == 0, d["r_ref"] == 0)
    if k == nc.K_LARGE:   # what the restatement needs on this fixture
        assert d["r_ref"].max() <= (18 if mode == "implicit" else 7)


# ---------------------------------------------------------------------------
# 2. KKT at the returned x
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", KS)
def test_kkt(gpu, k, mode, side):
    d = case(k, mode, side)
    worst = kkt_violation(d, np.flatnonzero(d["rounds"] > 0))
    print(f"k={k} {mode} {side}: worst KKT excess {worst:.3e}")
    assert worst <= 0.0, worst


# ---------------------------------------------------------------------------
# 3. the constraint bites
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", KS)
def test_constraint_bites(gpu, k, mode, side):
    d = case(k, mode, side)
    solved = d["rounds"] > 0
    fac = d["x"][solved][:, :k]
    share = float(np.mean(fac == 0.0))
    print(f"k={k} {mode} {side}: zeros {share:.3f} max rounds {d['stats']['rounds_max']}")
    assert 0.2 <= share <= 0.8, share
    assert d["stats"]["rounds_max"] >= 2
    assert not np.any(np.signbit(d["x"][:, :k])), "a zero was stored as -0"


# ---------------------------------------------------------------------------
# 4. the bias stays free (and the solver's own ridge is applied)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ridge", [0.0, 0.25])
def test_bias_stays_free(gpu, ridge):
    k = 20
    with make_ctx(k, "explicit", r_shift=-3.0, ridge=ridge) as ctx:
        d = half_step(ctx, k, "explicit", "users", ridge=ridge)
    solved = d["rounds"] > 0
    bias = d["x"][solved, k]
    print(f"ridge={ridge}: min bias {bias.min():.3f} err {worst_error(d):.3e}")
    assert np.sum(bias < 0.0) >= 1
    assert worst_error(d) <= EPS
    assert np.all(d["x"][:, :k] >= 0.0)
    assert kkt_violation(d, np.flatnonzero(solved)) <= 0.0
    if ridge > 0.0:   # every entity is PD now: the empty users solve to 0
        assert np.all(d["rounds"] > 0) and np.all(d["x"][-2:] == 0.0)


# ---------------------------------------------------------------------------
# 5. the round cap
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_round_cap(gpu, mode):
    k = 40
    for side in SIDES:
        full = case(k, mode, side)
        with make_ctx(k, mode) as ctx:
            ctx.set_nnls(max_rounds=1)
            d = half_step(ctx, k, mode, side, max_rounds=1)
            ctx.set_nnls(0)
            again = half_step(ctx, k, mode, side)
        needs_more = full["r_ref"] > 1
        assert needs_more.sum() >= 10
        assert np.all(np.isin(d["rounds"], [-1, 0, 1]))
        assert np.mean((d["rounds"] == -1) == needs_more) >= 0.95
        assert d["stats"]["unconverged"] == int(np.sum(d["rounds"] == -1))
        assert np.mean(d["rounds"] == d["r_ref"]) >= 0.95
        assert np.all(d["x"][:, :k] >= 0.0)
        assert kkt_violation(d, np.flatnonzero(d["rounds"] == 1)) <= 0.0
        # entities cut at the cap hold the clamped first solve, as the restatement
        agree = d["rounds"] == d["r_ref"]
        assert worst_error(d, agree) <= EPS
        # the default is back
        assert again["stats"]["unconverged"] == 0
        assert np.array_equal(again["rounds"], full["rounds"])
        assert np.array_equal(again["x"], full["x"])
    from movie_recommender_amd import _lib
    with make_ctx(5, mode) as ctx:
        assert _lib.lib().mr_als_set_nnls(ctx._h, -1, 1) == -1
        assert "max_rounds" in _lib.last_error()


# ---------------------------------------------------------------------------
# 6. entities that are not positive definite
# ---------------------------------------------------------------------------
def test_nonpd_keeps_clamped_previous(gpu):
    """Explicit, lambda = 0: the two users and the item without ratings have
    G = 0.  k = 5: every other entity has >= 13 ratings for <= 6 unknowns."""
    k = 5
    with make_ctx(k, "explicit", reg=0.0) as ctx:
        for side, n_empty in (("users", 2), ("items", 1)):
            d = half_step(ctx, k, "explicit", side)
            assert d["nonpd"] == n_empty
            assert np.array_equal(np.flatnonzero(d["rounds"] == 0),
                                  np.arange(len(d["rounds"]) - n_empty, len(d["rounds"])))
            prev = d["prev"][-n_empty:]
            want = prev.copy()
            want[:, :k] = np.maximum(prev[:, :k], 0.0)   # the bias (users) as it was
            assert np.any(prev[:, :k] < 0.0)
            assert np.array_equal(d["x"][-n_empty:], want)
            assert not np.any(np.signbit(d["x"][-n_empty:, :k]))
            assert worst_error(d) <= EPS and d["stats"]["unconverged"] == 0


# ---------------------------------------------------------------------------
# 7. cold start = warm start
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_cold_equals_warm(gpu, mode):
    k = 40
    with make_ctx(k, mode) as ctx:
        ctx.set_nnls(0, warm_start=False)
        for side in SIDES:
            warm = case(k, mode, side)
            cold = half_step(ctx, k, mode, side, warm=False)
            assert worst_error(cold) <= EPS                       # against its own restatement
            cold["x_ref"] = warm["x_ref"]
            err = worst_error(cold)
            print(f"{mode} {side}: cold vs warm restatement {err:.3e}, rounds "
                  f"{cold['stats']['rounds_total']} vs {warm['stats']['rounds_total']}")
            assert err <= EPS
            assert cold["stats"]["unconverged"] == 0
            assert np.mean(cold["rounds"] == cold["r_ref"]) >= 0.95


# ---------------------------------------------------------------------------
# 8. training
# ---------------------------------------------------------------------------
def check_monotone(history):
    for a, b in zip(history, history[1:]):
        assert b <= a * (1.0 + 1e-6), history


def test_training_explicit(gpu):
    k = 20
    _, _, _, _, _, nU, nI = nc.fixture(k)
    U0, V0 = start_of(k, "explicit")
    history = []
    with make_ctx(k, "explicit") as ctx:
        ctx.set_factors(U0, V0)
        for _ in range(8):
            ctx.iterate(1)
            history.append(ctx.objective()["J"])
        U, V = ctx.get_factors()
        assert ctx.stats()["iterations"] == 8
        assert ctx.nnls_stats("users")["unconverged"] == 0
    print("J:", " ".join(f"{j:.6g}" for j in history))
    check_monotone(history)
    assert history[-1] < history[0]
    U = U.reshape(nU, k + 1)
    assert np.all(U[:, :k] >= 0.0) and np.all(V >= 0.0)
    assert np.any(U[:, k] != 0.0)


def test_training_implicit(gpu):
    from movie_recommender_amd.implicit import als_implicit
    k = 20
    u, i, r, _, _, nU, nI = nc.fixture(k)
    X, Y, its, history = als_implicit(u, i, r, k, nU, nI, alpha=nc.ALPHA, reg=nc.LAM,
                                      solver="nnls", max_iterations=8, tol=0.0)
    print("J:", " ".join(f"{j:.6g}" for j in history))
    assert its == len(history) and its >= 2
    check_monotone(history)
    assert np.all(X >= 0.0) and np.all(Y >= 0.0) and np.any(X > 0.0) and np.any(Y > 0.0)
    U0, V0 = start_of(k, "implicit")
    with make_ctx(k, "implicit") as ctx:
        ctx.set_factors(U0, V0)
        ctx.iterate(2)
        U, _ = ctx.get_factors()
    assert np.all(U.reshape(nU, k + 1)[:, k] == 0.0)


# ---------------------------------------------------------------------------
# 9. nothing else moved
# ---------------------------------------------------------------------------
def test_switching_solvers_leaves_cholesky_bitwise(gpu):
    k = 40
    U0, V0 = start_of(k, "explicit")
    with make_ctx(k, "explicit", solver="cholesky") as a, \
            make_ctx(k, "explicit", solver="cholesky") as b:
        a.set_factors(U0, V0)
        a.set_solver("nnls")
        a.set_nnls(max_rounds=3, warm_start=False)
        a.iterate(1)
        a.set_solver("cholesky")
        for ctx in (a, b):
            ctx.set_factors(U0, V0)
            ctx.iterate(2)
        Ua, Va = a.get_factors()
        Ub, Vb = b.get_factors()
    assert np.array_equal(Ua, Ub) and np.array_equal(Va, Vb)
    assert np.any(Ua.reshape(-1, k + 1)[:, :k] < 0.0)   # the unconstrained solver again


def test_refusals(gpu):
    from movie_recommender_amd import distributed
    from movie_recommender_amd.engine import AlsContext
    k = 8
    u, i, r, _, _, nU, nI = nc.fixture(k)
    (u0, u1), (i0, i1), uv, iv, _, _ = distributed.shard_views(u, i, r, nU, nI, 1, 3, k=k)
    with AlsContext(uv[0], uv[1], uv[2], k, nU, nI, user_range=(u0, u1), item_range=(i0, i1),
                    item_view=iv, solver="cholesky", ridge=0.5) as ctx:
        with pytest.raises(RuntimeError, match="NNLS"):
            ctx.set_solver("nnls")
        ctx.init_factors(3)
        assert ctx.half_step("users")[0] == 0           # still the Cholesky solver:
        with pytest.raises(RuntimeError, match="no NNLS solve"):
            ctx.nnls_stats("users")                      # no NNLS solve ran
    for solver in ("cholesky", "nnls"):
        with AlsContext(u, i, r, 144, nU, nI, solver=solver, reg=nc.LAM) as ctx:
            ctx.init_factors(3)
            with pytest.raises(RuntimeError, match="k <= 128"):
                ctx.half_step("users")
