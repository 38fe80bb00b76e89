"""The fold-in cases of foldin_lstsq_cases.py and the sweep fixture are fit to
test with: on every case numpy.linalg.lstsq alone returns the designed rank
and lands within the case's tolerance of the known answer, no singular value
sits near lstsq's cut-off, and the conditioning ladder straddles the kernel's
Cholesky / Jacobi limit.  (The builders assert their own exactness in integer
arithmetic when a case is made.)  Runs on the CPU; the GPU side is
test_gpu_serving_foldin.py."""
import numpy as np
import pytest

import foldin_lstsq_cases as C
from conftest import load_golden


def test_limit_is_the_kernels():
    assert C.source_cond_limit() == C.COND_LIMIT


@pytest.mark.parametrize("k", C.SIZES)
def test_cases_are_sound(k):
    print()
    print(f"{'case':34s} {'M':>5s} {'rank':>4s} {'ratio':>9s} {'must':>4s} {'cond_eff':>9s} "
          f"{'e_ref':>9s} {'tol':>9s}")
    for c in C.cases_for(k):
        r = C.reference(c)
        print(f"{c.name:34s} {c.M:5d} {c.rank:4d} {r['ratio']:9.2e} {r['must']:4d} "
              f"{r['cond_eff']:9.2e} {r['e_ref']:9.2e} {r['tol']:9.2e}")
        assert r["rank"] == c.rank, c.name
        assert len(r["kept"]) == c.rank, c.name
        # nothing near the cut-off: kept values 1e3 above it (the dropped ones
        # are below it, or lstsq's rank would differ)
        assert r["kept"][-1] >= 1e3 * r["cut"], (c.name, r["kept"][-1], r["cut"])
        assert r["e_ref"] <= r["tol"], c.name
        # lstsq is backward stable on these consistent-plus-orthogonal systems
        assert r["e_ref"] <= 64 * c.K * C.EPS * r["cond_eff"], c.name
        if c.kind != "full":
            assert r["must"] == 2


def test_case_shapes_cover_the_kernel_paths():
    for k in C.SIZES:
        K = k + 1
        cs = C.cases_for(k)
        full = {c.M for c in cs if c.kind == "full" and C.reference(c)["must"] == 1}
        assert {K, K + 1, 301} <= full
        assert {m for m in (32, 33, 64) if m > K + 1} <= full
        kinds = {c.kind for c in cs}
        assert {"a", "b"} <= kinds and (k < 3 or {"c", "d"} <= kinds)
        assert any(c.kind != "full" and c.M == K for c in cs)
    for k in (11, 128):
        assert {c.kind == "full" for c in C.cases_for(k) if c.M == C.LONG_M} == {True, False}


@pytest.mark.parametrize("k,M", C.LADDER_SHAPES)
def test_ladder_straddles_the_limit(k, M):
    ratios = np.array([C.reference(c)["ratio"] for c in C.ladder(k, M)])
    conds = np.array([C.reference(c)["cond_eff"] for c in C.ladder(k, M)])
    musts = [C.reference(c)["must"] for c in C.ladder(k, M)]
    assert np.sum(ratios > C.COND_LIMIT) >= 3 and np.sum(ratios < C.COND_LIMIT) >= 3
    assert musts.count(1) >= 3 and musts.count(2) >= 3
    near = (ratios > C.COND_LIMIT / 5) & (ratios < C.COND_LIMIT * 5)
    assert np.sum(near & (ratios > C.COND_LIMIT)) >= 1
    assert np.sum(near & (ratios < C.COND_LIMIT)) >= 1
    assert conds.min() < 50 and conds.max() > 3e9


def test_sweep_fixture():
    """The stored noisy sweep: the inputs reproduce the stored lstsq answer,
    the levels lie on both sides of the limit, and lstsq's own error against
    the 60-digit answer is what the GPU test takes as its yardstick."""
    d = load_golden("foldin_sweep.npz")
    for k in (3, 11):
        ratios = d[f"ratio_k{k}"]
        S, L = ratios.shape
        assert S >= 1 and L >= 12
        for s in range(S):
            for lv in range(L):
                A = np.c_[C.sweep_factors(d, k, s, lv), np.ones(40)]
                x, _, rank, _ = np.linalg.lstsq(A, d[f"r_k{k}"][s], rcond=None)
                assert rank == k + 1
                assert C.rel_err(x, d[f"x_lstsq_k{k}"][s, lv]) <= 1e-6
                if ratios[s, lv] > 1e-9:        # below, the ratio itself is rounding
                    assert abs(C.pivot_ratio(A) / ratios[s, lv] - 1) < 1e-2
            assert np.sum(ratios[s] > 100 * C.COND_LIMIT) >= 1
            assert np.sum((ratios[s] < 5 * C.COND_LIMIT) & (ratios[s] > C.COND_LIMIT)) >= 1
            assert np.sum(ratios[s] < C.COND_LIMIT) >= 3
            assert np.sum(ratios[s] < C.COND_LIMIT / 100) >= 1
