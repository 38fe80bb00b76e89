"""Noisy near-collinear fold-in lists with their exact least-squares answers.

    python tests/golden/make_golden_foldin_sweep.py

The known-answer cases of tests/foldin_lstsq_cases.py are consistent systems
plus a residual that is exactly orthogonal to range(A).  The generic case --
ordinary random factors, half-star ratings, a large residual that is not
orthogonal to anything in particular -- has no closed form, and its
sensitivity goes as cond(A)^2, so this script stores the answer instead.
For k in {3, 11} and M = 40: four random lists, each at thirteen levels of
near-collinearity (``V[:, 1] = V[:, 0] + s * noise``), with the exact
minimiser of |A x - r| for the fp64 inputs as stored, from the normal
equations in 60-digit mpmath arithmetic, beside numpy.linalg.lstsq's own
answer on the same inputs.

The levels aim at Cholesky pivot ratios of A^T A (min / max pivot, the number
fold_in_kernel compares with its cond_limit) from 1e-2 down to 1e-13, dense
between 1e-8 and 4e-6: normal equations err by about eps / ratio there, which
is where they stop meeting the 1e-8 the fold-in promises.  Four lists per
level because that error varies severalfold from list to list.

foldin_sweep.npz, per k (S lists, L levels):
  V0_k (S, 40, k)      the factors; level l replaces column 1 by col1_k[s, l]
  col1_k (S, L, 40), r_k (S, 40), s_k / ratio_k / cond_k (S, L),
  x_exact_k, x_lstsq_k (S, L, k+1)
"""
import os
import sys

import mpmath
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from foldin_lstsq_cases import pivot_ratio  # noqa: E402

M = 40
SEEDS = 4
TARGETS = (1e-2, 1e-4, 1e-5, 4e-6, 2e-6, 5e-7, 2.5e-7, 1e-7, 4e-8, 2e-8, 1.1e-8, 1e-10, 1e-13)


def exact_lstsq(A, b):
    mpmath.mp.dps = 60
    Am = mpmath.matrix(A.tolist())
    bm = mpmath.matrix(b.tolist())
    x = mpmath.lu_solve(Am.T * Am, Am.T * bm)
    # the residual of the normal equations in the same arithmetic: the
    # stored answer is good to far more than fp64
    g = Am.T * (Am * x - bm)
    assert max(abs(v) for v in g) < mpmath.mpf(10) ** -35
    return np.array([float(v) for v in x])


def make_list(k, seed, targets=TARGETS):
    """One random list at every level."""
    rs = np.random.RandomState(seed)
    V0 = rs.normal(0, 0.6, (M, k))
    noise = rs.normal(0, 0.6, M)
    r = rs.choice(np.arange(1, 11) / 2.0, M)

    def design(col1):
        V = V0.copy()
        V[:, 1] = col1
        return np.c_[V, np.ones(M)]

    c = pivot_ratio(design(V0[:, 0] + 2.0 ** -8 * noise)) * 2.0 ** 16
    out = {n: [] for n in ("col1", "s", "ratio", "cond", "x_exact", "x_lstsq")}
    for t in targets:
        s = (t / c) ** 0.5
        col1 = V0[:, 0] + s * noise
        A = design(col1)
        out["col1"].append(col1)
        out["s"].append(s)
        out["ratio"].append(pivot_ratio(A))
        out["cond"].append(np.linalg.cond(A))
        out["x_exact"].append(exact_lstsq(A, r))
        out["x_lstsq"].append(np.linalg.lstsq(A, r, rcond=None)[0])
    out = {n: np.array(v) for n, v in out.items()}
    out["V0"], out["r"] = V0, r
    return out


def make_lists(k, seeds):
    ls = [make_list(k, s) for s in seeds]
    return {f"{n}_k{k}": np.array([l[n] for l in ls]) for n in ls[0]}


def main():
    out = {}
    for k in (3, 11):
        d = make_lists(k, [4100 + k + 100 * j for j in range(SEEDS)])
        xe, xl = d[f"x_exact_k{k}"], d[f"x_lstsq_k{k}"]
        err = np.max(np.abs(xl - xe), axis=2) / np.max(np.abs(xe), axis=2)
        for j in range(SEEDS):
            for l in range(len(TARGETS)):
                print(f"k={k} list {j} ratio={d[f'ratio_k{k}'][j, l]:.3e} "
                      f"cond={d[f'cond_k{k}'][j, l]:.3e} lstsq err={err[j, l]:.2e}")
        out.update(d)
    np.savez_compressed(os.path.join(HERE, "foldin_sweep.npz"), **out)


if __name__ == "__main__":
    main()
