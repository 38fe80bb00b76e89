"""Implicit-feedback ALS (Hu, Koren, Volinsky 2008) on the device-resident
engine: plays, clicks or view counts instead of ratings.

A stored ``(user, item, r)`` with ``r >= 0`` means "preference 1 with
confidence ``1 + alpha r``"; every other pair means "preference 0 with
confidence 1".  The loss runs over ALL pairs,

    J = sum_ui c_ui (p_ui - x_u . y_i)^2 + reg (pen_users + pen_items),

and is never formed densely (``AlsContext.set_implicit``, DESIGN.md "Implicit
feedback").  There is no user bias in this model.
"""
import numpy as np

from .engine import AlsContext, check_implicit, check_regularization


def als_implicit(user_ids, item_ids, confidence, k, num_users, num_items, alpha=40.0,
                 reg=0.01, reg_mode="constant", solver="cholesky", max_iterations=15,
                 tol=1e-4, seed=0):
    """Trains one implicit-feedback model.  ``confidence`` holds the counts /
    strengths ``r >= 0`` of the stored pairs.  U0 then V0 are drawn from
    ``numpy.random.RandomState(seed)`` (uniform(-1, 1), ``cpp_ls.als``'s
    shapes; the bias column is dropped); ALS iterations run until the relative
    decrease of J falls below ``tol`` or ``max_iterations`` is reached.
    Returns ``(X[num_users, k], Y[num_items, k], iterations, [J after every
    iteration])``; the score of a pair is ``X[u] @ Y[i]``.

    ``solver="nnls"`` constrains every factor to be >= 0 (each half-step is
    the exact non-negative block minimiser, ``AlsContext.set_nnls``): X and Y
    come back non-negative, so every score is a non-negative affinity."""
    alpha = check_implicit(alpha)
    if not alpha > 0.0:
        raise ValueError("alpha must be > 0")
    check_regularization(reg, reg_mode)
    k, num_users, num_items = int(k), int(num_users), int(num_items)
    rs = np.random.RandomState(seed)
    U0 = rs.uniform(-1, 1, num_users * (k + 1))
    V0 = rs.uniform(-1, 1, num_items * k)
    history = []
    with AlsContext(user_ids, item_ids, confidence, k, num_users, num_items, solver=solver,
                    reg=reg, reg_mode=reg_mode, implicit_alpha=alpha) as ctx:
        ctx.set_factors(U0, V0)
        iterations = 0
        while iterations < max_iterations:
            ctx.iterate(1)
            iterations += 1
            history.append(ctx.objective()["J"])
            if len(history) > 1 and history[-2] - history[-1] < tol * abs(history[-2]):
                break
        U, V = ctx.get_factors()
    X = U.reshape(num_users, k + 1)[:, :k].copy()
    Y = V.reshape(num_items, k).copy()
    return X, Y, iterations, history
