"""CPU: the implicit-feedback entry point exists, fails cleanly on a NULL
context, and the Python face rejects bad arguments before any native call."""
import inspect
import os

import numpy as np
import pytest


def test_symbol_exists_and_rejects_null_context():
    from movie_recommender_amd import _lib
    L = _lib.lib()
    assert hasattr(L, "mr_als_set_implicit")
    assert "mr_als_set_implicit" in _lib.SIGNATURES
    # a message from this very call: set a different one first
    assert L.mr_set_gram_chunk(1) == -1 and "chunk" in _lib.last_error()
    assert L.mr_als_set_implicit(None, 8.0) == -1
    msg = _lib.last_error()
    assert msg and "chunk" not in msg and "mr_als_set_implicit" in msg, msg
    assert L.mr_set_gram_chunk(2048) == 0


@pytest.mark.parametrize("alpha", [-1, float("nan"), float("inf"), "8"])
def test_check_implicit_rejects(alpha):
    from movie_recommender_amd.engine import check_implicit
    with pytest.raises(ValueError):
        check_implicit(alpha)


def test_check_implicit_accepts():
    from movie_recommender_amd.engine import check_implicit
    assert check_implicit(0) == 0.0
    assert check_implicit(np.float32(8)) == 8.0


@pytest.mark.parametrize("alpha", [-1, float("nan"), "x"])
def test_context_rejects_before_touching_the_device(alpha, monkeypatch):
    from movie_recommender_amd import _lib
    from movie_recommender_amd.engine import AlsContext

    def no_native():
        raise AssertionError("native library touched before validation")
    monkeypatch.setattr(_lib, "lib", no_native)
    u = np.zeros(2, np.int32)
    with pytest.raises(ValueError):
        AlsContext(u, u, np.ones(2), 2, 1, 1, implicit_alpha=alpha)
    ctx = AlsContext.__new__(AlsContext)   # no context behind it: nothing native may run
    ctx._h = None
    with pytest.raises(ValueError):
        ctx.set_implicit(alpha)


def test_signatures():
    from movie_recommender_amd import implicit
    from movie_recommender_amd.engine import AlsContext
    p = inspect.signature(AlsContext.__init__).parameters
    assert p["implicit_alpha"].default == 0.0
    assert list(p)[-3:] == ["reg", "reg_mode", "implicit_alpha"]   # appended: positions kept
    sig = inspect.signature(implicit.als_implicit)
    assert list(sig.parameters) == ["user_ids", "item_ids", "confidence", "k", "num_users",
                                    "num_items", "alpha", "reg", "reg_mode", "solver",
                                    "max_iterations", "tol", "seed"]
    d = {n: q.default for n, q in sig.parameters.items()}
    assert (d["alpha"], d["reg"], d["reg_mode"], d["solver"], d["max_iterations"], d["tol"],
            d["seed"]) == (40.0, 0.01, "constant", "cholesky", 15, 1e-4, 0)
    u = np.zeros(2, np.int32)
    for kw in ({"alpha": 0.0}, {"alpha": -2.0}, {"reg": -1.0}, {"reg_mode": "x"}):
        with pytest.raises(ValueError):   # validated before any device is touched
            implicit.als_implicit(u, u, np.ones(2), 2, 1, 1, **kw)


def test_header_declares_the_function():
    from conftest import ROOT
    src = open(os.path.join(ROOT, "include", "mr_als.h")).read()
    assert "int mr_als_set_implicit(mr_als* ctx, double alpha);" in src
