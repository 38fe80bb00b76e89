"""GPU: the gather-Gram kernels' output is bit for bit that of the commit
before the Gram loop was rescheduled (row gathers a full MFMA phase ahead),
and within the Gram parity tolerance of an fp64 NumPy Gram.

tests/golden/gram_bits_parent.json holds SHA-256 digests made by
tests/golden/make_gram_bits.py (cases and what is hashed: its docstring) on
the GPU with that earlier build.  Each case here recomputes them with the
current build: (G, c) of both sides from the unfused kernels, (r0, p0, q0) of
both sides from the start fused into the Gram, and the factors after two
iterations.  k = 32, 33, 48, 64 run gram_kernel<NB = 2, 3, 3, 4>; k = 65 is the
sentinel that the NB = 5 path has not moved.

The value check (fp64 Gram from oracle.als_oracle, <= 2e-5 of the block's
largest entry or 1, as tests/test_gpu_parity.py) keeps a wrong digest file
from hiding a wrong kernel."""
import importlib.util
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_gram_bits",
                                               os.path.join(GOLDEN, "make_gram_bits.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

CASES = [(name, k, chunk) for name in gen.SETS for chunk in gen.CHUNKS for k in gen.KS]


@pytest.fixture(scope="module")
def parent_digests():
    with open(gen.OUT) as f:
        return json.load(f)


def test_edge_set_has_the_counts_it_promises():
    u, i, r, nU, nI, _, _ = gen.rating_set("edge", 64)
    cu = np.bincount(u, minlength=nU)
    assert (nU, nI) == (30, 40)
    assert sorted(set(cu.tolist())) == sorted(gen.COUNTS)
    ci = np.bincount(i, minlength=nI)
    assert ci[-1] == 0 and ci[:-1].min() > 0          # one item without ratings
    assert cu.max() > 64 and ci.max() > 64            # split entities at chunk 64


@pytest.mark.parametrize("name,k,chunk", CASES,
                         ids=[gen.case_id(*c) for c in CASES])
def test_gram_bits_and_values(gpu, parent_digests, name, k, chunk):
    from oracle import als_oracle as O
    dig, ne = gen.compute(name, k, chunk)
    u, i, r, nU, nI, U0, V0 = gen.rating_set(name, k)
    for side, (Gf, cf) in (("users", O.gram_user(u, i, r, V0, k, nU)),
                           ("items", O.gram_item(u, i, r, U0, k, nI))):
        G, c = ne[side]
        gs = np.maximum(np.abs(Gf).max(axis=(1, 2)), 1.0)
        eg = float(np.max(np.abs(G - Gf).max(axis=(1, 2)) / gs))
        cs = np.maximum(np.abs(cf).max(axis=1), 1.0)
        ec = float(np.max(np.abs(c - cf).max(axis=1) / cs))
        print(f"{gen.case_id(name, k, chunk)} {side}: G err {eg:.3e} c err {ec:.3e}")
        assert eg < 2e-5 and ec < 2e-5, (side, eg, ec)
    if name == "edge":
        Gi, ci = ne["items"]
        assert np.all(Gi[-1] == 0) and np.all(ci[-1] == 0)   # the item without ratings
    assert dig == parent_digests[gen.case_id(name, k, chunk)]
