"""Digests of what the gather-Gram kernels (k = 32 .. 64, NB <= 4; k = 65 as
the NB = 5 sentinel) and the CG start fused into them produce, written to
gram_bits_parent.json.  tests/test_gpu_gram_bits.py recomputes the same
digests with the current build: a change of the Gram loop's schedule must not
move a single bit of G, c, Gs, Gn, r0, p0, q0 or of the factors after two
iterations.

Run on the GPU with the build whose bits are to be pinned (the commit before
a scheduling change), from the repository root:

    python tests/golden/make_gram_bits.py

Cases: k in {32, 33, 48, 64, 65} x Gram chunk {2048, 64} x two rating sets:
  edge: 30 users x 40 items; user u has COUNTS[u % 14] ratings (1 .. 161: no
        loop trip, one trip, several, a full and a partial last 32-rating
        half, the prefetch three halves ahead running past the end), drawn
        with repetition from items 0 .. 38 (item 39 has no ratings); at chunk
        64 the users above 64 ratings and the heavy items are split into slab
        records;
  hash: the 400 x 300 / 30,000-draw set of the former tools/probes/g_hash.py.
Per case, SHA-256 of: normal_equations() of both sides after
build_normal_equations (the unfused kernels), cg_vectors() of both sides after
a half-step with max_iteration = 0 (the fused start: r0, p0, q0), and
get_factors() after iterate(2).
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "gram_bits_parent.json")

KS = (32, 33, 48, 64, 65)
CHUNKS = (2048, 64)
SETS = ("edge", "hash")
COUNTS = (1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 128, 129, 160, 161)


def case_id(name, k, chunk):
    return f"{name}_k{k}_c{chunk}"


def rating_set(name, k):
    """(u, i, r, nU, nI, U0, V0): ids int32, ratings and start factors fp64
    holding fp32-exact factor values (set_factors rounds to fp32)."""
    if name == "edge":
        rng = np.random.default_rng(1000 + k)
        nU, nI = 30, 40
        us, its = [], []
        for u in range(nU):
            n = COUNTS[u % len(COUNTS)]
            us.append(np.full(n, u))
            its.append(rng.integers(0, nI - 1, n))     # item nI - 1: no ratings
        u = np.concatenate(us).astype(np.int32)
        i = np.concatenate(its).astype(np.int32)
        perm = rng.permutation(len(u))                 # not sorted by user
        u, i = u[perm], i[perm]
    else:
        rng = np.random.default_rng(k)
        nU, nI, n = 400, 300, 30000
        u = rng.integers(0, nU, n).astype(np.int32)
        i = (rng.zipf(1.3, n) % nI).astype(np.int32)
        key = np.unique(u.astype(np.int64) * nI + i)
        u = (key // nI).astype(np.int32)
        i = (key % nI).astype(np.int32)
    r = rng.normal(0, 1, len(u))
    U0 = rng.uniform(-1, 1, nU * (k + 1)).astype(np.float32).astype(np.float64)
    V0 = rng.uniform(-1, 1, nI * k).astype(np.float32).astype(np.float64)
    return u, i, r, nU, nI, U0, V0


def sha(*arrs):
    m = hashlib.sha256()
    for a in arrs:
        m.update(np.ascontiguousarray(a).tobytes())
    return m.hexdigest()


def compute(name, k, chunk):
    """(digests, normal equations {side: (G, c)}) of one case on the GPU with
    the library that is loaded."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from movie_recommender_amd import _lib
    from movie_recommender_amd.engine import AlsContext
    u, i, r, nU, nI, U0, V0 = rating_set(name, k)
    dig, ne = {}, {}
    try:
        with AlsContext(u, i, r, k, nU, nI, gram_chunk=chunk) as ctx:
            for side, nE in (("users", nU), ("items", nI)):
                ctx.set_factors(U0, V0)
                ctx.build_normal_equations(side)
                G, c = ctx.normal_equations(side, np.arange(nE))
                ne[side] = (G, c)
                dig["ne_" + side] = sha(G, c)
            for side in ("users", "items"):
                ctx.set_factors(U0, V0)
                ctx.half_step(side, 0.01, 0)
                dig["cg_" + side] = sha(*ctx.cg_vectors(side))
            ctx.set_factors(U0, V0)
            ctx.iterate(2)
            dig["factors"] = sha(*ctx.get_factors())
    finally:
        _lib.check(_lib.lib().mr_set_gram_chunk(2048), "reset chunk")
    return dig, ne


def main():
    out = {}
    for name in SETS:
        for chunk in CHUNKS:
            for k in KS:
                out[case_id(name, k, chunk)] = compute(name, k, chunk)[0]
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {OUT}: {len(out)} cases")


if __name__ == "__main__":
    main()
