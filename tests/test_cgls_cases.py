"""CPU: the exact least-squares cases of tests/cgls_cases.py are what
tests/test_gpu_cgls_structures.py needs them to be -- exact, holding every
block shape the CSR-stream SpMV treats differently on both A and A^T, long
enough for the workgroups' pipeline to advance -- and their restatement of 0
and 1 CG iterations agrees with the existing oracle."""
import numpy as np
import pytest

import cgls_cases as C
from conftest import rel_err

ALL = [C.zoo] + [lambda c=c: c for c in C.small_cases() + C.degenerate_cases()]
IDS = ["zoo"] + [c.name for c in C.small_cases() + C.degenerate_cases()]


@pytest.mark.parametrize("make", ALL, ids=IDS)
def test_exactness_bounds(make):
    c = make()
    r, p, q = (a.astype(object) for a in (c.r0, c.p0, c.q0))     # Python integers
    assert c.rr0 == int(np.dot(r, r)) and c.pAp == int(np.dot(p, q))
    assert c.abs_pq == int(np.sum(np.abs(p * q)))
    assert 0 <= c.rr0 < 2 ** 52 and 0 <= c.abs_pq < 2 ** 52
    assert c.pAp == int(np.sum(c.t0 * c.t0))        # p.A^T A p = |A p|^2
    assert np.array_equal(c.r0, c.At @ (c.A @ c.x0.astype(np.int64)) - c.b2)


def test_zoo_second_rhs_is_exact():
    z = C.zoo()
    z2 = C.with_rhs(z, *z.rhs2)
    assert 0 < z2.rr0 < 2 ** 52 and z2.abs_pq < 2 ** 52 and z2.rr0 != z.rr0
    assert z.rr0 == C.zoo().rr0                      # the shared case is left unchanged


def _g_of(rows):
    g = 1
    while g < 64 and 2 * g * rows <= 256:
        g *= 2
    return g


@pytest.mark.parametrize("side", ["A", "At"])
def test_zoo_holds_every_block_shape(side):
    z = C.zoo()
    i = 0 if side == "A" else 1
    blocks = C.block_lists(z)[i]
    lengths = C.row_lengths(z)[i]
    shapes = {(r, n) for _, r, _, n in blocks}
    # a row just below, at and just above the tile, each a block of its own
    for n in (2047, 2048, 2049, 4000):
        assert (1, n) in shapes, n
    rows = {r for r, _ in shapes}
    assert (256, 2048) in shapes and (256, 256) in shapes and (256, 7 * 256) in shapes
    assert (2, 2048) in shapes and (128, 2048) in shapes
    # both sides of every row count at which the row-sum group G changes
    for r in (2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256):
        assert r in rows, r
    # the 16-terms-per-thread split (a row of 16 G terms or fewer | more) for
    # every G, inside one block
    split = set()
    for s, r, _, n in blocks:
        if n <= C.TILE:
            g = _g_of(r)
            rl = lengths[s:s + r]
            if rl.min() <= 16 * g < rl.max():
                split.add(g)
    assert split == {1, 2, 4, 8, 16, 32, 64}, split
    # whole blocks of empty rows; blocks that start at an odd non-zero (an
    # 8-byte id load from a 4-byte-aligned base); a last block (of those that
    # hold any) that ends off a multiple of 8, at the arrays' padding
    assert (256, 0) in shapes
    assert sum(1 for _, _, o, n in blocks if o % 2 == 1 and 0 < n <= C.TILE) > 100
    last = [b for b in blocks if b[3] > 0][-1]
    assert last[3] % 8 != 0 and last[2] + last[3] == len(z.ci)
    if side == "At":
        assert blocks[-1] == last and last[3] == 3
    # short and long blocks follow each other in every order, at any distance
    # a grid can have (the stride between a workgroup's blocks): spot-check
    # the limits of the grid
    long_ = np.array([n > C.TILE for _, _, _, n in blocks])
    for gs in (256, 1024, 1280, 2048):
        a, b = long_[:-gs], long_[gs:]
        for pair in ((0, 0), (0, 1), (1, 0), (1, 1)):
            assert np.any((a == pair[0]) & (b == pair[1])), (gs, pair)


def test_zoo_pipeline_advances_twice():
    """More than 2 x the grid's upper limit of blocks on both sides: every
    workgroup takes a third block, so the two-ahead bounds fetch is used."""
    ba, bt = C.block_lists(C.zoo())
    assert len(ba) > 2 * C.MAX_PARTS and len(bt) > 2 * C.MAX_PARTS
    # P's non-empty rows keep their order on the device
    z = C.zoo()
    ne = np.nonzero(np.diff(z.rp[:z.p_rows + 1]) > 0)[0]
    assert np.array_equal(C.device_row_order(z)[:len(ne)], ne)


def test_cut_blocks_is_the_plain_greedy_loop():
    rng = np.random.default_rng(0)
    for trial in range(20):
        L = rng.choice([0, 1, 7, 300, 2047, 2048, 2049, 5000], int(rng.integers(0, 700)),
                       p=[.3, .3, .2, .1, .025, .025, .025, .025])
        off = np.concatenate([[0], np.cumsum(L)])
        want, r = [], 0
        while r < len(L):
            s = r
            if L[r] > C.TILE:
                r += 1
            else:
                while r < len(L) and r - s < C.MAX_ROWS and off[r + 1] - off[s] <= C.TILE:
                    r += 1
            want.append((s, r - s, int(off[s]), int(off[r] - off[s])))
        assert C.cut_blocks(L) == want


@pytest.mark.parametrize("make", ALL, ids=IDS)
@pytest.mark.parametrize("max_it", [0, 1])
def test_restatement_equals_oracle(make, max_it):
    c = make()
    it, x, rr = C.restate(c, max_it)
    xo, ito, rro = C.oracle(c, max_it)
    assert it == ito
    assert abs(rr - rro) <= 1e-12 * max(rro, 1e-300) or rr == rro == 0
    assert rel_err(x, xo) <= 1e-12 if c.cols else len(xo) == 0
    if c.rr0 == 0:
        assert it == 0 and rr == 0 and np.array_equal(x, c.x0)


def test_degenerate_cases_are_degenerate():
    for c in C.degenerate_cases():
        assert len(c.ci) == 0 and c.rr0 == 0
        for max_it in (0, 1, 3):
            xo, ito, rro = C.oracle(c, max_it)
            assert ito == 0 and rro == 0 and np.array_equal(xo, c.x0)
