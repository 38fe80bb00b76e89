"""CPU: every input that tests/test_gpu_serving_edges.py sends through the
top-N select reaches the path it was designed for.  The path is worked out by
``serving_cases.select_walk``, a host restatement of the select's documented
rule; the device cannot be asked which path it took, so this test is what
keeps the GPU test from silently losing a path when an input is edited."""
import numpy as np
import pytest

from serving_cases import (SEL_BINS, exact_scores, select_exclusions, select_inputs, select_walk,
                           signs_input, value_table)

INPUTS = select_inputs()


def walk(inp, excluded=(), x0=1.0):
    mids = np.asarray(inp["mids"])
    mask = np.array([int(m) in excluded for m in mids]) if excluded else None
    return select_walk(x0 * inp["values"] + 0.0, mids, inp["N"], mask)


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_value_table_scores_are_the_values(name):
    """k = 1, user [x0, 0], medians 0: the exact score is x0 * v, bit for bit."""
    inp = INPUTS[name]
    k, V, als_ids, med = value_table(inp["values"], inp["mids"])
    assert k == 1 and list(med) == [int(m) for m in inp["mids"]]
    S = exact_scores(np.array([[1.0, 0.0], [-1.0, 0.0], [0.5, 0.0]]), V.reshape(-1, 1),
                     np.zeros(len(V)))
    for row, x0 in zip(S, (1.0, -1.0, 0.5)):
        assert np.array_equal(row.view(np.int64), (x0 * inp["values"]).view(np.int64))


def test_r1_radix_levels_with_elements_above():
    fits, levels, above, straddles, collected = walk(INPUTS["R1"])
    assert not fits and levels >= 3 and above > 0 and not straddles
    assert INPUTS["R1"]["N"] <= collected <= SEL_BINS
    # top of the order excluded: still radix, still a level that starts with
    # elements above; fewer than N left: everything is collected
    top, few = select_exclusions(INPUTS["R1"])[1:]
    fits, levels, above, _, _ = walk(INPUTS["R1"], top)
    assert not fits and levels >= 3 and above > 0
    assert walk(INPUTS["R1"], few)[4] == INPUTS["R1"]["N"] - 7
    # negated, the cluster leads: radix with nothing above
    fits, levels, above, _, _ = walk(INPUTS["R1"], x0=-1.0)
    assert not fits and levels >= 2 and above == 0


def test_r6_forgetting_the_elements_above_overflows():
    """On R1 and R2 a select that left `above` out of the boundary test would
    still collect a superset that fits the buffer, and sort it right; on R6
    it cannot."""
    inp = INPUTS["R6"]
    fits, levels, above, _, collected = walk(inp)
    assert not fits and levels >= 2 and above == 1000 and inp["N"] <= collected <= SEL_BINS
    wrong = select_walk(inp["values"], inp["mids"], inp["N"], count_above=False)
    assert wrong[4] > SEL_BINS
    # the N-th place is inside a 300-way tie
    v = np.sort(inp["values"])[::-1]
    assert v[1000] == v[inp["N"] - 1] == v[inp["N"]] == v[1299] > v[1300]


@pytest.mark.parametrize("name", ["R2", "R2_dense"])
def test_r2_digit_straddles_key_and_id(name):
    inp = INPUTS[name]
    fits, levels, above, straddles, collected = walk(inp)
    assert not fits and straddles and above == 100 and levels >= 6
    assert inp["N"] <= collected <= SEL_BINS
    # the N-th place is inside the tie group: ids decide the cut
    v = np.sort(inp["values"])[::-1]
    assert v[inp["N"] - 1] == v[inp["N"]] == 3.5
    fits, _, above, straddles, _ = walk(inp, select_exclusions(inp)[1])
    assert not fits and straddles and above == 0      # the 100 leaders excluded
    assert walk(inp, select_exclusions(inp)[2])[4] == inp["N"] - 7
    assert walk(INPUTS["R2"])[1] < walk(INPUTS["R2_dense"])[1]   # dense ids: one level deeper


@pytest.mark.parametrize("ids", ["", "_spread"])
def test_r3_fast_path_capacity_boundary(ids):
    for g in (2047, 2048):
        assert walk(INPUTS[f"R3_{g}{ids}"]) == (True, 0, 0, False, g)
    assert SEL_BINS == 2048
    inp = INPUTS[f"R3_2049{ids}"]
    fits, levels, above, straddles, collected = walk(inp)
    assert not fits and straddles and levels >= 5 and inp["N"] <= collected <= SEL_BINS
    # 30 of the tie group excluded: 2,019 left, back on the fast path
    assert walk(inp, select_exclusions(inp)[1]) == (True, 0, 0, False, 2019)
    # negated, the 3,000 lower ties lead: radix at every g
    for g in (2047, 2048, 2049):
        fits, _, _, straddles, _ = walk(INPUTS[f"R3_{g}{ids}"], x0=-1.0)
        assert not fits and straddles


def test_r5_one_level_on_the_ids_top_bits():
    inp = INPUTS["R5"]
    for ex in select_exclusions(inp):
        fits, levels, above, straddles, collected = walk(inp, ex)
        assert (fits, levels, above, straddles) == (False, 1, 0, False)
        assert collected <= SEL_BINS
    assert walk(inp, select_exclusions(inp)[2])[4] == inp["N"] - 7
    top = np.sort(inp["mids"])[::-1][:inp["N"] + 1] >> 21        # id bits 31..21
    assert top.max() >= 1 << 9 and len(set(top.tolist())) > 50   # set, and deciding


def test_signs_input_paths():
    inp = signs_input()
    v, mids = inp["values"], np.asarray(inp["mids"])
    assert (v < 0).sum() == (v > 0).sum() == 3000 and (v == 0).sum() == 100
    assert np.signbit(v[v == 0]).sum() == 50

    def w(u, n):
        x0, ex = inp["users"][u]
        mask = np.array([int(m) in ex for m in mids])
        return select_walk(x0 * v + 0.0, mids, n, mask), int(((x0 * v > 0) & ~mask).sum())

    (fits, *_), n_pos = w(0, 400)
    assert fits and n_pos == 3000
    (fits, levels, above, _, _), _ = w(1, 400)        # keys differ in the first bit
    assert not fits and levels >= 3 and above == 0
    (fits, levels, _, _, _), _ = w(2, 400)            # all +0.0: ids only
    assert not fits and levels == 1
    (fits, *_), n_pos = w(3, 400)                     # place 400 is a zero
    assert fits and n_pos < 400 < n_pos + 100
    (fits, levels, above, _, _), n_pos = w(4, 400)    # place 400 is in the negative cluster
    assert not fits and levels >= 3 and above == n_pos + 100 == 200
