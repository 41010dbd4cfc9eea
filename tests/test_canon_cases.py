"""The designed carry-chain vectors of tests/canon_cases.py against a plain sequential carry on Python integers, at small geometries
with the stretch structure of the sizes the GPU tests use (tests/test_gpu_canon_chains.py).  No GPU."""
import numpy as np
import pytest

import canon_cases as cc

NAMES = ["thread_block_stretch_edges", "inside_one_stretch_across_its_blocks", "exactly_one_stretch", "several_stretches", "wrap_short",
         "wrap_from_last_stretch", "wrap_lands_on_digit0", "almost_all", "full_loop_mid", "full_loop_0", "full_loop_last", "all_ones",
         "ones_hole_mid", "ones_hole_0", "ones_hole_last", "propagate_without_generate"]


def strong_carry(d, w):
    """carry until none is left, the carry out of the last digit entering digit 0 (2^p = 1); all ones (2^p - 1) is 0"""
    d, w = [int(x) for x in d], [int(x) for x in w]
    c = 0
    while True:
        for j in range(len(d)):
            v = d[j] + c
            d[j] = v & ((1 << w[j]) - 1)
            c = v >> w[j]
        if c == 0:
            break
    if all(dj == (1 << wj) - 1 for dj, wj in zip(d, w)):
        d = [0] * len(d)
    return d


# blocks of 16 digits: 320 blocks (two per stretch, 96 idle threads), 640 (three per stretch, the last stretch holds one), 64 (one)
@pytest.mark.parametrize("n,per,stretches", [(16 * 320, 2, 160), (16 * 640, 3, 214), (16 * 64, 1, 64)])
def test_designed_vectors_are_what_a_sequential_carry_gives(n, per, stretches):
    B = 16
    assert cc.geometry(n, B) == (n // B, per, per * B, stretches)
    w = cc.widths(20 * n + 2 * n // 7 + 1, n)
    assert set(w.tolist()) == {20, 21}
    cs = cc.cases(n, w, B=B)
    assert [c.name for c in cs] == NAMES
    for c in cs:
        assert (c.d <= (np.uint64(1) << w)).all(), c.name
        got = strong_carry(c.d, w)
        if c.zero:
            assert got == [0] * n and np.array_equal(c.t, cc.ones_of(w)), c.name
        else:
            assert got == c.t.tolist(), c.name
        assert np.array_equal(c.d != c.t, c.touched), c.name
        assert (cc.local_passes(c.d, w) <= (np.uint64(1) << w)).all(), c.name   # still a 0/1 chain after the local passes
    m = cc.merged("both", w, ["several_stretches", "wrap_from_last_stretch"], B=B)
    assert strong_carry(m.d, w) == m.t.tolist()


def test_designed_vectors_at_a_real_geometry():
    """n = 5 2^18 with blocks of 4096 (320 blocks, two per stretch): the expected vectors are canonical and differ from the inputs exactly
    on the chains; the inputs are within what the three local passes leave alone."""
    p, n = 27525101, 5 << 18
    w = cc.widths(p, n)
    assert int(w.sum()) == p and set(w.tolist()) == {20, 21}
    assert cc.geometry(n) == (320, 2, 8192, 160)
    table = cc.chain_table(n)
    ones = cc.ones_of(w)
    names = []
    for c in cc.iter_cases(n, w):
        names.append(c.name)
        assert (c.t <= ones).all() and (c.d <= ones + np.uint64(1)).all(), c.name
        assert np.array_equal(c.d != c.t, c.touched), c.name
        on_chains = np.zeros(n, dtype=bool)
        for a, L in table.get(c.name, []):
            on_chains[(a + np.arange(min(L + 1, n))) % n] = True
        if c.name == "propagate_without_generate":
            on_chains[8 * 8192 + 3 + np.arange(8192 + 9 + 1)] = True
            assert (c.t[15 * 8192 - 2:17 * 8192 + 2] == ones[15 * 8192 - 2:17 * 8192 + 2]).all() and c.t[15 * 8192 - 3] == 0
        assert np.array_equal(c.touched, on_chains), c.name
    assert names == NAMES


def test_the_local_passes_model_flags_wide_digits_only():
    """what tests/test_gpu_canon_chains.py relies on to know which path a vector takes: at widths 16-17 three local passes leave digits
    below 2^62 above 2^w (host fallback) and bring digits below 2^(3w - 2) down to at most 2^w (device chain)"""
    p, n = 73751, 9 << 9
    w = cc.widths(p, n)
    assert set(w.tolist()) == {16, 17}
    wide = np.random.default_rng(4).integers(0, 1 << 62, n, dtype=np.uint64)
    assert (cc.local_passes(wide, w) > (np.uint64(1) << w)).any()
    narrow = wide & ((np.uint64(1) << (np.uint64(3) * w - np.uint64(2))) - np.uint64(1))
    assert (cc.local_passes(narrow, w) <= (np.uint64(1) << w)).all()
    # the value is unchanged by a pass
    val = lambda d: sum(int(x) << int(o) for x, o in zip(d, np.concatenate([[0], np.cumsum(w)[:-1]]))) % ((1 << p) - 1)
    assert val(cc.local_passes(wide, w)) == val(wide)
