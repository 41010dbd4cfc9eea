"""The case list of the second field family's product, size and switch tests (crt_cases.py) stays complete: every column length, every
class of the prime-factor index maps, every reachable kernel choice, exponents the constructor takes, the worst-case input inside the
design's range, and a pin for every exponent too large for Python integers.  CPU only."""
import itertools
import json
import math

import pytest

import crt_cases as cc


def test_every_column_length_and_every_index_map_class():
    assert len(cc.CASES) == len(set(cc.CASES)) == 21
    h1 = {1 << cc.grid_of(ln)[0] for odd, ln in cc.CASES if odd == 1}
    assert h1 == {1 << k for k in range(1, 12)}                                  # H1 = 2 .. 2048 with rows of 1024
    assert all(cc.grid_of(ln)[1] == 10 for _, ln in cc.CASES)
    assert {(1 << ln) % 3 for odd, ln in cc.CASES if odd == 3} == {1, 2}           # gr.mm, gr.minv for odd = 3
    assert {(1 << ln) % 9 for odd, ln in cc.CASES if odd == 9} == {1, 2, 4, 5, 7, 8}   # the six classes of 2^ln mod 9 (period 6 in ln)
    assert {ln % 6 for odd, ln in cc.CASES if odd == 9} == set(range(6))
    assert set(cc.SWITCH_CASES) <= set(cc.CASES) and {c for c in cc.CASES if c[0] == 1} <= set(cc.SWITCH_CASES)
    assert {(3, 13), (9, 14), (3, 21), (9, 20)} <= set(cc.SWITCH_CASES)


def test_the_switch_matrix_reaches_every_kernel_choice():
    settings = list(itertools.product(cc.KERNEL_SETS, cc.TUNES))
    assert len(settings) == 16
    got = {}
    for (odd, ln), (ks, tune) in itertools.product(cc.SWITCH_CASES, settings):
        got.setdefault(cc.kernels_of_case(odd, ln, ks, tune), []).append((odd, ln, ks, tune))
    # everything the rule can return for any grid the constructor can make
    reachable = {cc.choose_kernels(odd, logH1, logH2, ks, tune)
                 for odd in (1, 3, 9) for logH2 in range(1, 11) for logH1 in range(0, 12) for ks, tune in settings}
    assert set(got) == reachable == {(r8, sp, fu) for r8, sp in ((False, False), (True, False), (True, True)) for fu in (False, True)}
    H1 = lambda ln: 1 << cc.grid_of(ln)[0]
    split = {(odd, H1(ln)) for t, runs in got.items() if t[1] for odd, ln, ks, tune in runs if ks == "split"}
    assert {(1, 8), (1, 2048), (3, 1024), (9, 512)} <= split                     # a whole row to a work-group; CA61 = 2; the C4 sizes
    for odd, ln in cc.SWITCH_CASES:                                              # the silent fallback below H1 = 8
        assert cc.kernels_of_case(odd, ln, "split", 0)[1] == (H1(ln) >= 8)
    assert {H1(ln) for odd, ln in cc.SWITCH_CASES if H1(ln) < 8} == {2, 4}
    joint = {H1(ln) for t, runs in got.items() if t[0] and not t[1] for odd, ln, ks, tune in runs if ks == "joint"}
    assert {1024, 2048} <= joint                                                 # k_cols_fast at CA = 2 and 1: the default is split there
    assert all(cc.kernels_of_case(1, ln)[1] == (H1(ln) >= 1024) for ln in range(12, 23))
    for odd in (3, 9):                                                           # back + carry in one kernel and in two
        forms = {cc.kernels_of_case(o, ln, None, tune)[2] for o, ln in cc.SWITCH_CASES if o == odd for tune in cc.TUNES}
        assert forms == {True, False}
    assert not any(cc.kernels_of_case(1, ln, None, tune)[2] for ln in range(12, 23) for tune in cc.TUNES)   # odd = 1 has no fused form
    assert cc.algorithmic_bytes(8, True) == 8 * 112 and cc.algorithmic_bytes(8, False) == 8 * 136


@pytest.mark.parametrize("odd,ln", cc.CASES, ids=[cc.case_id(c) for c in cc.CASES])
def test_exponents_pass_the_constructor(odd, ln):
    n = odd << ln
    top, low = cc.p_top(odd, ln), cc.p_low(odd, ln)
    assert top % 2 == low % 2 == 1 and low < top < 2**32
    assert cc.constructor_accepts(top, n) and cc.constructor_accepts(low, n)
    assert not cc.constructor_accepts(top + 2, n)                                # the top of the range
    assert low // n == 15 and (low - 2) // n == 14 and not cc.constructor_accepts(low - 2, n)   # and its bottom


# p_top worked out by hand from the size rule (bits per word 39.0 at 2^12 down to 34.0 at 2^22, 33.7 at 3 2^21, 33.4 at 9 2^20), with two
# comparison sizes that are not cases
TABLE = {(1, 12): 159743, (1, 13): 315391, (1, 14): 622591, (1, 15): 1228799, (1, 16): 2424831, (1, 17): 4784127, (1, 18): 9437183,
         (1, 19): 18612223, (1, 20): 36700159, (1, 21): 72351743, (1, 22): 142606335, (3, 12): 469493, (3, 18): 27688319,
         (3, 21): 212069371, (9, 12): 1379267, (9, 18): 81195259, (9, 20): 315343857}


def test_p_top_matches_the_table():
    for (odd, ln), p in TABLE.items():
        assert cc.p_top(odd, ln) == p, (odd, ln)


@pytest.mark.parametrize("odd,ln", [c for c in cc.CASES if c[1] <= 18], ids=[cc.case_id(c) for c in cc.CASES if c[1] <= 18])
def test_the_worst_case_input_stays_inside_the_design(odd, ln):
    """Mp - 1 at p_top: the largest convolution coefficient stays half a bit under log2(M61 M31) (a float FFT is good to about 1e-10
    relative here; the sizes leave about 0.9 bit), so a failure of the all-maximum input on the GPU is a kernel bug, not the size rule's"""
    n, p = odd << ln, cc.p_top(odd, ln)
    bits = cc.worst_coefficient_bits(p, n)
    print("odd=%d ln=%d p_top=%d bits/word=%.1f log2 max coefficient=%.4f" % (odd, ln, cc.p_top(odd, ln), cc.p_top(odd, ln) / (odd << ln), bits))
    # (from below: a coefficient sums n products of digits of at least 2^q - 2, weights of at least 1, and loses a weight below 2)
    assert math.log2(n) + 2 * (p // n - 1) - 1 < bits < cc.LIMIT_BITS - 0.5


def test_every_large_exponent_has_its_pins():
    with open(cc.PIN_PATH) as f:
        doc = json.load(f)
    assert set(doc) == {"_source", "pins"}
    want = {cc.pin_key(*r): r for r in cc.pinned_runs()}
    assert set(doc["pins"]) == set(want)
    for key, (odd, ln, which) in want.items():
        pin = doc["pins"][key]
        assert set(pin) == {"odd", "ln", "p", "seed"} | set(cc.STEPS)
        assert (pin["odd"], pin["ln"], pin["p"], pin["seed"]) == (odd, ln, cc.exponent(odd, ln, which), cc.seed_of(odd, ln))
        assert pin["p"] > cc.PIN_THRESHOLD
        for s in cc.STEPS:
            assert len(pin[s]["res64"]) == 16 and len(pin[s]["sha256_words"]) == 64
    assert all(cc.exponent(*r) <= cc.PIN_THRESHOLD for r in cc.runs() if cc.pin_key(*r) not in want)
    # the switch test runs at p_top only, on cases of the list: nothing more to pin
    assert all((odd, ln, "top") in cc.runs() for odd, ln in cc.SWITCH_CASES)


def test_the_seeded_operands_and_the_integer_checker():
    """the operands are what the pins describe (low p bits, little-endian) and the integer path of `expected` is plain arithmetic"""
    odd, ln, which = 1, 12, "top"
    p = cc.exponent(odd, ln, which)
    Mp = (1 << p) - 1
    x, y = (cc.int_of(w) for w in cc.operands(odd, ln, which))
    assert 0 < x < Mp and 0 < y < Mp and x != y
    v1 = x * x * cc.A % Mp
    v2 = v1 * y * cc.A % Mp
    want = {"v1": v1, "v2": v2, "xy": x * y % Mp, "v3": (v2 - 2) ** 2 * y % Mp}
    got = cc.expected(odd, ln, which)
    for s, v in want.items():
        assert got[s] == cc.stamp(v.to_bytes(4 * cc.word_count(p), "little")), s
    assert cc.red(Mp, p) == 0 and cc.red(-1, p) == Mp - 1 and cc.red(Mp * Mp + 5, p) == 5
