"""square_mul_prepare (img_out <- the multiplicand image of src, src <- src^2 factor: the row sweeps' mode 4) against the oracle running
set_multiplicand + square_mul, against Python integers at the operand edges, and on registers with pending state, on every row kernel and
on the second field family.  Needs a real MI355X:  python -m pytest tests -m gpu"""
import numpy as np
import pytest

import orc
from mul_sum_cases import CASES

pytestmark = pytest.mark.gpu

BIG_FACTOR = 0xFFFFFFFF      # above the fused bound of every plan that has one below 2^32 (2^30 at p = 300007, 7254967 at p = 136279841)
FACTORS = (1, 3, BIG_FACTOR)


def Engine(*a, **k):
    from prmers_amd import Engine as E
    return E(*a, **k)


def rand_residue(rng, p):
    return int.from_bytes(rng.bytes((p + 7) // 8), "little") % ((1 << p) - 1)


@pytest.mark.parametrize("p,plan", CASES)
def test_square_and_image_match_the_oracle(p, plan):
    rng = np.random.default_rng(p + 4)
    Mp = (1 << p) - 1
    x, y = rand_residue(rng, p), rand_residue(rng, p)
    o = orc.OracleEngine(p, 4)
    o.set_int(0, x); o.set_int(1, y)
    o.set_multiplicand(2, 0); o.mul(1, 2)                  # y x, once: the three images below must all stand for x
    want_y = o.digits(1)
    with Engine(p, 10, plan=plan) as e:
        assert e.square_mul_prepare_is_fused() is True
        # image registers: 3 held an image before, 4 a residue with pending run carries, 5 nothing
        e.set_int(9, y); e.set_multiplicand(3, 9)
        e.set_int(4, y); e.square_mul(4)
        for i, f in enumerate(FACTORS):
            src, img, yr = i, 3 + i, 6 + i
            e.set_int(src, x); e.set_int(yr, y)
            e.square_mul_prepare(src, img, f)
            e.mul(yr, img)
            if f == BIG_FACTOR:
                # the oracle multiplies in 64 bits and overflows above the fused bound (oracle/oracle.c adc_mul): its x^2 times the
                # factor as integers instead, the same words
                assert e.get_int(src) == x2 * f % Mp, f
            else:
                o.set_int(3, x); o.square_mul(3, f)
                assert np.array_equal(e.digits(src), o.digits(3)), f
                if f == 1:
                    x2 = o.get_int(3)
            assert np.array_equal(e.digits(yr), want_y), f
        if p <= 400063:
            assert x2 == x * x % Mp and e.get_int(8) == x * y % Mp
        # the image survives further use, and src is a residue that squares on
        e.set_int(9, y); e.mul(9, 3)
        assert np.array_equal(e.digits(9), want_y)
        if p < 2000000:                                    # (the oracle takes half a second per transform above)
            e.square_mul(1, 3); o.set_int(3, x); o.square_mul(3, 3); o.square_mul(3, 3)
            assert np.array_equal(e.digits(1), o.digits(3))


def times_small(k, y, p):
    """k y mod 2^p - 1 for a small k: one linear multiplication and a fold (a % of numbers this long would take minutes)"""
    return orc.mers_reduce(k * y, p)


@pytest.mark.parametrize("p,plan", CASES)
def test_operand_edges_against_integers(p, plan):
    """x in {0, 1, 2, Mp - 1, the all-ones digit vector}: x^2 is 0, 1, 4, 1, 0 and x y is 0, y, 2 y, -y, 0, so every expected value is a
    small multiple of y folded modulo 2^p - 1 and costs nothing at any exponent"""
    Mp = (1 << p) - 1
    rng = np.random.default_rng(p + 5)
    y = rand_residue(rng, p) | 1
    with Engine(p, 4, plan=plan) as e:
        e.set(0, 0)
        for x, xsq, xy in ((0, 0, 0), (1, 1, y), (2, 4, times_small(2, y, p)), (Mp - 1, 1, Mp - y), ("ones", 0, 0)):
            if x == "ones":                                # every digit at its largest value: the integer 2^p - 1, which is 0
                w = e.digits(0) >> np.uint64(32)
                e.set_digits(0, ((np.uint64(1) << w) - np.uint64(1)) | (w << np.uint64(32)))
            else:
                e.set_int(0, x)
            e.set_int(1, y)
            e.square_mul_prepare(0, 2, 3)
            e.mul(1, 2)
            assert e.get_int(0) == 3 * xsq, x              # at most 12: below 2^p - 1 at every exponent of the cases
            assert e.get_int(1) == xy, x
            e.square_mul_prepare(0, 2, 1)                  # and once more on the state that leaves
            e.set_int(1, y); e.mul(1, 2)
            assert e.get_int(0) == 9 * xsq * xsq and e.get_int(1) == times_small(3 * xsq, y, p), x


@pytest.mark.parametrize("p,plan", CASES)
def test_pending_state_goes_into_the_image(p, plan):
    """The image must be the one set_multiplicand(img, src) would write at that moment: after a small subtraction, and while the run
    carries of a chain of squarings are outstanding.  Reference: the composition on a copy of the register (copy keeps the pending
    state), and Python integers where they are cheap."""
    Mp = (1 << p) - 1
    rng = np.random.default_rng(p + 6)
    x, y = rand_residue(rng, p), rand_residue(rng, p)
    with Engine(p, 8, plan=plan) as e:
        for state in ("sub", "chain"):
            e.set_int(0, x); e.set_int(1, y); e.set_int(5, y)
            if state == "sub":
                e.sub(0, 2)
                v = (x - 2) % Mp
            else:
                e.square_mul_n(0, 3, 3)
                v = None
            e.copy(4, 0)
            e.square_mul_prepare(0, 2, 3); e.mul(1, 2)
            e.set_multiplicand(6, 4); e.square_mul(4, 3); e.mul(5, 6)
            assert np.array_equal(e.digits(0), e.digits(4)), state
            assert np.array_equal(e.digits(1), e.digits(5)), state
            if p <= 400063:
                if v is None:
                    v = x
                    for _ in range(3):
                        v = 3 * v * v % Mp
                assert e.get_int(0) == 3 * v * v % Mp and e.get_int(1) == v * y % Mp, state


def square_prepare_script(e, p):
    """square_mul_prepare after a small subtraction at every factor: the square and a product by the image (registers 0 .. 2 of e)"""
    red = lambda v: orc.mers_reduce(v, p)            # (Python's % is quadratic at a million bits)
    rng = np.random.default_rng(11)
    x, y = rand_residue(rng, p), rand_residue(rng, p)
    for f in FACTORS:
        e.set_int(0, x); e.set_int(1, y)
        e.sub(0, 2)
        e.square_mul_prepare(0, 2, f); e.mul(1, 2)
        assert e.get_int(0) == red(red((x - 2) ** 2) * f) and e.get_int(1) == red((x - 2) * y), f


def test_second_family_runs_the_composition_with_the_same_values():
    from prmers_amd import CrtEngine
    p = 9949
    got = []
    for make in (lambda: CrtEngine(p, 9, n=576, reg_count=6), lambda: Engine(p, 6)):
        with make() as e:
            got.append(e.square_mul_prepare_is_fused())
            square_prepare_script(e, p)
    assert got == [False, True]


def test_bad_arguments_are_refused_and_change_nothing():
    from prmers_amd import EngineError
    p = 9941
    with Engine(p, 5, plan="m2=16,c=4") as e:
        e.set(0, 3); e.set(1, 5); e.set(2, 7); e.set(3, 11); e.set(4, 13)
        e.square_mul(0)                              # pending run carries on src
        e.set_multiplicand(2, 2)
        for bad in (lambda: e.square_mul_prepare(0, 0),        # img_out == src
                    lambda: e.square_mul_prepare(2, 1),        # src holds an image
                    lambda: e.square_mul_prepare(0, 1, 0),     # factor 0
                    lambda: e.square_mul_prepare(0, 5), lambda: e.square_mul_prepare(5, 1), lambda: e.square_mul_prepare(0, 2**40)):
            with pytest.raises(EngineError):
                bad()
        with pytest.raises(ValueError):
            e.square_mul_prepare(0, 1, 2**32)
        assert [e.get_int(r) for r in (0, 1, 3, 4)] == [9, 5, 11, 13]
        e.mul(3, 2)                                  # register 2 is still the image of 7
        assert e.get_int(3) == 77
        e.square_mul_prepare(0, 1, 2)                # and the operation still works: 1 <- image of 9, 0 <- 162
        e.mul(4, 1)
        assert e.get_int(0) == 162 and e.get_int(4) == 117
