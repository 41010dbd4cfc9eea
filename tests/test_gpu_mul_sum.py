"""mul_sum (dst <- dst (a + b) for two multiplicand images: the row sweeps' mode 3, or the two-product composition where the plan has no
room for the summed operand) and square_mul_bits, against the oracle running the compositions and against Python integers, on every row
kernel, at the top of a size's exponent range, and on the second field family.  Needs a real MI355X:  python -m pytest tests -m gpu"""
import numpy as np
import pytest

import orc
from mul_sum_cases import CASES, sum_product_ok

pytestmark = pytest.mark.gpu


def Engine(*a, **k):
    from prmers_amd import Engine as E
    return E(*a, **k)


def rand_residue(rng, p):
    return int.from_bytes(rng.bytes((p + 7) // 8), "little") % ((1 << p) - 1)


def plan_c(e):
    return int(e.describe().split(":c=")[1].split(":")[0])


def o_mul_sum(o, dst, a, b, tmp):
    o.copy(tmp, dst); o.mul(dst, a); o.mul(tmp, b); o.add(dst, tmp)


@pytest.mark.parametrize("p,plan", CASES)
def test_mul_sum_matches_the_two_product_composition(p, plan):
    rng = np.random.default_rng(p)
    Mp = (1 << p) - 1
    o = orc.OracleEngine(p, 8)
    with Engine(p, 8, plan=plan) as e:
        assert e.mul_sum_is_fused() == sum_product_ok(p // e.n, e.n, plan_c(e))
        x, y, z = (rand_residue(rng, p) for _ in range(3))
        big = p > 2000000                              # the oracle takes half a second per transform there: the short form
        for eng in (e, o):
            eng.set_int(0, x); eng.set_int(1, y); eng.set_int(2, z)
            eng.square_mul(0, 3); eng.sub(0, 2)        # dst: pending run carries and a small subtraction on top of them
            if not big:
                eng.square_mul(1); eng.square_mul(2, 3)    # the sources are transformed with their run carries pending
            eng.set_multiplicand(3, 1); eng.set_multiplicand(4, 2)
        e.mul_sum(0, 3, 4, 5); o_mul_sum(o, 0, 3, 4, 5)
        assert np.array_equal(e.digits(0), o.digits(0))
        if big:                                        # a squaring on the pending state mul_sum leaves
            for eng in (e, o):
                eng.square_mul(0)
            assert np.array_equal(e.digits(0), o.digits(0))
            return
        for eng in (e, o):
            eng.set_int(6, z)
        want = None
        if p <= 400063:
            want = (3 * x * x - 2) * (y * y + 3 * z * z) % Mp
            assert e.get_int(0) == want
        # the same image twice, on a dst that has the pending state mul_sum leaves; then a squaring on that state
        e.mul_sum(0, 4, 4, 5); o_mul_sum(o, 0, 4, 4, 5)
        assert np.array_equal(e.digits(0), o.digits(0))
        for eng in (e, o):
            eng.square_mul(0)
        assert np.array_equal(e.digits(0), o.digits(0))
        if want is not None:
            assert e.get_int(0) == pow(want * 6 * z * z, 2, Mp)
        # the sources are intact
        for eng in (e, o):
            eng.mul(6, 3); eng.mul(6, 4)
        assert np.array_equal(e.digits(6), o.digits(6))


@pytest.mark.parametrize("p,plan", CASES)
def test_mul_sum_at_the_operand_edges(p, plan):
    Mp = (1 << p) - 1
    rng = np.random.default_rng(p + 1)
    x = rand_residue(rng, p) | 1
    with Engine(p, 8, plan=plan) as e:
        # every digit at its largest value on all three operands: (Mp - 1) (2 (Mp - 1)) = (-1)(-2) = 2
        for r in (0, 1, 2):
            e.set_int(r, Mp - 1)
        e.set_multiplicand(1, 1); e.set_multiplicand(2, 2)
        e.mul_sum(0, 1, 2, 3)
        assert e.get_int(0) == 2
        e.mul_sum(0, 1, 1, 3)                      # 2 (-2) = -4
        assert e.get_int(0) == Mp - 4
        # a + b = Mp as integers: the product is dst Mp, the value Mp itself when dst = 1
        e.set(7, 0)
        for dst in (1, x):
            e.set_int(0, dst); e.set_int(4, x); e.set_int(5, Mp - x)
            e.set_multiplicand(4, 4); e.set_multiplicand(5, 5)
            e.mul_sum(0, 4, 5, 3)
            assert e.get_int(0) == 0 and e.is_equal(0, 7)
        # dst = 0
        e.set(0, 0)
        e.mul_sum(0, 4, 5, 3)
        assert e.get_int(0) == 0 and e.is_equal(0, 7)
        e.mul_sum(0, 4, 4, 3)
        assert e.get_int(0) == 0
        e.set(0, 1)
        e.mul_sum(0, 4, 4, 3)                      # the result is still a usable residue
        assert e.get_int(0) == 2 * x % Mp


def mul_sum_script(e, p):
    """mul_sum on pending run carries and a small subtraction, the same image twice, a squaring on the state that leaves, and every
    digit at its largest value on all three operands (registers 0 .. 5 of e), against Python integers"""
    Mp = (1 << p) - 1
    red = lambda v: orc.mers_reduce(v, p)            # (Python's % is quadratic at a million bits)
    rng = np.random.default_rng(3)
    x, y, z = (rand_residue(rng, p) for _ in range(3))
    e.set_int(0, x); e.set_int(1, y); e.set_int(2, z)
    e.square_mul(0, 3); e.sub(0, 2); e.square_mul(1); e.square_mul(2, 3)
    e.set_multiplicand(3, 1); e.set_multiplicand(4, 2)
    e.mul_sum(0, 3, 4, 5)
    want = red(red(3 * x * x + Mp - 2) * red(y * y + 3 * z * z))
    assert e.get_int(0) == want
    e.mul_sum(0, 4, 4, 5)
    e.square_mul(0)
    assert e.get_int(0) == red(red(red(want * 6) * red(z * z)) ** 2)
    for r in (0, 1, 2):
        e.set_int(r, Mp - 1)
    e.set_multiplicand(1, 1); e.set_multiplicand(2, 2)
    e.mul_sum(0, 1, 2, 3)
    assert e.get_int(0) == 2


def test_mul_sum_on_the_second_family():
    from prmers_amd import CrtEngine
    p = 9941
    with CrtEngine(p, 3, reg_count=8) as e:
        assert not e.mul_sum_is_fused()
        mul_sum_script(e, p)


def _bits(value, nbits):
    return (value << (-nbits % 8)).to_bytes((nbits + 7) // 8, "big")


def _check_square_mul_bits(e, p, factors):
    Mp = (1 << p) - 1
    rng = np.random.default_rng(p)
    for f in factors:
        nbits = 37                                   # not a whole number of bytes
        B = int(rng.integers(1 << 36, 1 << 37)) | 1
        x = rand_residue(rng, p)
        e.set_int(0, x); e.set_int(1, x)
        e.square_mul_bits(0, f, _bits(B, nbits), nbits)
        for i in range(nbits - 1, -1, -1):
            e.square_mul(1, f if (B >> i) & 1 else 1)
        assert e.is_equal(0, 1)
        assert e.get_int(0) == pow(x, 1 << nbits, Mp) * pow(f, B, Mp) % Mp
        e.square_mul_bits(0, f, _bits(0, 5), 5)      # leading zeros: five plain squarings
        assert e.get_int(0) == pow(pow(x, 1 << nbits, Mp) * pow(f, B, Mp), 32, Mp)
        before = e.get_int(0)
        e.square_mul_bits(0, f, b"", 0)              # nothing
        e.square_mul_bits(0, f, b"\xff", 0)
        assert e.get_int(0) == before
    e.set(0, 1)
    E = 2 * p * 3**5 * 5**3 * 7 * 11                 # a stage-1 exponent in miniature: 3^E from the value 1
    e.square_mul_bits(0, 3, _bits(E, E.bit_length()), E.bit_length())
    assert e.get_int(0) == pow(3, E, Mp)


@pytest.mark.parametrize("p,plan", [(9941, "m2=16,c=4"), (300007, "m2=4096")])
def test_square_mul_bits(p, plan):
    with Engine(p, 4, plan=plan) as e:
        _check_square_mul_bits(e, p, (1, 3, 0xFFFFFFFF))   # 2^32 - 1 is above the fused bound at p = 300007 (chi a < 2^64 needs a < 2^30)


def test_square_mul_bits_on_the_second_family():
    from prmers_amd import CrtEngine
    with CrtEngine(9941, 9) as e:
        _check_square_mul_bits(e, 9941, (1, 3, 0xFFFFFFFF))


def test_bad_arguments_are_refused_and_change_nothing():
    from prmers_amd import EngineError
    p = 9941
    with Engine(p, 6, plan="m2=16,c=4") as e:
        e.set(0, 3); e.set(1, 5); e.set(2, 7); e.set(3, 11)
        e.square_mul(0)                              # pending run carries on dst
        e.set_multiplicand(1, 1); e.set_multiplicand(2, 2)
        for bad in (lambda: e.mul_sum(0, 1, 3, 4),   # a residue given as a source
                    lambda: e.mul_sum(0, 3, 2, 4),
                    lambda: e.mul_sum(0, 1, 2, 0),   # tmp == dst
                    lambda: e.mul_sum(0, 1, 2, 1),   # tmp is a source
                    lambda: e.mul_sum(0, 0, 2, 4),   # dst is a source
                    lambda: e.mul_sum(1, 1, 2, 4),   # dst holds an image
                    lambda: e.mul_sum(0, 1, 2, 6), lambda: e.mul_sum(0, 1, 9, 4), lambda: e.mul_sum(6, 1, 2, 4),   # out of range
                    lambda: e.square_mul_bits(6, 3, b"\x80", 1), lambda: e.square_mul_bits(1, 3, b"\x80", 1),
                    lambda: e.square_mul_bits(0, 0, b"\x80", 1)):
            with pytest.raises(EngineError):
                bad()
        with pytest.raises(ValueError):
            e.square_mul_bits(0, 3, b"\x80", 9)      # more bits than bytes given
        assert e.get_int(0) == 9 and e.get_int(3) == 11
        e.mul_sum(0, 1, 2, 4)                        # and the registers still work: 9 (5 + 7)
        assert e.get_int(0) == 108
        e.mul(3, 1); e.mul(3, 2)
        assert e.get_int(3) == 11 * 35
