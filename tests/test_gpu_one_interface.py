"""Both field families behind the one register-machine interface (prmers_amd/csrc/register_machine.hpp): the same script of composed
operations through the C ABI on a Goldilocks engine and on two GF(M61^2) x GF(M31^2) engines, every register against Python integers, and
the same refusals, each of which leaves every register as it was.  Needs a real MI355X:  python -m pytest tests -m gpu"""
import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu

P, REGS = 9941, 6
MP = (1 << P) - 1
SPECS = ["", "crt:9", "crt:3"]   # Goldilocks with its automatic plan, the prime-factor axis of radix 9 and of radix 3


def make(spec):
    from prmers_amd import Engine
    return Engine(P, REGS, plan=spec or None)


def start_values(seed, p=P):
    rng = np.random.default_rng(seed)
    return [int.from_bytes(rng.bytes((p + 7) // 8), "little") % ((1 << p) - 1) for _ in range(REGS)]


def red(v, p):
    """v mod 2^p - 1 by folding: Python's % is quadratic at a million bits and more"""
    return orc.mers_reduce(v + ((1 << p) - 1) if v < 0 else v, p)


def pow_red(v, k, p):
    r = 1
    for i in range(int(k).bit_length() - 1, -1, -1):
        r = red(r * r, p)
        if (k >> i) & 1:
            r = red(r * v, p)
    return r


def check(e, model, what):
    """every register that holds a residue (model[r] is not None) against its integer"""
    for r, v in enumerate(model):
        if v is not None:
            assert e.get_int(r) == red(v, e.p), (what, r)


def composed_script(make, p=P):
    """square_mul_n, a checkpoint into a fresh engine, mul_add / mul_copy / square_mul_copy at factor 3, exp_mul, exp_mul2 and
    square_mul_bits on the engines make() creates (REGS registers at exponent p), every register against Python integers"""
    MP = (1 << p) - 1
    v = start_values(1, p)
    with make() as e:
        for r in range(REGS):
            e.set_int(r, v[r])
        v[1] = v[0]; e.copy(1, 0)
        # square_mul_n in one call against the same steps one by one
        e.square_mul_n(0, 5, a=3, sub=2)
        for _ in range(5):
            e.square_mul(1, 3); e.sub(1, 2)
            v[1] = red(red(v[1] * v[1], p) * 3 - 2, p)
        v[0] = v[1]
        check(e, v, "square_mul_n")
        assert e.is_equal(0, 1)
        # checkpoint out and into a fresh engine of the same spec; register 5 travels as a multiplicand image
        image = v[4]
        e.set_multiplicand(5, 4)
        ck = e.get_checkpoint()
        assert ck.size == e.get_checkpoint_size() == REGS * e.get_register_data_size()
    with make() as e:
        assert e.set_checkpoint(ck)
        v[5] = None
        check(e, v, "checkpoint")
        assert not e.set_checkpoint(ck[:-1])
        # the compositions, at factor 3, multiplying by the image that came through the checkpoint
        e.mul_add(0, 5, 1, 3); v[0] = red(v[0] * image, p) * 3 + v[1]
        check(e, v, "mul_add")
        e.mul_copy(1, 5, 2, 3); v[1] = v[2] = red(v[1] * image, p) * 3
        check(e, v, "mul_copy")
        e.square_mul_copy(2, 3, 3); v[2] = v[3] = red(v[2] * v[2], p) * 3
        check(e, v, "square_mul_copy")
        # a = a^h b: b and tmp end as multiplicand images
        for h, b in ((0, 12345), (1, v[4]), (0b1011, MP - 7)):
            e.set_int(3, b)
            e.exp_mul(0, h, 3, 5)
            v[0] = pow_red(red(v[0], p), h, p) * b; v[3] = None
            check(e, v, "exp_mul h=%d" % h)
            for r in (3, 5):
                with pytest.raises(Exception, match="multiplicand"):
                    e.square_mul(r)
        e.set_int(3, 3)
        e.exp_mul2(0, 2, 3, 5); v[0] = red(v[0] * v[0], p) * 9
        check(e, v, "exp_mul2")
        # reg^(2^9) * 3^B for the nine bits 1 0110 0101
        e.square_mul_bits(1, 3, bytes([0b10110010, 0b10000000]), 9)
        v[1] = pow_red(red(v[1], p), 1 << 9, p) * pow_red(3, 0b101100101, p)
        check(e, v, "square_mul_bits")


@pytest.mark.parametrize("spec", SPECS)
def test_the_same_script_on_both_families(spec):
    composed_script(lambda: make(spec))


@pytest.mark.parametrize("spec", SPECS)
def test_a_refused_call_leaves_every_register_as_it_was(spec):
    v = start_values(2)
    with make(spec) as e:
        for r in range(REGS):
            e.set_int(r, v[r])
        before = [e.get_words(r) for r in range(REGS)]
        refused = [
            (lambda: e.exp_mul(0, 5, 1, 0), "three different"),      # a == tmp
            (lambda: e.mul(0, 1), "multiplicand"),                   # register 1 holds a residue, not an image
            (lambda: e.square_mul_bits(0, 0, b"\xff\x80", 9), "factor"),
        ]
        for call, pattern in refused:
            with pytest.raises(Exception, match=pattern):
                call()
            for r in range(REGS):
                assert np.array_equal(e.get_words(r), before[r]), (pattern, r)
        check(e, v, "after the refusals")
