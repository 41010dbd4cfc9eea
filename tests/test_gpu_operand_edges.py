"""Operand edges of the register machine against Python integers (never against the oracle, which restates the same 64-bit carry).

Factors: every entry that takes one, at factors from 1 to 2^32 - 1, followed by plain squarings and a mul that consume the carries a
large factor leaves pending.  Subtraction: sparse registers (0, 1, 2^k at the digit / run / column edges) minus values up to 2^32 - 1,
followed by every kind of operation, with and without pending run carries.  Full size: the largest exponent of each transform size
(all digits at their maximum), closed forms and an identity instead of big squarings.  The second field family takes the same matrix.
"""
import random
import zlib

import numpy as np
import pytest

import orc
from prmers_amd import CrtEngine, Engine, resolve_plan

pytestmark = pytest.mark.gpu

# one shape per kernel set (plans of test_gpu_parity.SMALL_CASES): label -> (p, plan, expected plan text)
SHAPES = {
    "generic-c1": (86243, "m2=16,c=1", "n=4096:m1=128:m2=16:c=1"),
    "generic-c2": (102701, "m2=64,c=2", "n=5120:m1=40:m2=64:c=2"),
    "radix8-cols": (300007, "m2=8,c=4", "n=16384:m1=1024:m2=8:c=4"),
    "radix8-rows4096": (300007, "m2=4096", "n=16384:m1=2:m2=4096:c=16"),
    "radix4-cols256": (86243, "m2=8,c=4", "n=4096:m1=256:m2=8:c=4"),
    "radix4-rows1024": (300007, "m2=1024", "n=16384:m1=8:m2=1024:c=4"),
    "rows2048-planes": (300007, "m2=2048", "n=16384:m1=4:m2=2048:c=8"),
    "radix5-cols1280": (400063, "m2=8,c=4", "n=20480:m1=1280:m2=8:c=4"),
    "radix5-cols2560": (800283, "m2=8,c=2", "n=40960:m1=2560:m2=8:c=2"),
    "rows8192": (300007, "m2=8192", "n=16384:m1=1:m2=8192:c=16"),
    "split5": (53331, "m2=16,split5", "n=2560:m1=80:m2=16:c=1:split5"),
}
_rng = random.Random(20261016)
FACTORS = [1, 2, 3, 15, 16, 17, 255, 2**16 + 1, 2**20 + 1, 2**24 + 1, 2**28 + 1, 2**31, 2**32 - 1] + \
          [_rng.randrange(2**20, 2**32) for _ in range(3)]
SUBS = [1, 2, 3, 2**16, 2**30 - 1, 2**30, 2**32 - 1]
ENTRIES = ["square_mul", "mul", "square_mul_copy", "mul_copy", "mul_add", "square_mul_n"]
FOLLOW = ["square_mul", "square_mul_n", "mul_dst", "mul_src", "copy_square", "add"]


def _plan(p, spec):
    text = resolve_plan(p, spec)
    return {k: int(v) for k, v in (t.split("=") for t in text.split(":")[1:] if "=" in t)}


def _bit_of_digit(p, n, j):
    return -(-p * j // n)   # ceil(p j / n): first bit of natural digit j


def _sparse_positions(p, spec):
    """2^k at: the top bit of digit 0, the first digit of run 1 (2C digits in), the first digit of column 1 (a tile's second run
    of the same tile: natural digit 2 M2), the top bit of the value"""
    pl = _plan(p, spec)
    n, c, m2 = pl["n"], pl["c"], pl["m2"]
    return sorted({_bit_of_digit(p, n, 1) - 1, _bit_of_digit(p, n, 2 * c), _bit_of_digit(p, n, 2 * m2), p - 1})


def _red(v, p):
    """v mod 2^p - 1 by shifts (Python's % on numbers of this size is quadratic)"""
    return orc.mers_reduce(v + ((1 << p) - 1) if v < 0 else v, p)


def _assert_value(e, r, want, what):
    assert e.get_int(r) == _red(want, e.p), what


# ---- factor matrix on the small shapes --------------------------------------------------------------------------------------------

def _factor_case(e, entry, a, x, y, z):
    """runs `entry` with factor a on x (multiplicand y, addend z), then two squarings and a mul by y; returns (want, [registers])"""
    p = e.p
    e.set_int(5, y); e.set_multiplicand(2, 5)
    e.set_int(0, x)
    if entry == "square_mul":
        e.square_mul(0, a); want = x * x * a
    elif entry == "mul":
        e.mul(0, 2, a); want = x * y * a
    elif entry == "square_mul_copy":
        e.square_mul_copy(0, 3, a); want = x * x * a
    elif entry == "mul_copy":
        e.mul_copy(0, 2, 3, a); want = x * y * a
    elif entry == "mul_add":
        e.set_int(4, z); e.mul_add(0, 2, 4, a); want = x * y * a + z
    else:
        e.square_mul_n(0, 3, a, 2); want = x
        for _ in range(3):
            want = _red(_red(want * want, p) * a - 2, p)
    want = _red(want, p)
    copy_want = want if entry in ("square_mul_copy", "mul_copy") else None
    e.square_mul(0); e.square_mul(0); e.mul(0, 2)
    want = _red(want * want, p)
    want = _red(_red(want * want, p) * y, p)
    return want, copy_want


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_factor_matrix_small_shapes(shape, entry):
    p, spec, text = SHAPES[shape]
    assert resolve_plan(p, spec) == "marin-hip:" + text
    rng = random.Random(zlib.crc32(("%s:%s" % (shape, entry)).encode()))
    Mp = (1 << p) - 1
    with Engine(p, 6, plan=spec) as e:
        for a in FACTORS:
            x, y, z = rng.randrange(Mp), rng.randrange(Mp), rng.randrange(Mp)
            want, copy_want = _factor_case(e, entry, a, x, y, z)
            _assert_value(e, 0, want, (shape, entry, a))
            if copy_want is not None:
                _assert_value(e, 3, copy_want, (shape, entry, a, "copy"))


@pytest.mark.parametrize("shape", ["radix8-cols", "radix5-cols1280"])
def test_factor_matrix_generic_kernel_set(shape, monkeypatch):
    """MI355_KERNELS=generic on shapes the register-resident kernels would take"""
    monkeypatch.setenv("MI355_KERNELS", "generic")
    p, spec, _ = SHAPES[shape]
    rng = random.Random(7)
    Mp = (1 << p) - 1
    with Engine(p, 6, plan=spec) as e:
        for entry in ENTRIES:
            for a in (3, 2**24 + 1, 2**32 - 1):
                x, y, z = rng.randrange(Mp), rng.randrange(Mp), rng.randrange(Mp)
                want, copy_want = _factor_case(e, entry, a, x, y, z)
                _assert_value(e, 0, want, (shape, entry, a))
                if copy_want is not None:
                    _assert_value(e, 3, copy_want, (shape, entry, a, "copy"))


def test_mul_add_onto_itself_above_the_fused_bound():
    """mul_add(dst, y, dst, a): exact up to the fused bound; above it the call is refused, never computed wrongly"""
    p, spec, _ = SHAPES["radix8-cols"]
    rng = random.Random(3)
    Mp = (1 << p) - 1
    with Engine(p, 4, plan=spec) as e:
        x, y = rng.randrange(Mp), rng.randrange(Mp)
        e.set_int(1, y); e.set_multiplicand(2, 1)
        e.set_int(0, x); e.mul_add(0, 2, 0, 255)
        _assert_value(e, 0, x * y * 255 + x, "a = 255")
        e.set_int(0, x)
        with pytest.raises(Exception):
            e.mul_add(0, 2, 0, 2**32 - 1)


# ---- subtraction matrix on the small shapes -----------------------------------------------------------------------------------------

def _sub_follow(e, form, y):
    """the operation after the subtraction on register 0 (y: a dense value); returns f(value) for the expected result"""
    p = e.p
    if form == "square_mul":
        e.square_mul(0); return 0, lambda v: v * v
    if form == "square_mul_n":
        e.square_mul_n(0, 2, 1, 2)
        return 0, lambda v: _red(_red(v * v - 2, p) ** 2 - 2, p)
    if form == "mul_dst":
        e.set_int(5, y); e.set_multiplicand(2, 5); e.mul(0, 2); return 0, lambda v: v * y
    if form == "mul_src":
        e.set_multiplicand(2, 0); e.set_int(1, y); e.mul(1, 2); return 1, lambda v: v * y
    if form == "copy_square":
        e.copy(1, 0); e.square_mul(1); return 1, lambda v: v * v
    e.set_int(1, y); e.add(1, 0); e.square_mul(1); return 1, lambda v: (v + y) ** 2


@pytest.mark.parametrize("form", FOLLOW)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_subtraction_matrix_small_shapes(shape, form):
    p, spec, _ = SHAPES[shape]
    Mp = (1 << p) - 1
    rng = random.Random(zlib.crc32(("%s:%s" % (shape, form)).encode()))
    half = (p + 1) // 2   # 2^(2 j) = 2^k (mod Mp) for j = k (p + 1) / 2 mod p
    ks = _sparse_positions(p, spec)
    with Engine(p, 6, plan=spec) as e:
        cases = [(0, v) for v in SUBS] + [(1, v) for v in SUBS] + [(1 << k, v) for k in ks for v in SUBS] + [((1 << k) + 1, 2) for k in ks]
        for pending in (False, True):
            for x, v in cases:
                if pending:   # x as the result of a squaring: its run carries are pending when the subtraction comes
                    if x in (0, 1):
                        root = x
                    elif x & (x - 1) == 0:
                        root = 1 << (x.bit_length() - 1) * half % p
                    else:
                        continue
                    e.set_int(0, root); e.square_mul(0)
                else:
                    e.set_int(0, x)
                e.sub(0, v)
                y = rng.randrange(Mp)
                reg, f = _sub_follow(e, form, y)
                _assert_value(e, reg, f(_red(x - v, p)), (shape, form, pending, x.bit_length(), v))
        # several subtractions accumulating before one squaring
        for x in [0, 1] + [1 << k for k in ks]:
            for vs in ([1, 2, 3], [2**30 - 1, 2**30 - 1, 1], [2**32 - 1, 2**32 - 1]):
                e.set_int(0, x)
                for v in vs:
                    e.sub(0, v)
                e.square_mul(0)
                _assert_value(e, 0, _red(x - sum(vs), p) ** 2, (shape, form, "accumulated", x.bit_length(), vs))


# ---- all-zero and unit registers ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", list(SHAPES))
def test_zero_and_one_through_every_product(shape):
    """An all-zero register (and the value 1) through square_mul, mul and square_mul_n.  With zeros everywhere every negated shift of the
    butterflies returns P on the device ("a negated zero is left as P", gf.hpp), so this is the end-to-end companion of the self-test's
    operands equal to P: the result must be exactly 0 (resp. the closed form).
    (test_gpu_parity.test_edge_values squares a zero register at p = 1279 only, a shape that none of SHAPES' kernel sets serves.)"""
    p, spec, _ = SHAPES[shape]
    Mp = (1 << p) - 1
    rng = random.Random(zlib.crc32(shape.encode()))
    y = rng.randrange(Mp)
    with Engine(p, 6, plan=spec) as e:
        e.set_int(5, y); e.set_multiplicand(2, 5)
        e.set(4, 0); e.set_multiplicand(3, 4)                 # a zero multiplicand image
        for a in (1, 3, 2**32 - 1):
            e.set(0, 0); e.square_mul(0, a)
            assert e.get_int(0) == 0, (shape, "0^2", a)
            e.square_mul(0, a)                                  # the result of a zero squaring as the next operand
            assert e.get_int(0) == 0, (shape, "0^2 twice", a)
            e.set(0, 0); e.mul(0, 2, a)
            assert e.get_int(0) == 0, (shape, "0 * y", a)
            e.set_int(0, y); e.mul(0, 3, a)
            assert e.get_int(0) == 0, (shape, "y * 0", a)
            e.set(0, 0); e.square_mul_n(0, 3, a, 0)
            assert e.get_int(0) == 0, (shape, "square_mul_n on 0", a)
            e.set(0, 0); e.square_mul_n(0, 2, a, 2)             # 0 -> -2 -> 4 a - 2
            _assert_value(e, 0, 4 * a - 2, (shape, "LL steps from 0", a))
            e.set(0, 1); e.square_mul(0, a)
            _assert_value(e, 0, a, (shape, "1^2", a))
            e.set(0, 1); e.mul(0, 2, a)
            _assert_value(e, 0, y * a, (shape, "1 * y", a))
            e.set(0, 1); e.square_mul_n(0, 3, a, 0)
            _assert_value(e, 0, a ** 7, (shape, "square_mul_n on 1", a))
        e.set(0, 0); e.square_mul(0); e.set(1, 0)
        assert e.is_equal(0, 1)


# ---- full size: the largest exponent of each transform size -----------------------------------------------------------------------

def _p_max(n):
    """largest exponent the size rule maps to n (pinned by the CPU test of plan.hpp transform_size)"""
    lo, hi = 3, (1 << 32) - 1
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if orc.lib().orc_transform_size(mid) <= n:
            lo = mid
        else:
            hi = mid - 1
    return lo


FULL = [  # n -> plan text at p_max(n) (the register-resident shapes), plus one split5 size
    (2**18, None, "n=262144:m1=128:m2=1024:c=4"), (2**19, None, "n=524288:m1=256:m2=1024:c=4"),
    (5 * 2**19, None, "n=2621440:m1=1280:m2=1024:c=4"), (2**20, None, "n=1048576:m1=256:m2=2048:c=4"),
    (2**21, None, "n=2097152:m1=512:m2=2048:c=8"), (5 * 2**20, None, "n=5242880:m1=1280:m2=2048:c=4"),
    (2**22, None, "n=4194304:m1=512:m2=4096:c=8"), (2**23, None, "n=8388608:m1=1024:m2=4096:c=4"),
    (5 * 2**21, None, "n=10485760:m1=1280:m2=4096:c=4"), (2**24, None, "n=16777216:m1=2048:m2=4096:c=2"),
    (5 * 2**22, None, "n=20971520:m1=2560:m2=4096:c=2"), (2**25, None, "n=33554432:m1=2048:m2=8192:c=2"),
    (5 * 2**23, None, "n=41943040:m1=2560:m2=8192:c=2"), (5 * 2**19, "split5", "n=2621440:m1=1280:m2=1024:c=1:split5"),
]


def _minus_one_words(e):
    w = np.full(e.word_count, 0xFFFFFFFF, dtype=np.uint32)
    w[0] = 0xFFFFFFFE
    if e.p % 32:
        w[-1] = (1 << (e.p % 32)) - 1
    return w


def _check_all_max_digits(e):
    """x = Mp - 1 (every digit but the first at its maximum): (-1)^2 a = a, then (a^2)^2 after two plain squarings"""
    m1 = _minus_one_words(e)
    for a in (1, 3, 2**24 + 1, 2**32 - 1):
        e.set_words(0, m1); e.square_mul(0, a)
        e.set(1, a)
        assert e.is_equal(0, 1), (e.p, a)
    e.square_mul(0); e.square_mul(0)
    assert e.get_int(0) == (2**32 - 1) ** 4, (e.p, "follow")


@pytest.mark.xfail(strict=True, reason="the reference's size rule takes log2 5 as 2.4 and admits exponents at the top of the 5 2^k "
                   "ranges where the convolution sums of the all-maximum input pass the field prime (the oracle gives the same wrong value)")
@pytest.mark.parametrize("n", [5 * 2**19, 5 * 2**21, 40, 160, 640, 2560, 10240, 40960])   # (the small ones: the exact coefficients are
def test_all_max_digits_at_the_top_of_the_five_ranges(n, oracle_lib):                     # 1.20-1.25 P, test_factor_bound_cases.py)
    with Engine(_p_max(n), 4) as e:
        _check_all_max_digits(e)


@pytest.mark.parametrize("n,spec,text", FULL, ids=["%d%s" % (n, "-" + s if s else "") for n, s, _ in FULL])
def test_full_size_at_the_top_of_each_range(n, spec, text, oracle_lib):
    p = _p_max(n)
    assert resolve_plan(p, spec) == "marin-hip:" + text
    with Engine(p, 4, plan=spec) as e:
        assert e.n == n and e.describe() == "marin-hip:" + text
        if n & (n - 1) == 0:
            _check_all_max_digits(e)
        # (5 2^k sizes: the all-maximum input overflows at the top of their ranges, test_all_max_digits_at_the_top_of_the_five_ranges)
        # sparse: (2^k - 1)^2 a and (2^k + 1)^2 a by shifts
        for k, s, a in ((p // 2 + 1, -1, 2**32 - 1), (p - 3, 1, 2**28 + 1)):
            e.set_int(0, (1 << k) + s); e.square_mul(0, a)
            assert e.get_int(0) == _red(((1 << (2 * k)) + s * (1 << (k + 1)) + 1) * a, p), (p, k, s, a)
        # random x: square_mul(x, a) == square_mul(x, 1) * (image of the constant a)
        rng = np.random.default_rng(p)
        w = rng.integers(0, 2**32, e.word_count, dtype=np.uint64).astype(np.uint32)
        if p % 32:
            w[-1] &= (1 << (p % 32)) - 1
        for a in (2**24 + 1, 2**32 - 1):
            e.set_words(0, w); e.set_words(1, w)
            e.square_mul(0, a); e.square_mul(1, 1)
            e.set(2, a); e.set_multiplicand(3, 2); e.mul(1, 3)
            assert e.is_equal(0, 1) and np.array_equal(e.words(0), e.words(1)), (p, a)


# ---- the second field family ------------------------------------------------------------------------------------------------------

CRT_SMALL = [(9941, 1), (9941, 3), (9941, 9), (44497, 9)]


@pytest.mark.parametrize("p,odd", CRT_SMALL)
def test_crt_factor_and_subtraction_matrix(p, odd):
    Mp = (1 << p) - 1
    rng = random.Random(p * 10 + odd)
    with CrtEngine(p, odd, reg_count=6) as e:
        for entry in ENTRIES:
            for a in FACTORS:
                x, y, z = rng.randrange(Mp), rng.randrange(Mp), rng.randrange(Mp)
                want, copy_want = _factor_case(e, entry, a, x, y, z)
                _assert_value(e, 0, want, ("crt", odd, entry, a))
                if copy_want is not None:
                    _assert_value(e, 3, copy_want, ("crt", odd, entry, a, "copy"))
        for form in FOLLOW:
            for x in (0, 1, 1 << 40, 1 << (p - 1), (1 << (p // 2)) + 1):
                for v in SUBS:
                    e.set_int(0, x); e.sub(0, v)
                    y = rng.randrange(Mp)
                    reg, f = _sub_follow(e, form, y)
                    _assert_value(e, reg, f(_red(x - v, p)), ("crt", odd, form, x.bit_length(), v))


@pytest.mark.parametrize("odd", [9, 3])
def test_crt_c4_sizes_closed_forms(odd):
    p = 205271257
    with CrtEngine(p, odd, reg_count=4) as e:
        m1 = _minus_one_words(e)
        for a in (3, 2**24 + 1, 2**32 - 1):
            e.set_words(0, m1); e.square_mul(0, a)
            e.set(1, a)
            assert e.is_equal(0, 1), (odd, a)
        k = p - 3
        for v in (2, 2**32 - 1):
            e.set_int(0, 1 << k); e.sub(0, v); e.square_mul(0, 2**32 - 1)
            assert e.get_int(0) == _red(((1 << (2 * k)) - 2 * v * (1 << k) + v * v) * (2**32 - 1), p), (odd, v)
