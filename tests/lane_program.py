"""The register-machine program of the lane tests and its model on Python integers mod 2^p - 1, shared by test_gpu_lanes.py,
test_gpu_lanes_wide.py and test_gpu_coresident.py.  No GPU is needed to import this."""
import ctypes
import random

import orc
from prmers_amd import pm1

MAX_LANES = 5                  # what inputs(p) gives without a lane count (tests/test_gpu_lanes.py)
REGS = 10
OUT_REGS = (0, 4, 5, 6, 7)


# ---- integers mod 2^p - 1 (products through libgmp where it loads: Python's own take seconds each at 10^7 bits) ----

def have_gmp():
    return pm1.load_gmp() is not None


def _bigmul(a, b):
    G = pm1.load_gmp()
    if G is None or max(a.bit_length(), b.bit_length()) < 100000:
        return a * b
    P = ctypes.POINTER(G.Mpz)
    G.__gmpz_mul.argtypes = [P, P, P]
    za, zb = G.Mpz(), G.Mpz()
    for z in (za, zb):
        G.__gmpz_init(ctypes.byref(z))
    try:
        for z, v in ((za, a), (zb, b)):
            raw = v.to_bytes((v.bit_length() + 7) // 8 or 1, "little")
            G.__gmpz_import(ctypes.byref(z), len(raw), -1, 1, -1, 0, raw)
        G.__gmpz_mul(ctypes.byref(za), ctypes.byref(za), ctypes.byref(zb))
        size = (G.__gmpz_sizeinbase(ctypes.byref(za), 2) + 7) // 8
        buf = ctypes.create_string_buffer(size or 1)
        count = ctypes.c_size_t(0)
        G.__gmpz_export(buf, ctypes.byref(count), -1, 1, -1, 0, ctypes.byref(za))
        return int.from_bytes(buf.raw[:count.value], "little")
    finally:
        for z in (za, zb):
            G.__gmpz_clear(ctypes.byref(z))


def mulmod(p, a, b, f=1):
    """a b f mod 2^p - 1"""
    return orc.mers_reduce(_bigmul(a, b) * f, p)


def powmod(p, a, h):
    """a^h mod 2^p - 1, left to right over the bits of h"""
    r = 1
    for i in range(int(h).bit_length() - 1, -1, -1):
        r = mulmod(p, r, r)
        if (h >> i) & 1:
            r = mulmod(p, r, a)
    return r


def inputs(p, seed=0, lanes=None):
    """(x, y, z) per lane: seeded full-size operands; lane 0 has x = 2^p - 2, lane 1 has x = 0.  Without a lane count: MAX_LANES lanes.
    With one: that many, the first ones the same values (the generator is drawn lane by lane), and from three lanes on the last lane has
    x = 2^p - 2 as well."""
    rng = random.Random(1000 * p + seed)
    mp = (1 << p) - 1
    out = [[rng.getrandbits(p) % mp for _ in range(3)] for _ in range(MAX_LANES if lanes is None else lanes)]
    out[0][0] = mp - 1
    if len(out) > 1:
        out[1][0] = 0
    if lanes is not None and lanes >= 3:
        out[-1][0] = mp - 1
    return out


def model(p, x, y, z):
    """the program of run_program on integers -> the values of registers 0, 4, 5, 6, 7"""
    mp = (1 << p) - 1

    def mul(a, b, f=1):
        return orc.mers_reduce(_bigmul(a, b) * f, p)
    r0 = mul(x, x)
    r0 = mul(r0, r0, 3)                    # 1  square_mul, factors 1 and 3
    r0 = (r0 - 5) % mp                     # 2  sub
    r0 = mul(r0, y)                        # 3, 4  set_multiplicand, mul
    r0 = (r0 + z) % mp                     # 5  add
    r0 = (r0 - y) % mp                     # 6  sub_reg
    r4, r5 = (r0 + z) % mp, (r0 - z) % mp  # 7  addsub
    r4 = (mul(r4, y) + r5) % mp            # 8  mul_add
    r4 = mul(r4, r4, 2); r6 = r4           # 9  square_mul_copy
    r6 = mul(r6, y); r7 = r6               # 10 mul_copy
    r7 = mul(r7, (y + z) % mp)             # 11 mul_sum
    old5 = r5
    r5 = mul(r5, r5); r7 = mul(r7, old5)   # 12 square_mul_prepare, then a mul by its image
    for _ in range(5):
        r7 = (mul(r7, r7) - 2) % mp        # 13 square_mul_n(..., 5, sub=2)
    return {0: r0, 4: r4, 5: r5, 6: r6, 7: r7}


def run_program(e, lane_inputs):
    """every operation runs while the last result's run carries are still pending: nothing is read in between"""
    for r in (0, 1, 2):
        e.set(r, 0)
        for l, v in enumerate(lane_inputs):
            e.set_int(r, v[r], lane=l)
    e.square_mul(0, 1); e.square_mul(0, 3)
    e.sub(0, 5)
    e.set_multiplicand(3, 1)
    e.mul(0, 3)
    e.add(0, 2)
    e.sub_reg(0, 1)
    e.addsub(4, 5, 0, 2)
    e.mul_add(4, 3, 5)
    e.square_mul_copy(4, 6, 2)
    e.mul_copy(6, 3, 7)
    e.set_multiplicand(8, 2)
    e.mul_sum(7, 3, 8, 9)
    e.square_mul_prepare(5, 9)
    e.mul(7, 9)
    e.square_mul_n(7, 5, 1, 2)


_expected = {}


def expected(p, lanes=MAX_LANES, lane_inputs=None):
    """the model's registers for the first `lanes` lanes of inputs(p): each lane computed once and shared by the tests that need it"""
    if lane_inputs is not None:
        return [model(p, *v) for v in lane_inputs]
    return expected_of(p, inputs(p)[:lanes])


def expected_of(p, lane_inputs):
    """the model's registers for these operands, one entry per lane; cached by the operands, so the lane counts of one shape share
    every lane whose values they share"""
    out = []
    for v in lane_inputs:
        key = (p, tuple(v))
        if key not in _expected:
            _expected[key] = model(p, *v)
        out.append(_expected[key])
    return out
