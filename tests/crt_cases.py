"""The sizes at which the second field family (GF(M61^2) x GF(M31^2): prmers_amd/csrc/crt_engine.hip, crt_kernels.hip) is tested for products,
worst-case digits and kernel switches -- one list for the CPU guard (test_crt_cases.py), the pin generator
(golden/make_crt_product_pins.py) and the GPU tests (test_gpu_crt_products.py, test_gpu_crt_switches.py) -- with the Python restatement
of the engine's kernel choice, the seeded operands, the expected values and the scripts the GPU tests run.

A case is (odd, ln): n = odd << ln words, m = 2^ln, h = m / 2 slots per odd residue class, rows of H2 = 1024, columns of H1 = h / 1024.
Each case has two exponents: p_top, the largest odd p the size admits (log2 n + 2 (p / n + 1) < 92), and p_low, the smallest odd p with
at least 15 bits per word (the run-wise carry needs q (kRun - 1) >= 100)."""
import functools
import hashlib
import json
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PIN_PATH = os.path.join(HERE, "golden", "crt_product_pins.json")

M61, M31 = (1 << 61) - 1, (1 << 31) - 1
LIMIT_BITS = math.log2(M61 * M31)      # 92.0000: what an unweighted convolution coefficient must stay under
K_RUN = 8                              # crt_field.hpp kRun: digits per thread of the carry sweep
A = 2**32 - 1                          # the factor of the product script
FACTORS = (1, 3, 2**24 + 1, 2**32 - 1)
PIN_THRESHOLD = 2500000                # exponents above it are checked against the libgmp pins, the others against Python integers

# odd = 1: every H1 from 2 to 2048; odd = 3: both classes of m mod 3 and the radix-3 size of BASELINE configs[3] (H1 = 1024: split
# columns by default); odd = 9: all six classes of 2^ln mod 9 and the radix-9 size of configs[3] (H1 = 512)
CASES = [(1, ln) for ln in range(12, 23)] + [(3, 12), (3, 13), (3, 21)] + [(9, ln) for ln in range(12, 18)] + [(9, 20)]
LOW_MAX_LN = 20                        # p_low runs where n <= 2^20 odd
SWITCH_CASES = [(1, ln) for ln in range(12, 23)] + [(3, 13), (9, 14), (3, 21), (9, 20)]
KERNEL_SETS = [None, "generic", "joint", "split"]      # MI355_CRT_KERNELS
TUNES = [0, 1, 2, 3]                                   # MI355_CRT_TUNE: bit 0 plain tile order in the column kernels, bit 1 back and carry as two kernels


def case_id(case):
    return "%dx2^%d" % case


def max_exponent(n):
    """the largest p with log2(n) + 2 (p / n + 1) < 92 (the size rule of crt_transform_size, in the same double arithmetic)"""
    lo, hi = n, 60 * n
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if math.log2(n) + 2.0 * (mid / n + 1.0) < 92.0:
            lo = mid
        else:
            hi = mid - 1
    return lo


def p_top(odd, ln):
    p = max_exponent(odd << ln)
    return p if p % 2 else p - 1


def p_low(odd, ln):
    p = 15 * (odd << ln)
    return p if p % 2 else p + 1


def exponent(odd, ln, which):
    return p_top(odd, ln) if which == "top" else p_low(odd, ln)


def constructor_accepts(p, n):
    """the two checks of CrtEngine::CrtEngine on a forced size: the size rule and the bits per word the run-wise carry needs"""
    return math.log2(n) + 2.0 * (p / n + 1.0) < 92.0 and (p // n) * (K_RUN - 1) >= 100


def runs(which=("top", "low")):
    """(odd, ln, which) of every engine the product test creates"""
    return [(odd, ln, w) for odd, ln in CASES for w in which if w == "top" or ln <= LOW_MAX_LN]


# ---- the kernel choice ----------------------------------------------------------------------------------------------------------------

K_SLOTS31 = 8192      # crt_kernels.hip kSlots31: slots per work-group of the one-field column kernel of GF(M31^2)


def grid_of(ln):
    """(logH1, logH2) as the constructor splits h = 2^(ln - 1) without a plan text"""
    logh = ln - 1
    logH2 = min(10, logh)
    return logh - logH2, logH2


def choose_kernels(odd, logH1, logH2, kernel_set, tune):
    """crt::choose_kernels (prmers_amd/csrc/crt_kernels.hip) restated: (radix8, cols_split, back_fused) from the grid, MI355_CRT_KERNELS
    and MI355_CRT_TUNE.  `split` below H1 = 8 falls back to the joint column kernel without a word: a work-group of the one-field
    kernel would hold more than the H2 columns of a row there."""
    radix8 = logH2 == 10 and 1 <= logH1 <= 11 and kernel_set != "generic"
    groups = K_SLOTS31 >> logH1
    cols_split = radix8 and kernel_set != "joint" and (logH1 >= 10 or kernel_set == "split") and 1 <= groups <= (1 << logH2)
    h = 1 << (logH1 + logH2)
    back_fused = odd > 1 and h % 256 == 0 and not tune & 2
    return radix8, cols_split, back_fused


def kernels_of_case(odd, ln, kernel_set=None, tune=0):
    return choose_kernels(odd, *grid_of(ln), kernel_set, tune)


def algorithmic_bytes(n, back_fused):
    """CrtEngine::algorithmic_bytes: digits r + w, four row passes r + w of 12 bytes, and the carry sweep's input w + r in the two-kernel form"""
    return n * (8 + 8 + 96 + (0 if back_fused else 24))


# ---- digits and the worst-case input ------------------------------------------------------------------------------------------------

def widths(p, n):
    j = np.arange(n + 1, dtype=np.uint64)
    c = (j * np.uint64(p) + np.uint64(n - 1)) // np.uint64(n)
    return (c[1:] - c[:-1]).astype(np.int64)


def worst_coefficient_bits(p, n):
    """log2 of the largest unweighted convolution coefficient of (Mp - 1)^2 -- every digit at its maximum but the first, one below -- by
    a float FFT: digit j carries the weight 2^(ceil(p j / n) - p j / n), the cyclic convolution of the weighted digits divided by the
    weight of its place is the integer the engine's Garner step has to reconstruct below M61 M31"""
    w = widths(p, n)
    x = np.exp2(w.astype(np.float64)) - 1.0
    x[0] -= 1.0
    j = np.arange(n, dtype=np.uint64)
    frac = (-(j * np.uint64(p) % np.uint64(n)).astype(np.int64)) % n       # n (ceil(p j / n) - p j / n)
    a = np.exp2(frac.astype(np.float64) / n)
    f = np.fft.rfft(a * x)
    c = np.fft.irfft(f * f, n) / a
    return float(np.log2(c.max()))


# ---- seeded operands ------------------------------------------------------------------------------------------------------------------

def seed_of(odd, ln):
    return 1000 * odd + ln


def word_count(p):
    return (p + 31) // 32


def operand_bytes(seed, p):
    """x and y: the low p bits of two draws of (p + 7) // 8 bytes, little-endian, padded to whole 32-bit words; all ones map to 0"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        b = bytearray(rng.bytes((p + 7) // 8))
        if p % 8:
            b[-1] &= (1 << (p % 8)) - 1
        if bytes(b) == b"\xff" * (len(b) - 1) + bytes([(1 << (p % 8 or 8)) - 1]):
            b = bytearray(len(b))
        out.append(bytes(b) + bytes(4 * word_count(p) - len(b)))
    return out


@functools.lru_cache(maxsize=2)
def operands(odd, ln, which):
    """(x words, y words) of a run as uint32 arrays"""
    p = exponent(odd, ln, which)
    return tuple(np.frombuffer(b, dtype="<u4").astype(np.uint32) for b in operand_bytes(seed_of(odd, ln), p))


def red(v, p):
    """v mod 2^p - 1 by folding (v >= -(2^p - 1))"""
    M = (1 << p) - 1
    if v < 0:
        v += M
    while v > M:
        v = (v & M) + (v >> p)
    return 0 if v == M else v


def int_of(words):
    return int.from_bytes(np.ascontiguousarray(words, dtype="<u4").tobytes(), "little")


def words_of_int(v, p):
    return np.frombuffer(v.to_bytes(4 * word_count(p), "little"), dtype="<u4").astype(np.uint32)


def stamp(word_bytes):
    """what a pin holds of a value: res64 and the SHA-256 of its canonical little-endian 32-bit words"""
    return {"res64": "%016X" % int.from_bytes(word_bytes[:8], "little"), "sha256_words": hashlib.sha256(word_bytes).hexdigest()}


STEPS = ("v1", "v2", "xy", "v3")      # v1 = x^2 A, v2 = v1 y A, xy = x y, v3 = (v2 - 2)^2 y, all mod 2^p - 1


def pin_key(odd, ln, which):
    return "%d,%d,%s" % (odd, ln, which)


def pinned_runs():
    return [r for r in runs() if exponent(*r) > PIN_THRESHOLD]


@functools.lru_cache(maxsize=1)
def pins():
    with open(PIN_PATH) as f:
        return json.load(f)["pins"]


@functools.lru_cache(maxsize=None)
def expected(odd, ln, which):
    """{step: {"res64", "sha256_words"}} of the product script: the libgmp pins above the threshold, Python integers below it"""
    p = exponent(odd, ln, which)
    if p > PIN_THRESHOLD:
        pin = pins()[pin_key(odd, ln, which)]
        assert (pin["p"], pin["seed"]) == (p, seed_of(odd, ln))
        return {s: pin[s] for s in STEPS}
    x, y = (int_of(w) for w in operands(odd, ln, which))
    v1 = red(red(x * x, p) * A, p)
    v2 = red(red(v1 * y, p) * A, p)
    v3 = red(red(red(v2 - 2, p) ** 2, p) * y, p)
    values = {"v1": v1, "v2": v2, "xy": red(x * y, p), "v3": v3}
    return {s: stamp(v.to_bytes(4 * word_count(p), "little")) for s, v in values.items()}


# ---- what the GPU tests run -------------------------------------------------------------------------------------------------------------

def assert_engine(e, odd, ln, kernel_set=None, tune=0):
    """the engine is the one the case means: forced size, column length and kernel set in its plan text, the traffic model of its form"""
    n = odd << ln
    radix8, _, back_fused = kernels_of_case(odd, ln, kernel_set, tune)
    text = e.describe()
    assert e.n == n and ":h1=%d:" % (1 << grid_of(ln)[0]) in text and text.endswith("radix8" if radix8 else "generic"), text
    assert e.algorithmic_bytes() == algorithmic_bytes(n, back_fused), (text, tune)


def assert_step(e, reg, want, what):
    w = e.words(reg)
    got = stamp(w.astype("<u4").tobytes())
    assert e.res64(reg) == int(want["res64"], 16), what
    assert got == want, what


def product_script(e, odd, ln, which, with_copied_image=True, label=""):
    """x in register 0, y in register 1 and its image in register 2; then
       v1: square_mul(0, A);  v2: mul(0, 2, A) on the weak carries of a factor-A squaring;
       xy: a copy of y made into an image in place, times x set by words (registers 3 and 4; left out by the switch test);
       v3: sub(0, 2), square_mul(0), mul(0, 2) -- image 2 has by then survived every other transform through the shared work arrays.
    Every step against the pins or the integers of `expected`."""
    x, y = operands(odd, ln, which)
    want = expected(odd, ln, which)
    what = (odd, ln, which, label)
    e.set_words(0, x); e.set_words(1, y); e.set_multiplicand(2, 1)
    e.square_mul(0, A)
    assert_step(e, 0, want["v1"], what + ("v1",))
    e.mul(0, 2, A)
    assert_step(e, 0, want["v2"], what + ("v2",))
    if with_copied_image:
        e.copy(3, 1); e.set_multiplicand(3, 3); e.set_words(4, x); e.mul(4, 3)
        assert_step(e, 4, want["xy"], what + ("xy",))
    e.sub(0, 2); e.square_mul(0); e.mul(0, 2)
    assert_step(e, 0, want["v3"], what + ("v3",))


def assert_words(e, reg, want, what):
    assert np.array_equal(e.words(reg), want), what


def small_words(a, p):
    w = np.zeros(word_count(p), dtype=np.uint32)
    w[0] = a
    return w


def worst_case_script(e, odd, ln, which, m1):
    """m1 = the words of Mp - 1 (every digit but the first at its maximum) through every kind of product; registers 1 and 2 hold y and
    its image (left by product_script), 3 and 4 are free.  Every expected value is a closed form or a small multiple of y folded mod 2^p - 1."""
    p = e.p
    Mp = (1 << p) - 1
    yw = operands(odd, ln, which)[1]
    y = int_of(yw)
    for a in FACTORS:                                        # (-1)^2 a = a
        e.set_words(0, m1); e.square_mul(0, a)
        assert_words(e, 0, small_words(a, p), (p, "square_mul", a))
    e.set_words(3, m1); e.set_multiplicand(3, 3)             # the image of -1
    for a in FACTORS:
        e.set_words(0, m1); e.mul(0, 3, a)                   # (-1)(-1) a = a
        assert_words(e, 0, small_words(a, p), (p, "mul by the worst-case image", a))
        e.set_words(4, yw); e.mul(4, 3, a)                   # y (-1) a
        assert_words(e, 4, words_of_int(red(a * (Mp - y), p), p), (p, "y times the worst-case image", a))
    e.set_words(0, m1); e.mul(0, 2)                          # (-1) y
    assert_words(e, 0, words_of_int(red(Mp - y, p), p), (p, "worst case times the image of y"))
    e.set_words(0, m1); e.sub(0, 1); e.square_mul(0)         # (-2)^2
    assert_words(e, 0, small_words(4, p), (p, "(Mp - 2)^2"))
    e.set_words(0, m1); e.square_mul_n(0, 3, 1, 2)           # -1 -> 1 - 2 = -1, three times: a subtraction after every worst-case squaring
    assert_words(e, 0, m1, (p, "square_mul_n"))
