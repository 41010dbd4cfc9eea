"""First HIP kernel of the second field family: the fused unweight + Garner + carry sweep over GF(M61^2) x GF(M31^2)
(prmers_amd/csrc/crt_kernels.hip, crt_carry.hpp; reference third_party/aevum/src/cl/carry.cl:506-588) through the C ABI, against the CRT oracle
(oracle/oracle_crt.c).  Needs a real MI355X:  python -m pytest tests -m gpu"""
import ctypes as C

import numpy as np
import pytest

import orc_crt

pytestmark = pytest.mark.gpu


def crt_carry(p, n, odd, a, r61, r31, timed=False):
    from prmers_amd.engine import load_library, EngineError
    L = load_library()
    digits = np.zeros(n, dtype=np.uint64)
    residual = np.zeros((n + 7) // 8, dtype=np.uint64)
    ms = C.c_double(0)
    ok = L.mi355_crt_carry(p, n, odd, a, r61.ctypes.data_as(C.c_void_p), r31.ctypes.data_as(C.c_void_p), digits.ctypes.data_as(C.c_void_p),
                           residual.ctypes.data_as(C.c_void_p), 0, C.byref(ms) if timed else None)
    if not ok:
        raise EngineError(L.mi355_engine_last_error().decode())
    return digits, residual, ms.value


def finish(digits, residual, widths):
    """the last carries (a unit here and there) in front of the following run, then the strong carry with wrap-around"""
    d = digits.astype(object)
    n = len(d)
    for run, c in enumerate(residual):
        if c:
            d[((run + 1) * 8) % n] += int(c)
    while True:
        over = [j for j in range(n) if d[j] >> int(widths[j])]
        if not over:
            return np.array(d, dtype=np.uint64)
        for j in over:
            c = d[j] >> int(widths[j])
            d[j] &= (1 << int(widths[j])) - 1
            d[(j + 1) % n] += c


@pytest.mark.parametrize("p,odd,a", [(521, 1, 1), (1279, 3, 1), (9941, 9, 3), (11213, 9, 1), (86243, 9, 1), (216091, 3, 3), (1257787, 9, 1), (3021377, 1, 1)])
def test_crt_carry_matches_the_oracle(p, odd, a):
    o = orc_crt.OracleCrt(p, odd)
    rng = np.random.default_rng(p)
    w = o.widths().astype(np.uint64)
    o.set_digits(rng.integers(0, 1 << 62, o.n, dtype=np.uint64) & ((np.uint64(1) << w) - np.uint64(1)))
    for _ in range(2):
        o.square_mul(a)
        r61, r31 = o.weighted()
        digits, residual, _ = crt_carry(p, o.n, odd, a, r61, r31)
        assert int(residual.max()) <= 8
        assert np.array_equal(finish(digits, residual, w), o.digits()), (p, odd)


def test_crt_carry_at_the_radix_9_size_of_config_4_and_its_rate():
    """p = 205271257 at 9*2^20 words (BASELINE configs[3]): parity with the oracle and the sweep's duration"""
    p, odd, n = 205271257, 9, 9 << 20
    o = orc_crt.OracleCrt(p, odd, n)
    rng = np.random.default_rng(p)
    w = o.widths().astype(np.uint64)
    o.set_digits(rng.integers(0, 1 << 62, o.n, dtype=np.uint64) & ((np.uint64(1) << w) - np.uint64(1)))
    o.square_mul(1)
    r61, r31 = o.weighted()
    digits, residual, ms = crt_carry(p, n, odd, 1, r61, r31, timed=True)
    want = o.digits()
    # vectorised finish: residual carries, then carry passes until nothing is left
    d = digits.copy()
    idx = ((np.nonzero(residual)[0] + 1) * 8) % n
    np.add.at(d, idx, residual[np.nonzero(residual)[0]])
    for _ in range(64):
        c = d >> w
        if not c.any():
            break
        d = (d & ((np.uint64(1) << w) - np.uint64(1))) + np.roll(c, 1)
    assert np.array_equal(d, want)
    print("crt carry sweep: %.3f ms for %d words (%.0f GB/s of 20 B/word)" % (ms, n, 20 * n / ms / 1e6))
    assert ms < 1.0


# ---- the sweep against Python integers at the extremes of its operands ------------------------------------------------------------------

M61, M31 = (1 << 61) - 1, (1 << 31) - 1
VMAX = M61 * M31 - 1   # the largest coefficient the two residues can name


def _geometry(p, n):
    """bit position and width of every digit, and the exponents that take a coefficient back to the weighted residues the sweep expects:
    digit j carries the weight 2^(e / n), e = (n - p j mod n) mod n, and 2^(1 / n) = 2^l with l n = 1 (mod 61 resp. 31)"""
    pos = [-(-p * j // n) for j in range(n + 1)]
    widths = [pos[j + 1] - pos[j] for j in range(n)]
    l61, l31 = pow(n, -1, 61), pow(n, -1, 31)
    e = [(n - p * j % n) % n for j in range(n)]
    return pos, widths, [l61 * ej % 61 for ej in e], [l31 * ej % 31 for ej in e]


def _garner(x61, x31):
    return x31 + M31 * ((x61 - x31) * pow(M31, -1, M61) % M61)


def _widest_p(n):
    """the largest exponent CrtEngine's constructor admits at n words: log2 n + 2 (p / n + 1) < 92"""
    import math
    p = int(n * (45 - math.log2(n) / 2)) + 1
    while math.log2(n) + 2.0 * (p / n + 1.0) >= 92.0:
        p -= 1
    return p


# (n, odd): the narrowest words the constructor admits (15 bits: 7 words must hold a coefficient) and the widest (_widest_p)
EXTREME_SIZES = [(64, 1), (1024, 1), (96, 3), (768, 3), (72, 9), (4608, 9)]
PATTERNS = ["max", "zero", "x61_lt_x31", "x61_eq_x31", "x61_top_x31_zero", "x61_zero_x31_top", "max_at_run_edges", "max_at_last_digit"]


def _pattern(name, n, rng):
    if name == "max":
        return [VMAX] * n
    if name == "zero":
        return [0] * n
    if name == "x61_lt_x31":
        return [_garner(j % 1000, M31 - 1 - j) for j in range(n)]
    if name == "x61_eq_x31":
        return [_garner(x, x) for x in (j * 2654435761 % M31 for j in range(n))]
    if name == "x61_top_x31_zero":
        return [_garner(M61 - 1, 0)] * n
    if name == "x61_zero_x31_top":
        return [_garner(0, M31 - 1)] * n
    if name == "max_at_run_edges":   # the first and the last digit of every run of 8 (the last digit of all: the carry wraps around)
        return [VMAX if j % 8 in (0, 7) else rng.randrange(1 << 20) for j in range(n)]
    return [0] * (n - 1) + [VMAX]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("width", ["narrow", "wide"])
@pytest.mark.parametrize("n,odd", EXTREME_SIZES)
def test_crt_carry_extreme_coefficients_against_integers(n, odd, width, pattern):
    """mi355_crt_carry on chosen coefficients v_j in [0, M61 M31), expected values from Python integers only: the weighted residues are
    derived by rotating v_j mod M61 / M31 back by the digit's weight, and after the file's finish() the digits must name
    sum_j a v_j 2^bitpos(j) mod 2^p - 1.  Coefficients at M61 M31 - 1 everywhere, at the run edges and at the last digit (wrap-around
    carry), every order of the two residues in the Garner step, factors up to 2^32 - 1, the narrowest and the widest words the engine's
    constructor admits.  The 128-bit carry holds all of it: v a < 2^124, and a carry is below 2^(124 - 15 + 1), so their sum stays below
    2^125; a run's outgoing carry (< 2^110) dies inside the following run's 8 x 15 bits, as k_crt_runs_fix needs."""
    import random
    p = 15 * n + 37 if width == "narrow" else _widest_p(n)
    pos, widths, w61, w31 = _geometry(p, n)
    assert min(widths) >= 15 and (width == "wide" or min(widths) == 15)
    Mp = (1 << p) - 1
    v = _pattern(pattern, n, random.Random(n * 31 + len(pattern)))
    assert all(0 <= x <= VMAX for x in v)
    # kernel: x61 = r61 2^unweight, unweight = -weight  =>  r61 = (v mod M61) 2^weight
    r61 = np.array([(x % M61) * pow(2, w, M61) % M61 for x, w in zip(v, w61)], dtype=np.uint64)
    r31 = np.array([(x % M31) * pow(2, w, M31) % M31 for x, w in zip(v, w31)], dtype=np.uint32)
    for a in (1, 3, 2**32 - 1):
        digits, residual, _ = crt_carry(p, n, odd, a, r61, r31)
        d = finish(digits, residual, widths)
        assert all(int(d[j]) >> widths[j] == 0 for j in range(n))
        got = sum(int(d[j]) << pos[j] for j in range(n)) % Mp
        want = sum(a * x << pos[j] for j, x in enumerate(v)) % Mp
        assert got == want, (p, n, odd, pattern, a)
