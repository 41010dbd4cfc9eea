"""Host-side operand bounds (no GPU): the size rule at the top of every range, the fused factor bound of the back sweeps
(plan.hpp fused_factor_limit) against a model of their carry chain, and the 32-bit range check of the Python binding."""
import os
import subprocess
import tempfile

import pytest

from prmers_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prmers_amd", "csrc")
FIELD = 2**64 - 2**32 + 1

# n -> the largest exponent that transform_size maps to n (the last size is capped by the 32-bit exponent)
P_MAX = {
    4: 119, 8: 239, 16: 463, 32: 927, 40: 1159, 64: 1791, 80: 2239, 128: 3583, 160: 4479, 256: 6911, 320: 8639, 512: 13823,
    640: 17279, 1024: 26623, 1280: 33279, 2048: 53247, 2560: 66559, 4096: 102399, 5120: 127999, 8192: 204799, 10240: 255999,
    16384: 393215, 20480: 491519, 32768: 786431, 40960: 983039, 65536: 1507327, 81920: 1884159, 131072: 3014655,
    163840: 3768319, 262144: 5767167, 327680: 7208959, 524288: 11534335, 655360: 14417919, 1048576: 22020095,
    1310720: 27525119, 2097152: 44040191, 2621440: 55050239, 4194304: 83886079, 5242880: 104857599, 8388608: 167772159,
    10485760: 209715199, 16777216: 318767103, 20971520: 398458879, 33554432: 637534207, 41943040: 796917759,
    67108864: 1207959551, 83886080: 1509949439, 167772160: 3019898879, 335544320: 4294967295,
}


@pytest.fixture(scope="module")
def plan_query():
    td = tempfile.mkdtemp()
    exe = os.path.join(td, "plan_query")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "host", "plan_query.cpp")])

    def run(*args):
        return subprocess.check_output([exe, *map(str, args)]).decode().splitlines()
    return run


def test_transform_size_at_the_top_of_every_range(plan_query):
    args = []
    for n, p in P_MAX.items():
        args += ["ts:%d" % p] + (["ts:%d" % (p + 1)] if p < 2**32 - 1 else [])
    got = {}
    for line in plan_query(*args):
        _, p, n = line.split()
        got[int(p[2:])] = int(n[2:])
    sizes = sorted(P_MAX)
    for i, n in enumerate(sizes):
        p = P_MAX[n]
        assert got[p] == n, (n, p)
        if p + 1 in got:
            assert got[p + 1] == sizes[i + 1], (n, p + 1, got[p + 1])


def _worst_case_terms(q, n, c, a):
    """Largest 64-bit term of the fused x a carry (adc_mul: r = dlo a + carry + addend, carry' = (r >> w) + (u >> w) a) over a run of 2c
    digits, a restatement of plan.hpp carry_chain_ok.  The inputs the bound holds for: digits below 2^w_j of their own width (q or
    q + 1), except the one per run that keeps the remainder of the carry-in (E); the addend of mul_add at 2^32.  The terms are written
    with D = 2^(q+1) - 1, but 2^(q+1) - 1 on EVERY digit is not covered: the coefficients are sum x_i x_j 2^c(i,j), and the terms leave
    the factor 2 of the weight exponents' carry out.  For digits inside their own widths a narrow digit below D / 2 and the shift by the
    narrow width in chi = U >> q make up for it; the exact chain (chain_model.py, test_factor_bound_cases.py) holds the margins and
    the overflow of the all-wide input.  -> (largest r / carry seen, convolution bound, E)"""
    D = 2**(q + 1) - 1
    runs = n // (2 * c)
    E_ = D
    for _ in range(64):
        U = (n - runs) * D * D + runs * E_ * E_ if c >= 2 else n * D * D
        chi = U >> q
        carry, top = 0, 0
        for _ in range(4096):   # up to the carry's fixed point: no run carries more
            r = D * a + carry + 2**32
            nxt = (r >> q) + chi * a
            top = max(top, r, nxt)
            if nxt == carry or top >= 2**64:
                break
            carry = nxt
        if c < 2 or top >= 2**64:
            return top, U, E_
        E2 = D + (carry >> (3 * q)) + 3
        if E2 <= E_:
            return top, U, E_
        E_ = E2
    return top, U, E_


def _exact(q, n, c, a):
    top, U, E_ = _worst_case_terms(q, n, c, a)
    return top < 2**64 and U < FIELD and E_ < 2**31


CASES = ["9815459", "136279841", "205271257", "86243", "216091", "1200007", "86243:m2=16,c=1", "53331:m2=16,split5"] + \
        [str(P_MAX[n]) for n in (2**18, 2**20, 5 * 2**19, 2**23, 5 * 2**21, 2**25, 5 * 2**23)]


def test_fused_factor_bound_against_the_carry_model(plan_query):
    """a_fast is the largest factor whose worst-case carry chain stays inside 64 bits, the field and the digit bound; one more and it
    does not (runs of two digits: capped at 15, the factor their local carry passes are sized for)"""
    seen = {}
    for line in plan_query(*CASES):
        f = dict(t.split("=") for t in line.split())
        p, n, q, c, a = (int(f[k]) for k in ("p", "n", "q", "c", "a_fast"))
        seen[p if c > 1 else (p, c)] = a
        assert a >= 15, line
        assert _exact(q, n, c, a), line
        if c >= 2:
            assert not _exact(q, n, c, a + 1), line
        else:
            assert a == 15 and _exact(q, n, c, 15), line
    # the BASELINE exponents (C2, C3, C4), as stated in include/mi355_engine.h
    assert seen[9815459] == 33537975 and seen[136279841] == 7254967 and seen[205271257] == 838834
    # the largest factors the oracle was found exact for sit below these (it overflows at 2^28 + 1 on C2)
    assert seen[9815459] < 2**28 + 1


def test_u32_arguments_are_checked_before_the_c_call():
    for v in (0, 1, 2**31, 2**32 - 1):
        assert E.u32_arg("factor", v) == v
    for v in (2**32, 2**32 + 3, -1, -(2**32)):
        with pytest.raises(ValueError):
            E.u32_arg("factor", v)
    for v in (3.0, "3", None):
        with pytest.raises(TypeError):
            E.u32_arg("factor", v)

    calls = []

    class Recorder:
        def __getattr__(self, name):
            def f(*args):
                calls.append(name)
                return 1
            return f

    eng = object.__new__(E.Engine)   # no library, no device: only the argument checks run
    eng.L, eng.h = Recorder(), 1
    bad = 2**32 + 3
    for call in (lambda: eng.square_mul(0, bad), lambda: eng.mul(0, 1, bad), lambda: eng.mul_add(0, 1, 2, bad),
                 lambda: eng.square_mul_copy(0, 1, bad), lambda: eng.mul_copy(0, 1, 2, bad), lambda: eng.square_mul_n(0, 4, bad),
                 lambda: eng.square_mul_n(0, 4, 1, bad), lambda: eng.sub(0, -1), lambda: eng.set(0, bad),
                 lambda: eng.time_square_mul(0, 10, bad)):
        with pytest.raises(ValueError):
            call()
    assert calls == []
    eng.square_mul(0, 2**32 - 1)
    assert calls == ["mi355_engine_square_mul"]
    eng.h = None
