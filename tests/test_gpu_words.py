"""Residue words packed and cut on the device (prmers_amd/csrc/canon.hip k_pack_words / k_unpack_words behind get_words / set_words of both
engines) against Python integers and against the host loops of the same engine (MI355_HOST_CARRY=1).  Needs a real MI355X:
python -m pytest tests -m gpu"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (p, plan): n = 8 (one block, widths 15 / 16); the automatic plans of 9941 (n = 512) and 100003 (n = 4096: more than one block of words and
# of digits); 929, the smallest exponent whose automatic plan is 5 * 2^k (n = 40: the digit offsets need the division by the odd factor);
# 9815459, a register-resident plan whose registers are tile-major with C > 1 (n = 2^19)
GOLDILOCKS = [(127, None), (9941, None), (100003, None), (929, None), (9815459, None)]
# (p, odd): crt handles whose digits exceed 32 bits, where get_digits refuses: n = 72 with widths 34 / 35, n = 32 with widths 39 / 40 (a digit
# spans three words), n = 288 (two blocks of digits)
CRT = [(2503, 9), (1279, 1), (9941, 9)]


class host_carry:
    """engines created inside pack and cut on the host"""
    def __enter__(self):
        self.old = os.environ.get("MI355_HOST_CARRY")
        os.environ["MI355_HOST_CARRY"] = "1"
    def __exit__(self, *a):
        if self.old is None:
            del os.environ["MI355_HOST_CARRY"]
        else:
            os.environ["MI355_HOST_CARRY"] = self.old


def values(p, rng):
    """the values of the issue, all below 2^p"""
    wc = (p + 31) // 32
    v = [0, 1, (1 << p) - 2, (1 << p) - 1, 1 << (p - 1)]
    for i in sorted({1, wc // 2, wc - 1}):
        if 0 < 32 * i < p:
            v += [1 << (32 * i), (1 << (32 * i)) - 1]
    v += [int.from_bytes(rng.bytes(wc * 4), "little") >> (wc * 32 - p) for _ in range(64)]
    assert all(0 <= x < (1 << p) for x in v)
    return v


def to_words(x, p):
    return np.frombuffer(int(x).to_bytes(((p + 31) // 32) * 4, "little"), dtype="<u4")


def to_int(w):
    return int.from_bytes(np.ascontiguousarray(w, dtype="<u4").tobytes(), "little")


def widths(p, n):
    j = np.arange(n + 1, dtype=np.uint64)
    off = (np.uint64(p) * j + np.uint64(n - 1)) // np.uint64(n)
    return np.diff(off).astype(np.uint64)


class Cutter:
    """the digits of an integer below 2^p in the variable base of (p, n), from its bits"""
    def __init__(self, p, n):
        self.p, self.ws = p, widths(p, n)
        self.starts = np.concatenate(([0], np.cumsum(self.ws)[:-1])).astype(np.int64)
        self.shift = (np.arange(p, dtype=np.int64) - np.repeat(self.starts, self.ws.astype(np.int64))).astype(np.uint64)

    def __call__(self, x):
        bits = np.unpackbits(np.frombuffer(int(x).to_bytes((self.p + 7) // 8, "little"), dtype=np.uint8), bitorder="little")[:self.p]
        return np.add.reduceat(bits.astype(np.uint64) << self.shift, self.starts)


def check_engine(e, h, p, set_digits):
    """e: the device path, h: the same engine under MI355_HOST_CARRY=1; set_digits(engine, reg, values): plain digit values in"""
    rng = np.random.default_rng(p)
    Mp = (1 << p) - 1
    cut = Cutter(p, e.n)
    assert int(cut.ws.sum()) == p
    for k, x in enumerate(values(p, rng)):
        want = x % Mp                                    # 2^p - 1 reads back as 0
        e.set_words(0, to_words(x, p))
        got = e.words(0)
        assert to_int(got) == want, (p, hex(x)[:40])
        # the host loops of a fresh engine agree, on the same register contents and on the same words
        h.set_words(0, to_words(x, p))
        assert np.array_equal(h.words(0), got)
        h.set_data(1, e.get_data(0))                     # the register the device cut, read by the host loop
        assert np.array_equal(h.words(1), got)
        e.set_data(1, h.get_data(0))                     # the register the host cut, packed by the device
        assert np.array_equal(e.words(1), got)
        # digits computed here -> words (at the large size for a part of the values: the cut is the slow step of this test)
        if p < 1000000 or k < 14:
            set_digits(e, 2, cut(x))
            assert to_int(e.words(2)) == want
    # weakly carried digits (after arithmetic) go through the canonical form first
    x = values(p, rng)[-1]
    e.set_words(0, to_words(x, p)); h.set_words(0, to_words(x, p))
    e.square_mul(0, 3); h.square_mul(0, 3)
    assert to_int(e.words(0)) == 3 * x * x % Mp == to_int(h.words(0))


@pytest.mark.parametrize("p,plan", GOLDILOCKS)
def test_goldilocks_words_on_device(p, plan):
    from prmers_amd import Engine
    from prmers_amd.engine import resolve_plan
    n = int(resolve_plan(p, plan).split("n=")[1].split(":")[0])
    odd = n
    while odd % 2 == 0:
        odd //= 2
    assert odd == (5 if p == 929 else 1)
    if p == 929:   # ... and it is the smallest: no odd exponent below it resolves to a multiple of 5
        assert all(int(resolve_plan(q).split("n=")[1].split(":")[0]) % 5 for q in range(3, 929, 2))
    if p == 9815459:
        assert ":c=4" in resolve_plan(p, plan) and n == 1 << 19
    Mp = (1 << p) - 1
    with Engine(p, 3, plan=plan) as e:
        with host_carry():
            h = Engine(p, 3, plan=plan)
        try:
            def set_digits(eng, reg, vals):
                eng.set_digits(reg, vals | (widths(p, eng.n) << np.uint64(32)))
            check_engine(e, h, p, set_digits)
            # words with bits at and above p: folded back (2^p = 1) on the host before the upload
            wc = e.word_count
            tops = [(1 << (32 * wc)) - 1, ((1 << (32 * wc)) - 1) ^ 1, Mp + 5, 1 << p]
            if p % 32 == 0:
                tops = []
            for x in tops:
                if x >> (32 * wc):
                    continue
                w = np.frombuffer(x.to_bytes(wc * 4, "little"), dtype="<u4")
                e.set_words(0, w); h.set_words(0, w)
                assert to_int(e.words(0)) == x % Mp == to_int(h.words(0)), hex(x)[:40]
        finally:
            h.close()


@pytest.mark.parametrize("p,odd", CRT)
def test_crt_words_on_device(p, odd):
    from prmers_amd import CrtEngine, Engine, EngineError
    with CrtEngine(p, odd, reg_count=3) as e:
        assert int(widths(p, e.n).max()) > 32
        with pytest.raises(EngineError, match="32 bits"):
            Engine.digits(e, 0)                          # the value | width << 32 form cannot hold these digits
        with host_carry():
            h = CrtEngine(p, odd, reg_count=3)
        try:
            check_engine(e, h, p, lambda eng, reg, vals: eng.set_digits(reg, vals))
            # this family keeps refusing words at and above 2^p, and takes a shorter or longer vector as before
            wc = e.word_count
            if p % 32:
                with pytest.raises(EngineError, match="does not fit"):
                    e.set_words(0, np.full(wc, 0xFFFFFFFF, dtype=np.uint32))
            e.set_words(0, np.array([7], dtype=np.uint32))
            assert e.get_int(0) == 7
            e.set_words(0, np.concatenate([to_words(12345678901234567890 % (1 << p), p), np.zeros(3, dtype=np.uint32)]))
            assert e.get_int(0) == 12345678901234567890 % (1 << p)
        finally:
            h.close()
