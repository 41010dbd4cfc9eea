"""The device carry scan (prmers_amd/csrc/canon.hip) where one thread of k_scan_top spans several blocks, which is every size above
2^20 digits: designed carry chains (tests/canon_cases.py, checked on the CPU by tests/test_canon_cases.py) through the C ABI of both
field families, at the smallest sizes with two and three blocks per stretch; digits wider than 32 bits in the chain; and the host
fallback behind the sticky "digit too wide" flag.  Needs a real MI355X:  python -m pytest tests -m gpu"""
import numpy as np
import pytest

import canon_cases as cc

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
LOW32 = np.uint64(0xffffffff)


def run_vectors(e, h, w, crt):
    """Every designed vector through engine e (device chain) and h (MI355_HOST_CARRY=1: the sequential host loop).  Returns the
    failed checks as "vector: what" so that one run names every vector a wrong scan gets wrong."""
    n = e.n
    nb, per, S, ns = cc.geometry(n)
    ones = cc.ones_of(w)
    read = (lambda x, r: x.raw_digits(r)) if crt else (lambda x, r: x.digits(r) & LOW32)
    spots = (0, 63, 64, cc.BLOCK, S, n - 1)
    failed = []
    for k, c in enumerate(cc.iter_cases(n, w)):
        def check(ok, what):
            if not ok:
                failed.append("%s: %s" % (c.name, what))
        # the device path is the subject: digits of at most 2^w stay at most 2^w through the local passes, the "too wide" flag cannot rise
        assert (c.d <= (np.uint64(1) << w)).all(), c.name
        e.set_digits(0, c.d); h.set_digits(0, c.d)
        check(np.array_equal(read(e, 0), c.t), "digits")
        check(np.array_equal(read(h, 0), read(e, 0)), "digits differ from the host path")
        if c.zero and not crt:   # the Goldilocks engine keeps the reference's res64 of the all-ones vector
            check(e.res64(0) == h.res64(0), "res64 differs from the host path")
        else:
            check(e.res64(0) == (0 if c.zero else cc.low64(c.t, w)), "res64")
        other = c.t.copy()
        if c.zero:
            e.set(1, 0); other[:] = 0
        else:
            e.set_digits(1, c.t)
        check(e.is_equal(0, 1) and e.is_equal(1, 0), "is_equal with the canonical form")
        other[spots[k % len(spots)]] ^= np.uint64(1)   # one unit off at a wave, block or stretch edge: still canonical, another value
        e.set_digits(3, other)
        check(not e.is_equal(0, 3) and not e.is_equal(3, 0), "is_equal with a unit off at digit %d" % spots[k % len(spots)])
        if crt:
            e.set(2, 0); e.sub_reg(2, 0)
            check(np.array_equal(e.raw_digits(2), ones if c.zero else ones - c.t), "sub_reg")
    return failed


@pytest.mark.parametrize("p,n,blocks,per,plan", [
    (27525101, 5 << 18, 320, 2, "marin-hip:n=1310720:m1=640:m2=1024:c=4"),     # 160 stretches of two blocks, 96 idle threads
    (55050001, 5 << 19, 640, 3, "marin-hip:n=2621440:m1=1280:m2=1024:c=4"),    # 213 stretches of three blocks and one of one block
])
def test_carry_chains_across_the_blocks_of_a_stretch(p, n, blocks, per, plan, monkeypatch):
    from prmers_amd import Engine, resolve_plan
    assert resolve_plan(p) == plan
    assert cc.geometry(n)[:2] == (blocks, per)
    w = cc.widths(p, n)
    assert set(w.tolist()) == {20, 21}
    with Engine(p, 4) as e:
        assert e.n == n and e.describe() == plan, e.describe()
        monkeypatch.setenv("MI355_HOST_CARRY", "1")
        with Engine(p, 4) as h:
            monkeypatch.delenv("MI355_HOST_CARRY")
            failed = run_vectors(e, h, w, crt=False)
    assert not failed, failed


def test_carry_chains_of_digits_wider_than_32_bits(monkeypatch):
    """the second family at 9 2^17 digits of 34 and 35 bits (288 blocks, two per stretch): uint32_t(v >> w) and T(1) << w with w > 32"""
    from prmers_amd import CrtEngine
    p, n = 41187401, 9 << 17
    assert cc.geometry(n)[:2] == (288, 2)
    w = cc.widths(p, n)
    assert set(w.tolist()) == {34, 35}
    with CrtEngine(p, 9, n) as e:
        assert e.n == n
        monkeypatch.setenv("MI355_HOST_CARRY", "1")
        with CrtEngine(p, 9, n) as h:
            monkeypatch.delenv("MI355_HOST_CARRY")
            failed = run_vectors(e, h, w, crt=True)
    assert not failed, failed


def value_of(d, w, p):
    v, sh = 0, 0
    for dj, wj in zip(d.tolist(), w.tolist()):
        v += int(dj) << sh
        sh += int(wj)
    return v % ((1 << p) - 1)


def canonical_of(v, w):
    out = np.zeros(w.size, dtype=np.uint64)
    for j, wj in enumerate(w.tolist()):
        out[j] = v & ((1 << int(wj)) - 1)
        v >>= int(wj)
    return out


@pytest.mark.parametrize("wide", [True, False])
def test_host_fallback_of_the_second_family(wide):
    """Digits below 2^62 at widths 16-17: three local passes leave more than 2^w, the scan raises its sticky flag and get_digits, res64,
    is_equal and sub_reg take the host carry.  Control: the same digits cut to 3w - 2 bits stay on the device chain.  Python integers
    over the 4608 digits are the reference.
    (The Goldilocks engine's digits are u32, so its fallback needs widths of at most 10 bits: test_host_fallback_of_the_goldilocks_engine.)"""
    from prmers_amd import CrtEngine
    p, n = 73751, 9 << 9
    M = (1 << p) - 1
    w = cc.widths(p, n)
    assert set(w.tolist()) == {16, 17}
    d = np.random.default_rng(4).integers(0, 1 << 62, n, dtype=np.uint64)
    limit = np.uint64(1) << w
    if wide:
        assert (cc.local_passes(d, w) > limit).any()      # the flag rises
    else:
        d &= (np.uint64(1) << (np.uint64(3) * w - np.uint64(2))) - np.uint64(1)
        assert (cc.local_passes(d, w) <= limit).all()     # it does not
    want = value_of(d, w, p)
    assert 0 < want < M
    with CrtEngine(p, 9, n) as e:
        assert e.n == n
        e.set_digits(0, d)
        assert np.array_equal(e.raw_digits(0), canonical_of(want, w))
        assert e.get_int(0) == want
        assert e.res64(0) == want & M64
        e.set_int(1, want)
        assert e.is_equal(0, 1) and e.is_equal(1, 0)
        e.set_int(2, (want + 1) % M)
        assert not e.is_equal(0, 2) and not e.is_equal(2, 0)
        e.set_int(3, 12345); e.sub_reg(3, 0)
        assert e.get_int(3) == (12345 - want) % M
        # the flag is sticky on the device and cleared by every read of it: a canonical register afterwards is not sent to the host for it
        assert e.get_int(1) == want and e.res64(1) == want & M64


@pytest.mark.parametrize("wide", [True, False])
def test_host_fallback_of_the_goldilocks_engine(wide):
    """u32 digits reach the fallback only where widths are at most 10 bits: the size rule gives n = 4 below p = 44 (p = 31: widths 7-8,
    a plan tests/test_gpu_parity.py runs).  Full 32-bit digits there leave more than 2^w after three passes; 3w - 2 bits do not."""
    from prmers_amd import Engine, resolve_plan
    p, n = 31, 4
    M = (1 << p) - 1
    assert resolve_plan(p) == "marin-hip:n=4:m1=1:m2=2:c=2"
    w = cc.widths(p, n)
    assert w.tolist() == [8, 8, 8, 7]
    d = np.array([0xfedcba98, 0x89abcdef, 0xffffffff, 0x80000001], dtype=np.uint64)
    limit = np.uint64(1) << w
    if wide:
        assert (cc.local_passes(d, w) > limit).any()
    else:
        d &= (np.uint64(1) << (np.uint64(3) * w - np.uint64(2))) - np.uint64(1)
        assert (cc.local_passes(d, w) <= limit).all()
    want = value_of(d, w, p)
    assert 0 < want < M
    with Engine(p, 4) as e:
        assert e.n == n
        e.set_digits(0, d)
        assert np.array_equal(e.digits(0) & LOW32, canonical_of(want, w))
        assert np.array_equal(e.digits(0) >> np.uint64(32), w)
        assert e.get_int(0) == want
        assert e.res64(0) == want
        e.set_int(1, want)
        assert e.is_equal(0, 1) and e.is_equal(1, 0)
        e.set_int(2, (want + 1) % M)
        assert not e.is_equal(0, 2) and not e.is_equal(2, 0)
        assert e.get_int(1) == want and e.res64(1) == want
