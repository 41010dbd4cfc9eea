"""Lane engines at the lane counts ECM runs them at, on the thread shapes only a lane count reaches, and through the operations, read
paths and switches that the program of test_gpu_lanes.py leaves out.  The cases are lane_cases.py (test_lane_cases.py says what they
pin); every value of every lane is compared with Python integers mod 2^p - 1 (products through libgmp where it loads), bit for bit.
Needs a real MI355X:  python -m pytest tests -m gpu"""
import itertools
import random

import numpy as np
import pytest

import lane_cases as lc
from lane_program import OUT_REGS, REGS, expected_of, have_gmp, inputs, mulmod, powmod, run_program

pytestmark = pytest.mark.gpu

SWITCHES = ("MI355_KERNELS", "MI355_TUNE", "MI355_HOST_CARRY")


def Engine(*a, **k):
    from prmers_amd import Engine as E
    return E(*a, **k)


def clear_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def values(p, lanes, seed):
    """one full-size residue per lane, all different"""
    rng = random.Random(7919 * p + seed)
    mp = (1 << p) - 1
    return [rng.getrandbits(p) % mp for _ in range(lanes)]


def put(e, r, vs):
    e.set(r, 0)
    for l, v in enumerate(vs):
        e.set_int(r, v, lane=l)


def check(e, r, want, what):
    """register r of every lane"""
    for l in range(e.lanes):
        assert e.get_int(r, lane=l) == want[l], (e.p, what, "lane", l, "register", r)


# ---- B: the program on every lane, at these counts ------------------------------------------------------------------------------

@pytest.mark.parametrize("p, spec, lanes", lc.CASES, ids=[lc.case_id(c) for c in lc.CASES])
def test_program_on_every_lane_at_wide_lane_counts(p, spec, lanes, monkeypatch):
    from prmers_amd.engine import resolve_plan
    if p > 10**6 and not have_gmp():
        pytest.skip("libgmp does not load: the integer model of p = %d takes minutes in Python's own products" % p)
    clear_switches(monkeypatch)
    ins = inputs(p, lanes=lanes)
    mp = (1 << p) - 1
    assert len(ins) == lanes and ins[0][0] == mp - 1 and ins[1][0] == 0 and ins[-1][0] == mp - 1
    want = expected_of(p, ins)
    with Engine(p, REGS, plan=spec, lanes=lanes) as e:
        assert e.lanes == lanes and e.describe() == resolve_plan(p, spec) + ":lanes=%d" % lanes
        run_program(e, ins)
        for l in range(lanes):
            for r in OUT_REGS:
                assert e.get_int(r, lane=l) == want[l][r], (p, spec, lanes, "lane", l, "register", r)


# ---- C: the operations and read paths the program leaves out -----------------------------------------------------------------

OPS = [(9941, None, 9), (301447, None, 9), (86243, "c=1", 3)]   # 301447 at 9 lanes: beyond both switches; c=1: carries taken at once
OPS_IDS = [lc.case_id(c) for c in OPS]
EXPONENTS = [0, 1, 2, 0xB5, 2**64 - 1]


@pytest.mark.parametrize("p, spec, lanes", OPS, ids=OPS_IDS)
def test_copy_of_pending_carries_and_of_an_image(p, spec, lanes, monkeypatch):
    clear_switches(monkeypatch)
    x, y = values(p, lanes, 1), values(p, lanes, 2)
    with Engine(p, 6, plan=spec, lanes=lanes) as e:
        put(e, 0, x); put(e, 2, y)
        e.square_mul(0, 3)                                   # run carries pending on every lane
        e.copy(1, 0)
        e.square_mul(0); e.square_mul(1)                     # both take the carries in
        x2 = [mulmod(p, v, v, 3) for v in x]
        x4 = [mulmod(p, v, v) for v in x2]
        check(e, 0, x4, "square after copy, the source"); check(e, 1, x4, "square after copy, the copy")
        e.set_multiplicand(3, 2)
        e.copy(4, 3)                                         # an image: the whole slot
        e.mul(0, 4); e.mul(1, 3)
        x4y = [mulmod(p, a, b) for a, b in zip(x4, y)]
        check(e, 0, x4y, "mul by the copied image"); check(e, 1, x4y, "mul by the image")
        e.copy(5, 0)                                         # pending again, read without another sweep
        check(e, 5, x4y, "copy read directly"); check(e, 0, x4y, "its source")
        e.copy(4, 5)                                         # digits over an image: the register is a residue again
        e.square_mul(4)
        check(e, 4, [mulmod(p, v, v) for v in x4y], "digits copied over an image")


@pytest.mark.parametrize("p, spec, lanes", OPS, ids=OPS_IDS)
def test_addsub_copy_with_all_four_outputs(p, spec, lanes, monkeypatch):
    clear_switches(monkeypatch)
    mp = (1 << p) - 1
    x, y = values(p, lanes, 3), values(p, lanes, 4)
    with Engine(p, 6, plan=spec, lanes=lanes) as e:
        put(e, 0, x); put(e, 1, y)
        e.square_mul(0); e.square_mul(1, 3)                  # both operands with carries pending
        a, b = [mulmod(p, v, v) for v in x], [mulmod(p, v, v, 3) for v in y]
        e.addsub_copy(2, 3, 4, 5, 0, 1)
        s, d = [(u + v) % mp for u, v in zip(a, b)], [(u - v) % mp for u, v in zip(a, b)]
        for r, want, what in ((2, s, "sum"), (4, s, "sum copy"), (3, d, "difference"), (5, d, "difference copy"), (0, a, "a"), (1, b, "b")):
            check(e, r, want, "addsub_copy: " + what)
        e.addsub_copy(2, 3, 4, 5, 0, 1)                      # again; the outputs go into a squaring with their carries pending
        for r in (2, 3, 4, 5):
            e.square_mul(r)
        s2, d2 = [mulmod(p, v, v) for v in s], [mulmod(p, v, v) for v in d]
        for r, want in ((2, s2), (4, s2), (3, d2), (5, d2)):
            check(e, r, want, "addsub_copy, then squared")


@pytest.mark.parametrize("square_b", [False, True], ids=["exp_mul", "exp_mul2"])
@pytest.mark.parametrize("p, spec, lanes", OPS, ids=OPS_IDS)
def test_exp_mul_on_every_lane(p, spec, lanes, square_b, monkeypatch):
    clear_switches(monkeypatch)
    x, y, z = values(p, lanes, 5), values(p, lanes, 6), values(p, lanes, 7)
    a = [mulmod(p, v, v) for v in x]                         # a enters with carries pending
    b = [mulmod(p, v, v) for v in y] if square_b else y
    with Engine(p, 4, plan=spec, lanes=lanes) as e:
        for h in EXPONENTS:
            put(e, 0, x); put(e, 1, y); put(e, 3, z)
            e.square_mul(0)
            (e.exp_mul2 if square_b else e.exp_mul)(0, h, 1, 2)
            want = [mulmod(p, powmod(p, u, h), v) for u, v in zip(a, b)]
            check(e, 0, want, "a^h b, h = %#x" % h)
            # b and tmp end as images: of b, and of a as it was (h = 0: a copy of b)
            e.mul(3, 1)
            zb = [mulmod(p, u, v) for u, v in zip(z, b)]
            check(e, 3, zb, "mul by the image left in b, h = %#x" % h)
            e.mul(3, 2)
            check(e, 3, [mulmod(p, u, v) for u, v in zip(zb, b if h == 0 else a)], "mul by the image left in tmp, h = %#x" % h)


BITS, NBITS = 0x1B5A5C3E96, 37                               # first bit set, last bit clear


@pytest.mark.parametrize("p, spec, lanes", OPS, ids=OPS_IDS)
def test_square_mul_bits_and_pow(p, spec, lanes, monkeypatch):
    clear_switches(monkeypatch)
    assert BITS.bit_length() == NBITS and BITS & 1 == 0
    x = values(p, lanes, 8)
    with Engine(p, 3, plan=spec, lanes=lanes) as e:
        put(e, 0, x)
        e.square_mul_bits(0, 3, (BITS << (40 - NBITS)).to_bytes(5, "big"), NBITS)
        want = list(x)
        for i in range(NBITS - 1, -1, -1):
            want = [mulmod(p, v, v, 3 if (BITS >> i) & 1 else 1) for v in want]
        assert want == [mulmod(p, powmod(p, v, 1 << NBITS), powmod(p, 3, BITS)) for v in x]
        check(e, 0, want, "square_mul_bits")
        for exponent in (1000003, 0):
            put(e, 1, x)
            e.pow(2, 1, exponent)
            check(e, 2, [powmod(p, v, exponent) for v in x], "pow, e = %d" % exponent)


@pytest.mark.parametrize("p, spec, lanes", OPS, ids=OPS_IDS)
def test_set_digits_writes_every_lane(p, spec, lanes, monkeypatch):
    clear_switches(monkeypatch)
    v = values(p, 1, 9)[0]
    with Engine(p, 2, plan=spec) as plain:
        plain.set_int(0, v)
        d = plain.digits(0)
    with Engine(p, 2, plan=spec, lanes=lanes) as e:
        put(e, 0, values(p, lanes, 10))
        e.square_mul(0)                                      # carries pending on the register that is overwritten
        e.set_digits(0, d)
        check(e, 0, [v] * lanes, "set_digits")
        e.square_mul(0)
        check(e, 0, [mulmod(p, v, v)] * lanes, "set_digits, then squared")


@pytest.mark.parametrize("p, spec, lanes, a", lc.FACTOR_CASES, ids=["%s-a%d" % (lc.case_id(c[:3]), c[3]) for c in lc.FACTOR_CASES])
def test_factors_above_the_fused_bound(p, spec, lanes, a, monkeypatch):
    """every operation that takes a factor, each on a register whose last result left carries pending; then mul_add onto its own
    destination, which only the fused sweep can do: taken with a small factor, refused with a large one, the registers intact"""
    from prmers_amd import EngineError
    clear_switches(monkeypatch)
    mp = (1 << p) - 1
    x, y, z = values(p, lanes, 11), values(p, lanes, 12), values(p, lanes, 13)
    with Engine(p, 7, plan=spec, lanes=lanes) as e:
        put(e, 0, x); put(e, 1, y); put(e, 3, z)
        e.set_multiplicand(2, 1)
        e.square_mul(0); e.square_mul(3)
        v, z2 = [mulmod(p, u, u) for u in x], [mulmod(p, u, u) for u in z]
        e.mul(0, 2, a)
        v = [mulmod(p, u, w, a) for u, w in zip(v, y)]
        e.mul_add(0, 2, 3, a)
        v = [(mulmod(p, u, w, a) + t) % mp for u, w, t in zip(v, y, z2)]
        e.mul_copy(0, 2, 4, a)
        v = [mulmod(p, u, w, a) for u, w in zip(v, y)]
        r4 = v
        e.square_mul_copy(4, 5, a)
        r4 = [mulmod(p, u, u, a) for u in r4]
        r5_old = r4
        e.square_mul_prepare(5, 6, a)
        r5 = [mulmod(p, u, u, a) for u in r5_old]
        e.mul(0, 6)
        v = [mulmod(p, u, w) for u, w in zip(v, r5_old)]
        e.mul_add(0, 2, 0, lc.SMALL_FACTOR)
        v = [(mulmod(p, u, w, lc.SMALL_FACTOR) + u) % mp for u, w in zip(v, y)]
        with pytest.raises(EngineError, match="add_src == dst needs the fused sweep, which takes factors up to the plan's fused bound only"):
            e.mul_add(0, 2, 0, a)
        for r, want, what in ((0, v, "the chain"), (3, z2, "the addend"), (4, r4, "square_mul_copy"), (5, r5, "square_mul_prepare")):
            check(e, r, want, what + ", factor %d" % a)
        e.mul(4, 2)                                          # the image is intact as well
        check(e, 4, [mulmod(p, u, w) for u, w in zip(r4, y)], "mul after the refusal")


@pytest.mark.parametrize("p, spec, lanes", OPS + [(204799, None, 3)], ids=OPS_IDS + ["204799-lanes3-two-products"])
def test_mul_sum_of_one_image_twice_and_as_two_products(p, spec, lanes, monkeypatch):
    clear_switches(monkeypatch)
    mp = (1 << p) - 1
    x, y, z = values(p, lanes, 14), values(p, lanes, 15), values(p, lanes, 16)
    with Engine(p, 6, plan=spec, lanes=lanes) as e:
        assert e.mul_sum_is_fused() == (p != 204799)         # 204799: no room for the summed operand (tests/mul_sum_cases.py)
        put(e, 0, x); put(e, 1, y); put(e, 2, z)
        e.set_multiplicand(3, 1); e.set_multiplicand(4, 2)
        e.square_mul(0, 3)                                   # dst with carries pending
        v = [mulmod(p, u, u, 3) for u in x]
        e.mul_sum(0, 3, 3, 5)
        v = [mulmod(p, u, 2 * w % mp) for u, w in zip(v, y)]
        check(e, 0, v, "mul_sum(dst, a, a, tmp)")
        e.square_mul(0)
        v = [mulmod(p, u, u) for u in v]
        e.mul_sum(0, 3, 4, 5)
        v = [mulmod(p, u, (w + t) % mp) for u, w, t in zip(v, y, z)]
        check(e, 0, v, "mul_sum(dst, a, b, tmp) on pending carries")
        e.mul(0, 3); e.mul(0, 4)                             # the images are left intact
        check(e, 0, [mulmod(p, mulmod(p, u, w), t) for u, w, t in zip(v, y, z)], "the images after mul_sum")


def io_edges(e, plain, label=""):
    """writes and reads of one lane at the edges of the residue range, on a register whose other lanes have carries pending; `plain` is
    an engine without lanes of the same plan, made under the same switches"""
    p, lanes, wc = e.p, e.lanes, e.word_count
    mp = (1 << p) - 1
    x = values(p, lanes, 17)
    put(e, 0, x)
    e.square_mul(0)
    keep = [mulmod(p, v, v) for v in x]
    raw = lambda v: np.frombuffer(int(v).to_bytes(4 * wc, "little"), dtype="<u4")
    edges = [mp, 1 << p, (1 << (32 * wc)) - 1, mp - 1, 0, 1, (1 << 64) - 1, values(p, 1, 18)[0]]
    assert (1 << p) < (1 << (32 * wc))
    for lane, v in zip(itertools.cycle(sorted({0, lanes // 2, lanes - 1})), edges):
        e.set_words(0, raw(v), lane=lane)
        plain.set_words(0, raw(v))
        keep[lane] = v % mp
        assert e.get_int(0, lane=lane) == plain.get_int(0) == v % mp, (label, "lane", lane, "value %#x..." % (v >> max(0, p - 16)))
        assert e.res64(0, lane=lane) == plain.res64(0), (label, "res64, lane", lane)
        if v == mp and p >= 64:
            assert e.res64(0, lane=lane) == 2**64 - 1      # the all-ones digits, as the reference's digit::res64 reads them
        elif v % mp != 0 or v == 0:
            assert e.res64(0, lane=lane) == (v % mp) & (2**64 - 1)
        for l in range(lanes):
            assert e.get_int(0, lane=l) == keep[l], (label, "after a write to lane", lane, "lane", l)
    e.set_int(0, mp, lane=lanes - 1)                         # through the binding, which reduces first
    assert e.get_int(0, lane=lanes - 1) == 0 and e.res64(0, lane=lanes - 1) == 0
    keep[lanes - 1] = 0
    e.square_mul(0)                                          # the lanes written take part like the others
    check(e, 0, [mulmod(p, v, v) for v in keep], label + " squared after the writes")


@pytest.mark.parametrize("p, spec, lanes", OPS, ids=OPS_IDS)
def test_one_lane_written_and_read_at_the_edges_of_the_range(p, spec, lanes, monkeypatch):
    clear_switches(monkeypatch)
    with Engine(p, 2, plan=spec, lanes=lanes) as e, Engine(p, 1, plan=spec) as plain:
        io_edges(e, plain)


# ---- D: the switches ------------------------------------------------------------------------------------------------------------

SWITCH_SHAPES = [(9941, "m2=16,c=4", 3), (301447, None, 9), (86243, "c=1", 3),
                 (9815459, None, 2)]    # its single-lane default is the radix-4 set, which lanes must not pick up
KERNELS = [None, "generic", "v2rows", "v2cols"]
TUNE = [0, 1, 32, 33]                   # bit 0: the tile order of the back sweep (xcd_tile in k_back, lanes as grid.y)
HOST_CARRY = [None, "1"]                # the host read path lane by lane, and the host branch of the lane writes


@pytest.mark.parametrize("p, spec, lanes", SWITCH_SHAPES, ids=[lc.case_id(c) for c in SWITCH_SHAPES])
def test_every_switch_setting_gives_the_same_integers(p, spec, lanes, monkeypatch):
    from prmers_amd.engine import resolve_plan
    clear_switches(monkeypatch)
    text = resolve_plan(p, spec) + ":lanes=%d" % lanes
    ins = inputs(p, lanes=lanes)
    want = expected_of(p, ins)
    for ks, tune, host in itertools.product(KERNELS, TUNE, HOST_CARRY):
        label = "kernels=%s tune=%d host_carry=%s" % (ks, tune, host)
        for name, value in zip(SWITCHES, (ks, tune, host)):
            if value is None: monkeypatch.delenv(name, raising=False)
            else: monkeypatch.setenv(name, str(value))
        with Engine(p, REGS, plan=spec, lanes=lanes) as e:
            assert e.describe() == text, (label, e.describe())
            run_program(e, ins)
            for l in range(lanes):
                for r in OUT_REGS:
                    assert e.get_int(r, lane=l) == want[l][r], (p, spec, label, "lane", l, "register", r)
            assert e.res64(7, lane=lanes - 1) == want[-1][7] & (2**64 - 1), label
            if host == "1" and tune == 0:                    # the tile order plays no part in the I/O
                with Engine(p, 1, plan=spec) as plain:
                    io_edges(e, plain, label)


# ---- E: a lane beyond 4 GiB -----------------------------------------------------------------------------------------------------

def free_device_memory():
    """bytes free on device 0: torch.cuda.mem_get_info() where torch's HIP runtime is up; otherwise hipMemGetInfo of the runtime the
    engine library runs on.  (A torch wheel may bring a HIP runtime of its own: whichever of the two is loaded second cannot start in a
    process where the first is live, and if torch came first the engine library runs on torch's.)"""
    import ctypes
    import sys
    torch = sys.modules.get("torch")
    if torch is not None and torch.cuda.is_initialized():
        return torch.cuda.mem_get_info()[0]
    from prmers_amd.engine import load_library
    load_library()
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line}, key=lambda path: ("/torch/" in path, path))
    assert paths, "no HIP runtime is mapped"
    hip = ctypes.CDLL(paths[0])
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    rc = hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total))
    assert rc == 0, "hipMemGetInfo: error %d" % rc
    return free.value


def test_a_lane_that_starts_four_gibibytes_into_its_slot(monkeypatch):
    """p = 9815459: a lane is 8 n = 4 MiB, so lane 1024 of 1025 starts exactly 2^32 bytes into each of the three slots (two registers and
    the work buffer: 12 GiB); a lane offset kept in 32 bits would put it on lane 0"""
    p, lanes = 9815459, 1025
    free = free_device_memory()
    if free < 16 << 30:
        pytest.skip("%.1f GiB of device memory free, the engine of this test takes 12 GiB: needs 16 GiB" % (free / 2**30))
    clear_switches(monkeypatch)
    mp = (1 << p) - 1
    common = values(p, 1, 20)[0]
    own = dict(zip((0, 1023, 1024), values(p, 3, 21)))
    with Engine(p, 2, lanes=lanes) as e:
        assert e.n * 8 * 1024 == 1 << 32
        e.set_int(0, common)
        for l, v in own.items():
            e.set_int(0, v, lane=l)
        e.square_mul(0, 3)
        e.set_multiplicand(1, 0)
        e.square_mul(0)
        e.mul(0, 1)
        e.sub(0, 2)
        model = {}
        for l in (0, 1, 512, 1023, 1024):
            x = own.get(l, common)
            if x not in model:
                v1 = mulmod(p, x, x, 3)
                model[x] = (mulmod(p, mulmod(p, v1, v1), v1) - 2) % mp
            assert e.get_int(0, lane=l) == model[x], ("lane", l)
        assert len(model) == 4
