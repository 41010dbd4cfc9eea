"""Engines with lanes (plan token lanes=B, include/mi355_lanes.h): B residues per register, every operation on all of them in one launch.
A register-machine program per lane against Python integers mod 2^p - 1, isolation between lanes, the per-lane I/O and what a lane
engine refuses, and ECM with one curve per lane against ecm.run on a plain engine.
Needs a real MI355X:  python -m pytest tests -m gpu"""
import ctypes
import random

import numpy as np
import pytest

import orc
from prmers_amd import ecm, pm1

pytestmark = pytest.mark.gpu

# (p, spec): the shapes of the generic kernel set that lanes run on (plan strings: tests/host/plan_query.cpp)
SHAPES = [
    (127, None),               # 1 x 4, c=4: one column, one tile
    (1277, None),              # 2 x 16
    (9941, None),              # 8 x 32
    (102701, "m2=64,c=2"),     # radix-5 columns 40 x 64, runs of two pairs
    (216091, None),            # radix-5, 80 x 64, c=4
    (86243, "c=1"),            # runs of two digits: carries taken at once plus relax passes (lane by lane from the host)
    (301447, None),            # 32 x 256
    (1600589, "m2=32,c=4"),    # 1280 x 32: the radix-5 resident columns would serve it; lanes take the generic set; an 80 KiB tile
    (9815459, None),           # 256 x 1024: the default is the radix-4 sets; several groups per lane
]
LANES = [2, 3, 5]              # an odd count; more lanes than tiles at the small sizes
MAX_LANES = max(LANES)
REGS = 10


# ---- integers mod 2^p - 1 (products through libgmp where it loads: Python's own take seconds each at 10^7 bits) ----

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


def inputs(p, seed=0):
    """(x, y, z) for MAX_LANES lanes: seeded full-size operands; lane 0 has x = 2^p - 2, lane 1 has x = 0"""
    rng = random.Random(1000 * p + seed)
    mp = (1 << p) - 1
    lanes = [[rng.getrandbits(p) % mp for _ in range(3)] for _ in range(MAX_LANES)]
    lanes[0][0] = mp - 1
    lanes[1][0] = 0
    return lanes


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


OUT_REGS = (0, 4, 5, 6, 7)


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
    ins = inputs(p)
    for l in range(lanes):
        if (p, l) not in _expected:
            _expected[(p, l)] = model(p, *ins[l])
    return [_expected[(p, l)] for l in range(lanes)]


# ---- (a) the program per lane ----

@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("p, spec", SHAPES)
def test_program_on_every_lane_matches_integers(p, spec, lanes):
    from prmers_amd import Engine
    from prmers_amd.engine import resolve_plan
    want = expected(p, lanes)
    with Engine(p, REGS, plan=spec, lanes=lanes) as e:
        assert e.lanes == lanes and e.describe() == resolve_plan(p, spec) + ":lanes=%d" % lanes
        run_program(e, inputs(p)[:lanes])
        for l in range(lanes):
            for r in OUT_REGS:
                assert e.get_int(r, lane=l) == want[l][r], (p, spec, lanes, "lane", l, "register", r)
        assert e.square_mul_prepare_is_fused()


def test_factor_above_the_fused_bound_on_every_lane():
    """at n = 2^19 the back sweep multiplies factors below 2^25 in itself (plan.hpp fused_factor_ok: the carry's (u >> 18) a term must stay
    in 64 bits); 2^32 - 5 runs as factor 1 and the run-wise factor pass, which has a lane form of its own"""
    from prmers_amd import Engine
    p, a = 9815459, 2**32 - 5
    ins = inputs(p)[:3]
    with Engine(p, 2, lanes=3) as e:
        e.set(0, 0)
        for l in range(3):
            e.set_int(0, ins[l][1], lane=l)
        e.square_mul(0)
        e.square_mul(0, a)                                  # on pending run carries
        for l in range(3):
            sq = orc.mers_reduce(_bigmul(ins[l][1], ins[l][1]), p)
            assert e.get_int(0, lane=l) == orc.mers_reduce(_bigmul(sq, sq) * a, p)


# ---- (b) isolation ----

@pytest.mark.parametrize("p, spec", [(1277, None), (9941, None), (86243, "c=1"), (301447, None)])
def test_lanes_do_not_see_each_other(p, spec):
    from prmers_amd import Engine
    base = inputs(p)[:3]
    other = [base[0], inputs(p, seed=1)[3], base[2]]        # lane 1 gets other values
    want, want_other = expected(p, 3), expected(p, lane_inputs=[other[1]])[0]
    with Engine(p, REGS, plan=spec, lanes=3) as e:
        run_program(e, base)
        first = {(l, r): e.words(r, lane=l).copy() for l in range(3) for r in OUT_REGS}
        run_program(e, other)
        for l in (0, 2):
            for r in OUT_REGS:
                assert np.array_equal(e.words(r, lane=l), first[(l, r)]) and e.get_int(r, lane=l) == want[l][r]
        for r in OUT_REGS:
            assert e.get_int(r, lane=1) == want_other[r]
        # one lane written, with run carries pending on the register: the others keep theirs
        e.square_mul(0)
        mp = (1 << p) - 1
        sq = [orc.mers_reduce(want[0][0] ** 2, p), None, orc.mers_reduce(want[2][0] ** 2, p)]
        e.set_int(0, 12345, lane=1)
        assert [e.get_int(0, lane=l) for l in range(3)] == [sq[0], 12345, sq[2]]
        assert e.res64(0, lane=1) == 12345 and e.res64(0, lane=0) == sq[0] & (2**64 - 1)
        e.set(0, 7)
        assert [e.get_int(0, lane=l) for l in range(3)] == [7, 7, 7]
        e.set_int(0, mp + 5)                                # lane=None: every lane, reduced
        assert [e.get_int(0, lane=l) for l in range(3)] == [5, 5, 5]


# ---- (c) a plain handle ----

def test_plain_engine_has_one_lane():
    from prmers_amd import Engine, EngineError
    with Engine(9941, 2) as e:
        assert e.lanes == 1 and "lanes" not in e.describe()
        e.set_int(0, 3**500, lane=0)
        assert e.get_int(0, lane=0) == e.get_int(0) == 3**500 and e.res64(0, lane=0) == e.res64(0) == 3**500 % 2**64
        for call in (lambda: e.get_int(0, lane=1), lambda: e.set_int(0, 5, lane=1), lambda: e.res64(0, lane=1)):
            with pytest.raises(EngineError, match="lane"):
                call()
        assert e.get_int(0) == 3**500
    with Engine(9941, 2, plan="lanes=1") as e:
        assert e.lanes == 1 and "lanes" not in e.describe()


# ---- (d) what a lane engine refuses ----

def test_refusals_leave_the_registers_intact():
    from prmers_amd import Engine, EngineError
    p = 9941
    with Engine(p, 4, lanes=3) as e:
        vals = [3**100 + l for l in range(3)]
        for r in (0, 1):
            e.set(r, 0)
            for l in range(3):
                e.set_int(r, vals[l] + r, lane=l)
        e.set_multiplicand(2, 1)
        whole = [lambda: e.get_words(0), lambda: e.res64(0), lambda: e.is_equal(0, 1), lambda: e.get_data(0), lambda: e.get_checkpoint(),
                 lambda: e.time_square_mul(0, 4), lambda: e.digits(0), lambda: e.get_int(0)]
        for call in whole:
            with pytest.raises(EngineError, match="not with lanes|mi355_lanes_"):
                call()
        assert e.set_data(0, np.zeros(e.get_register_data_size(), dtype=np.uint8)) is False
        assert e.set_checkpoint(np.zeros(e.get_checkpoint_size(), dtype=np.uint8)) is False
        for call in (lambda: e.get_int(0, lane=3), lambda: e.set_int(0, 5, lane=3), lambda: e.res64(0, lane=3)):
            with pytest.raises(EngineError, match="lane"):
                call()
        with pytest.raises(EngineError, match="image"):
            e.set_int(2, 5, lane=0)                          # the kind is the register's
        with pytest.raises(EngineError, match="image|residue"):
            e.get_int(2, lane=0)
        for l in range(3):
            assert e.get_int(0, lane=l) == vals[l] and e.get_int(1, lane=l) == vals[l] + 1
        e.mul(0, 2)                                          # register 2 is still the image of register 1
        mp = (1 << p) - 1
        assert [e.get_int(0, lane=l) for l in range(3)] == [vals[l] * (vals[l] + 1) % mp for l in range(3)]
    with pytest.raises(EngineError, match="lanes"):
        Engine(p, 2, plan="crt:9", lanes=2)
    with pytest.raises(EngineError, match="lanes"):
        Engine(p, 2, lanes=0)


# ---- (e) ECM, one curve per lane ----

ECM_P, ECM_F = 301447, 142885879


def test_ecm_one_curve_per_lane_matches_single_curves():
    from prmers_amd import Engine
    p, b1, b2, D, sigmas = ECM_P, 50, 1000, 30, [37, 6, ECM_F, 77]
    regs = ecm.registers_needed(D)
    with Engine(p, regs) as e:
        single = [ecm.run(e, p, b1, b2, s, D) for s in sigmas]
    with Engine(p, regs, lanes=len(sigmas)) as e:
        out = ecm.run_lanes(e, p, b1, b2, sigmas, D)
        again = ecm.run_lanes(e, p, b1, b2, sigmas[::-1], D)      # a second batch on the same engine: images of the first are overwritten
    for l, s in enumerate(sigmas):
        assert (out[l]["g1"], out[l]["g2"]) == (single[l]["g1"], single[l]["g2"]) and out[l]["sigma"] == s and out[l]["fused"] is True
        assert (again[3 - l]["g1"], again[3 - l]["g2"]) == (out[l]["g1"], out[l]["g2"])
    assert out[0]["g1"] == 1 and out[0]["g2"] % ECM_F == 0                 # sigma 37: stage 2
    assert (out[1]["g1"], out[1]["g2"], out[1]["factors"]) == (1, 1, [])   # sigma 6: nothing
    assert out[2]["g1"] % ECM_F == 0 and out[2]["g2"] == 1                 # the inversion fails and reports the factor
    live = [r for r, s in zip(single, sigmas) if s != ECM_F][0]
    assert (out[0]["squarings"], out[0]["products"], out[0]["prepares"]) == (live["squarings"], live["products"], live["prepares"])


def test_ecm_entry_point_with_lanes():
    p = ECM_P
    res = ecm.ecm(p, 50, 1000, sigma=6, curves=6, lanes=3, seed=1)
    assert len(res["sigmas"]) % 3 == 0 and len(res["sigmas"]) in (3, 6) and res["sigmas"][0] == 6
    rng = random.Random(1)
    assert res["sigmas"][1:] == [rng.randrange(ecm.SIGMA_MIN, 1 << 32) for _ in range(len(res["sigmas"]) - 1)]
    for f in res["factors"]:
        assert pow(2, p, f) == 1
    assert len(res["sigmas"]) == 6 or res["factors"]
    rc = ecm.main([str(p), "50", "1000", "--sigma", "37", "--curves", "2", "--lanes", "2", "--D", "30"])
    assert rc == 0                                                         # sigma 37 finds 142885879 in stage 2
    rc = ecm.main([str(p), "50", "--sigma", "6", "--curves", "2", "--lanes", "2", "--seed", "5"])
    found = ecm.ecm(p, 50, 0, sigma=6, curves=2, lanes=2, seed=5)["factors"]
    assert rc == (0 if found else 1)
