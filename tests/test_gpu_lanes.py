"""Engines with lanes (plan token lanes=B, include/mi355_lanes.h): B residues per register, every operation on all of them in one launch.
A register-machine program per lane against Python integers mod 2^p - 1, isolation between lanes, the per-lane I/O and what a lane
engine refuses, and ECM with one curve per lane against ecm.run on a plain engine.
Needs a real MI355X:  python -m pytest tests -m gpu"""
import random

import numpy as np
import pytest

import orc
from lane_program import MAX_LANES, OUT_REGS, REGS, _bigmul, expected, inputs, model, run_program  # noqa: F401 -- the program and its model
from prmers_amd import ecm

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
assert MAX_LANES == max(LANES)


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


# ---- (f) ECM at 64 lanes ----

WIDE_P, WIDE_F, WIDE_NAMED = 3001, 3217073, [6, 8, 3217073, 36]      # tests/test_lanes_host.py: the third inversion fails on the factor


def test_ecm_at_64_lanes_matches_64_single_curves():
    from prmers_amd import Engine
    p, b1, b2, D = WIDE_P, 30, 300, 30
    rng = random.Random(7)
    sigmas = WIDE_NAMED + [rng.randrange(ecm.SIGMA_MIN, 1 << 32) for _ in range(60)]
    assert len(sigmas) == len(set(sigmas)) == 64 and pow(2, p, WIDE_F) == 1
    regs = ecm.registers_needed(D)
    with Engine(p, regs) as e:
        single = [ecm.run(e, p, b1, b2, s, D) for s in sigmas]
    oracle = []
    for s in WIDE_NAMED:
        with orc.OracleEngine(p, regs) as o:
            oracle.append(ecm.run(o, p, b1, b2, s, D))
    with Engine(p, regs, lanes=64) as e:
        out = ecm.run_lanes(e, p, b1, b2, sigmas, D)
    assert len(out) == 64
    for l, s in enumerate(sigmas):
        assert out[l]["sigma"] == s, ("lane", l)
        assert (out[l]["g1"], out[l]["g2"], out[l]["factors"]) == (single[l]["g1"], single[l]["g2"], single[l]["factors"]), ("lane", l, "sigma", s)
        for f in out[l]["factors"]:
            assert pow(2, p, f) == 1, ("lane", l, "sigma", s, f)
    for l, ref in enumerate(oracle):
        assert (out[l]["g1"], out[l]["g2"], out[l]["factors"]) == (ref["g1"], ref["g2"], ref["factors"]), ("lane", l, "against the CPU oracle")
    bad = WIDE_NAMED.index(WIDE_F)
    assert out[bad]["g1"] % WIDE_F == 0 and out[bad]["g2"] == 1 and single[bad]["squarings"] == 0   # the failed inversion reports the factor
    assert [l for l in range(64) if l != bad and any(f % WIDE_F == 0 for f in out[l]["factors"])]     # and a curve finds it
