"""Host side of the lanes (no GPU): the four mi355_lanes_* symbols through header, binding and library, the plan token lanes=B, and the
ECM driver's run_lanes / ecm(lanes=B) on a stand-in engine with lanes made of CPU oracles, against ecm.run on one oracle per sigma."""
import ctypes
import math
import os
import random
import re

import pytest

import orc
from prmers_amd import ecm
from prmers_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- symbols ----

def test_lane_symbols_are_declared_bound_and_exported_and_stay_out_of_the_engine_header():
    header = open(os.path.join(ROOT, "include", "mi355_lanes.h")).read()
    declared = sorted(set(re.findall(r"\b(mi355_lanes_[a-z0-9_]+)\s*\(", header)))
    assert declared == sorted(E.LANE_EXPORTS) and len(declared) == 4
    lib = ctypes.CDLL(E.LIB_PATH)
    for name in declared:
        getattr(lib, name)
    engine_header = open(os.path.join(ROOT, "include", "mi355_engine.h")).read()
    for name in declared:
        assert name not in engine_header and name not in E.EXPORTS
    assert "mi355_lanes_" not in engine_header
    L = E.load_library()
    assert L.mi355_lanes_count(None) == 0 and b"null" in L.mi355_engine_last_error()
    capi = open(os.path.join(ROOT, "prmers_amd", "csrc", "capi.cpp")).read()
    for name in declared:
        assert re.search(r"\b%s\(" % name, capi)


# ---- the plan token ----

def test_plan_token_lanes():
    assert E.resolve_plan(9941, "lanes=4") == "marin-hip:n=512:m1=8:m2=32:c=4:lanes=4"
    assert E.resolve_plan(9941, "marin-hip:n=512:m1=8:m2=32:c=4:lanes=4") == "marin-hip:n=512:m1=8:m2=32:c=4:lanes=4"
    assert E.resolve_plan(9941, "lanes=1") == E.resolve_plan(9941) == "marin-hip:n=512:m1=8:m2=32:c=4"
    assert E.resolve_plan(9941, "m2=16,c=4,lanes=65535") == "marin-hip:n=512:m1=16:m2=16:c=4:lanes=65535"
    assert E.resolve_plan(3200123, "m2=8,split5") .endswith(":split5")


@pytest.mark.parametrize("p, spec", [(9941, "lanes=0"), (9941, "lanes=x"), (9941, "lanes=65536"), (9941, "lanes="), (9941, "lanes=-2"),
                                     (9941, "crt:9,lanes=2"), (3200123, "m2=8,split5,lanes=2")])
def test_bad_lanes_are_refused_with_a_message_that_names_the_token(p, spec):
    with pytest.raises(E.EngineError, match="lanes"):
        E.resolve_plan(p, spec)


def test_the_largest_transform_implies_split5_and_refuses_lanes():
    assert E.resolve_plan(4000000007).endswith(":split5")
    with pytest.raises(E.EngineError, match="lanes"):
        E.resolve_plan(4000000007, "lanes=2")


# ---- the ECM driver on a stand-in with lanes ----

class LaneOracles:
    """B CPU oracles behind the interface of an Engine with B lanes: every operation goes to all of them, lane= routes the I/O"""
    made = []

    def __init__(self, p, reg_count, device=0, plan=None, lanes=1):
        self.o = [orc.OracleEngine(p, reg_count) for _ in range(lanes)]
        self.p, self.n, self.reg_count, self.lanes = p, self.o[0].n, reg_count, lanes
        self.calls = {"square_mul": 0, "mul": 0, "set_multiplicand": 0}
        LaneOracles.made.append(self)

    def close(self):
        for o in self.o:
            o.close()

    def __enter__(self): return self
    def __exit__(self, *a): self.close()

    def _all(self, name, *a):
        if name in self.calls:
            self.calls[name] += 1
        for o in self.o:
            getattr(o, name)(*a)

    def set(self, dst, a): self._all("set", dst, a)
    def copy(self, dst, src): self._all("copy", dst, src)
    def square_mul(self, src, a=1): self._all("square_mul", src, a)
    def set_multiplicand(self, dst, src): self._all("set_multiplicand", dst, src)
    def mul(self, dst, src, a=1): self._all("mul", dst, src, a)
    def add(self, dst, src): self._all("add", dst, src)
    def sub_reg(self, dst, src): self._all("sub_reg", dst, src)

    def set_int(self, dst, v, lane=None):
        for o in (self.o if lane is None else [self.o[lane]]):
            o.set_int(dst, v)

    def get_int(self, src, lane=None):
        if lane is None and self.lanes > 1:
            raise RuntimeError("get_int: not with lanes")
        return self.o[lane or 0].get_int(src)


def _single(p, b1, b2, sigma, D):
    with orc.OracleEngine(p, ecm.registers_needed(D) if D else ecm.FIXED_REGISTERS) as eng:
        res = ecm.run(eng, p, b1, b2, sigma, D)
        return res, ((eng.get_int(ecm.R_XQ), eng.get_int(ecm.R_ZQ)) if res["squarings"] else None)


BATCHES = [
    # (p, b1, b2, D, sigmas, index and factor of the lane whose inversion fails)
    (3001, 30, 300, 30, [6, 8, 3217073, 36], 2, 3217073),
    (1009, 50, 0, None, [69, 7, 3454817], 2, 3454817),
]


@pytest.fixture(scope="module")
def singles():
    return {(p, s): _single(p, b1, b2, s, D) for p, b1, b2, D, sigmas, _, _ in BATCHES for s in sigmas}


@pytest.mark.parametrize("p, b1, b2, D, sigmas, bad, factor", BATCHES)
def test_run_lanes_gives_every_lane_what_run_gives_that_sigma(p, b1, b2, D, sigmas, bad, factor, singles):
    mp = (1 << p) - 1
    # the lane that fails does so in the inversion, on the CPU: v = 4 sigma is 0 modulo the factor
    assert pow(2, p, factor) == 1 and sigmas[bad] == factor
    assert math.gcd(16 * pow(factor * factor - 5, 3, mp) * pow(4 * factor, 4, mp) % mp, mp) % factor == 0
    with LaneOracles(p, ecm.registers_needed(D) if D else ecm.FIXED_REGISTERS, lanes=len(sigmas)) as eng:
        out = ecm.run_lanes(eng, p, b1, b2, sigmas, D)
        points = [(eng.get_int(ecm.R_XQ, lane=l), eng.get_int(ecm.R_ZQ, lane=l)) for l in range(len(sigmas))]
        calls = dict(eng.calls)
    assert len(out) == len(sigmas)
    found = 0
    for l, sigma in enumerate(sigmas):
        ref, pt = singles[(p, sigma)]
        assert (out[l]["g1"], out[l]["g2"]) == (ref["g1"], ref["g2"]) and out[l]["factors"] == ref["factors"] and out[l]["sigma"] == sigma
        assert (out[l]["b2"], out[l]["D"], out[l]["fused"]) == (ref["b2"], ref["D"], ref["fused"])
        if l == bad:
            assert ref["squarings"] == 0 and out[l]["g1"] % factor == 0 and out[l]["g2"] == 1
        else:
            assert (points[l][0] * pt[1] - pt[0] * points[l][1]) % mp == 0        # the same point, projectively
            assert (out[l]["squarings"], out[l]["products"], out[l]["prepares"]) == (ref["squarings"], ref["products"], ref["prepares"])
        found += bool(out[l]["factors"])
    assert found >= 2                                    # a curve that finds the factor, and the failed inversion
    # one sequence of engine calls for the whole batch
    assert calls["square_mul"] == out[0]["squarings"] and calls["mul"] == out[0]["products"] and calls["set_multiplicand"] == out[0]["prepares"]


def test_run_lanes_when_every_inversion_fails_runs_nothing():
    p, f = 1009, 3454817
    with LaneOracles(p, ecm.FIXED_REGISTERS, lanes=2) as eng:
        out = ecm.run_lanes(eng, p, 50, 0, [f, 2 * f])
        assert eng.calls["square_mul"] == 0
    assert [r["g1"] % f for r in out] == [0, 0] and all(r["squarings"] == 0 for r in out)


def test_run_lanes_wants_one_sigma_per_lane():
    with LaneOracles(1009, ecm.FIXED_REGISTERS, lanes=3) as eng:
        with pytest.raises(ValueError, match="lane"):
            ecm.run_lanes(eng, 1009, 50, 0, [6, 7])
        with pytest.raises(ValueError):
            ecm.run_lanes(eng, 1009, 50, 0, [6, 7, 5])     # sigma below the range
    with orc.OracleEngine(1009, ecm.FIXED_REGISTERS) as eng, pytest.raises(ValueError, match="lane"):
        ecm.run_lanes(eng, 1009, 50, 0, [6, 7])             # an engine without lanes has one


def test_ecm_entry_point_batches_by_lanes(monkeypatch):
    monkeypatch.setattr(E, "Engine", LaneOracles)
    LaneOracles.made = []
    # nothing found: 5 curves in batches of 3 are two whole batches, drawn like the single-lane run draws them
    res = ecm.ecm(1009, 20, 0, sigma=7, curves=5, lanes=3, seed=1)
    one = ecm.ecm(1009, 20, 0, sigma=7, curves=2, lanes=1, seed=1)
    assert [e.lanes for e in LaneOracles.made] == [3, 1] and "batch" not in one
    rng = random.Random(1)
    drawn = [7] + [rng.randrange(ecm.SIGMA_MIN, 1 << 32) for _ in range(5)]
    assert len(res["sigmas"]) % 3 == 0 and res["sigmas"] == drawn[:len(res["sigmas"])] and one["sigmas"] == drawn[:len(one["sigmas"])]
    assert len(res["sigmas"]) == 6 or res["factors"]
    assert len(res["batch"]) == 3 and [r["sigma"] for r in res["batch"]] == res["sigmas"][-3:]
    # sigma 69 finds 3454817 at B1 = 50 (tests/test_ecm.py): the first batch is the last
    res = ecm.ecm(1009, 50, 0, sigma=69, curves=9, lanes=2, seed=3)
    assert len(res["sigmas"]) == 2 and res["sigmas"][0] == 69 and res["sigma"] == 69
    assert 3454817 in res["factors"] and res["factors"] == sorted({f for r in res["batch"] for f in r["factors"]})
    for f in res["factors"]:
        assert pow(2, 1009, f) == 1
    with pytest.raises(ValueError):
        ecm.ecm(1009, 50, 0, lanes=0)
