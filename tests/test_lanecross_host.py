"""Host side of the product across lanes (no GPU): the symbol of include/mi355_lanecross.h through header, binding and library;
prmers_amd/lanecross.py on a stand-in that keeps one Python integer a lane, with mul_sibling written from the rule; and ECM's affine
stage 2 with inverse="engine" on lanes made of CPU oracles, where mul_sibling moves the partner's raw image between the oracles, against
inverse="host" on the same stand-in and against the integer model of tests/test_ecm_affine.py."""
import ctypes
import math
import os
import random
import re

import pytest

import orc
from prmers_amd import ecm, ecm_edwards, lanecross, pm1
from prmers_amd import engine as E
from test_ecm_affine import m_run_affine
from test_lanes_host import LaneOracles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mi355_lanecross_mul_sibling"


# ---- symbols ----

def test_the_symbol_is_declared_in_its_own_header_bound_exported_and_refuses_a_null_handle():
    header = open(os.path.join(ROOT, "include", "mi355_lanecross.h")).read()
    assert sorted(set(re.findall(r"\b(mi355_lanecross_[a-z0-9_]+)\s*\(", header))) == [NAME] == E.LANECROSS_EXPORTS
    for prefix in ("mi355_engine_", "mi355_crt_", "mi355_lanes_", "mi355_lanewise_", "mi355_batch_"):
        assert not re.findall(r"\b%s[a-z0-9_]+\s*\(" % prefix, header), prefix
    for other in ("mi355_engine.h", "mi355_lanes.h", "mi355_batch.h", "mi355_lanewise.h"):
        assert "mi355_lanecross_" not in open(os.path.join(ROOT, "include", other)).read()
    assert NAME not in E.EXPORTS + E.LANE_EXPORTS + E.BATCH_EXPORTS + E.LANEWISE_EXPORTS
    getattr(ctypes.CDLL(E.LIB_PATH), NAME)
    L = E.load_library()
    assert L.mi355_lanecross_mul_sibling.argtypes[-1] is ctypes.c_uint32 and callable(E.Engine.mul_sibling)
    assert L.mi355_lanecross_mul_sibling(None, 0, 1, 2, 0) == 0 and b"null" in L.mi355_engine_last_error()
    capi = open(os.path.join(ROOT, "prmers_amd", "csrc", "capi.cpp")).read()
    assert re.search(r"\b%s\(" % NAME, capi) and "mi355_lanecross.h" in capi


# ---- lanecross.py on integers ----

class IntLanes:
    """one Python integer a lane and register; an image is the value itself, with the register's kind kept as the engine keeps it"""

    def __init__(self, p, lanes, regs):
        self.p, self.lanes, self.mp = p, lanes, (1 << p) - 1
        self.r = [[0] * lanes for _ in range(regs)]
        self.image = [False] * regs
        self.log = []

    def set(self, dst, v):
        self.r[dst], self.image[dst] = [v % self.mp] * self.lanes, False

    def copy(self, dst, src):
        self.log.append("copy")
        self.r[dst], self.image[dst] = list(self.r[src]), self.image[src]

    def set_multiplicand(self, dst, src):
        assert not self.image[src]
        self.log.append("prep")
        self.r[dst], self.image[dst] = list(self.r[src]), True

    def mul_sibling(self, dst, src, alt, level):
        assert not self.image[dst] and self.image[src] and self.image[alt] and dst not in (src, alt) and level <= 31
        self.log.append("sib")
        out = []
        for l in range(self.lanes):
            g = ((l >> level) ^ 1) << level                  # the rule of include/mi355_lanecross.h
            out.append(self.r[dst][l] * (self.r[src][g] if g < self.lanes else self.r[alt][l]) % self.mp)
        self.r[dst] = out

    def get_int(self, src, lane=None):
        assert not self.image[src] and (lane is not None or self.lanes == 1)
        self.log.append("read")
        return self.r[src][lane or 0]

    def set_int(self, dst, v, lane=None):
        assert lane is None
        self.log.append("write")
        self.set(dst, v)


def test_sibling_and_levels_restate_the_rule():
    assert [lanecross.levels(b) for b in (1, 2, 3, 4, 5, 8, 9, 512, 513)] == [0, 1, 2, 2, 3, 3, 4, 9, 10]
    assert [lanecross.sibling(l, 0, 5) for l in range(5)] == [1, 0, 3, 2, None]
    assert [lanecross.sibling(l, 1, 5) for l in range(5)] == [2, 2, 0, 0, None]
    assert [lanecross.sibling(l, 2, 5) for l in range(5)] == [4, 4, 4, 4, 0]
    assert [lanecross.sibling(l, 3, 5) for l in range(5)] == [None] * 5
    assert lanecross.sibling(0, 10, 1025) == 1024 and lanecross.sibling(1024, 10, 1025) == 0 and lanecross.sibling(1, 10, 1025) == 1024
    assert lanecross.registers_needed(1) == 2 and lanecross.registers_needed(512) == 11
    with pytest.raises(ValueError):
        lanecross.levels(0)


P = 67                                                       # 2^67 - 1 = 193707721 x 761838257287
Z, U = 0, 1


def _machine(B, values):
    L = lanecross.levels(B)
    m = IntLanes(P, B, L + 4)
    m.r[Z] = list(values)
    m.r[U] = [77] * B
    work = list(range(2, L + 4))
    lanecross.prepare_one(m, work[1])
    del m.log[:]
    return m, work, L


@pytest.mark.parametrize("B", list(range(1, 71)) + [300])
def test_every_lane_gets_the_product_and_then_its_inverse(B):
    mp = (1 << P) - 1
    rng = random.Random(B)
    values = [rng.randrange(2, mp) for _ in range(B)]
    m, work, L = _machine(B, values)
    # the up pass alone: every lane holds the product
    T, ONE, R = work[0], work[1], work[2:]
    m.copy(T, Z)
    for s in range(L):
        m.set_multiplicand(R[s], T)
        m.mul_sibling(T, R[s], ONE, s)
    assert m.r[T] == [math.prod(values) % mp] * B
    for negate in (False, True):
        m, work, L = _machine(B, values)
        assert lanecross.invert(m, Z, U, work, negate) == (True, 1)
        assert m.r[Z] == values and not m.image[U]
        assert [u * z % mp for u, z in zip(m.r[U], values)] == [mp - 1 if negate else 1] * B
        assert m.log == ["copy"] + ["prep", "sib"] * L + ["read", "write"] + ["sib"] * L


@pytest.mark.parametrize("B, bad, value, g", [(5, 3, 0, (1 << P) - 1), (13, 12, 193707721 * 10, 193707721), (1, 0, 761838257287, 761838257287),
                                             (8, 0, 0, (1 << P) - 1)])
def test_a_product_without_an_inverse_is_reported_with_its_gcd_and_nothing_is_written(B, bad, value, g):
    mp = (1 << P) - 1
    rng = random.Random(B)
    values = [rng.randrange(2, mp) for _ in range(B)]
    values[bad] = value
    m, work, L = _machine(B, values)
    assert lanecross.invert(m, Z, U, work) == (False, g)
    assert m.r[Z] == values and m.r[U] == [77] * B and "write" not in m.log and m.log.count("sib") == L


def test_invert_wants_its_registers():
    m, work, L = _machine(5, [3] * 5)
    with pytest.raises(ValueError, match="work registers"):
        lanecross.invert(m, Z, U, work[:-1])
    with pytest.raises(ValueError, match="work registers"):
        lanecross.invert(m, Z, U, [Z] + work[1:])


# ---- ECM on lanes of CPU oracles ----

class CrossOracles(LaneOracles):
    """LaneOracles with the product across lanes -- the partner's raw image goes into a spare register of the lane's own oracle, which
    then multiplies by it -- and with the lane-wise read and write; every call is logged"""

    def __init__(self, p, reg_count, device=0, plan=None, lanes=1):
        LaneOracles.__init__(self, p, reg_count + 1, lanes=lanes)
        self.reg_count, self.spare = reg_count, reg_count
        self.log = []

    def _all(self, name, *a):
        self.log.append(name)
        LaneOracles._all(self, name, *a)

    def mul_sibling(self, dst, src, alt, level):
        assert dst not in (src, alt) and max(dst, src, alt) < self.reg_count
        self.log.append("mul_sibling")
        raw = []
        for l in range(self.lanes):
            g = lanecross.sibling(l, level, self.lanes)
            raw.append(self.o[l].o.raw(alt) if g is None else self.o[g].o.raw(src))
        for l, o in enumerate(self.o):
            o.o.L.orc_set_raw(o.o.h, self.spare, raw[l].ctypes.data_as(ctypes.c_void_p))
            o.mul(dst, self.spare)

    def get_ints(self, src):
        self.log.append("get_ints")
        return [o.get_int(src) for o in self.o]

    def set_ints(self, dst, values):
        self.log.append("set_ints")
        for o, v in zip(self.o, values):
            o.set_int(dst, v)

    def get_int(self, src, lane=None):
        self.log.append("get_int")
        return LaneOracles.get_int(self, src, lane)

    def set_int(self, dst, v, lane=None):
        self.log.append("set_int")
        LaneOracles.set_int(self, dst, v, lane)


def test_the_stand_in_s_mul_sibling_is_the_rule_on_integers():
    p, B = 127, 5
    mp = (1 << p) - 1
    with CrossOracles(p, 4, lanes=B) as e:
        e.set_ints(0, [3 + l for l in range(B)])
        e.set_ints(1, [100 + l for l in range(B)]); e.set_multiplicand(1, 1)
        e.set_ints(2, [7] * B); e.set_multiplicand(2, 2)
        for level in range(4):
            before = e.get_ints(0)
            e.mul_sibling(0, 1, 2, level)
            g = [lanecross.sibling(l, level, B) for l in range(B)]
            assert e.get_ints(0) == [before[l] * (7 if g[l] is None else 100 + g[l]) % mp for l in range(B)]


def _engine_and_host(p, b1, b2, D, sigmas, driver=ecm):
    B = len(sigmas)
    regs = driver.registers_needed(D, "affine", lanes=B, inverse="engine")
    assert regs == ecm.registers_needed(D, "affine") + lanecross.levels(B) + 3
    with CrossOracles(p, regs, lanes=B) as e:
        out = driver.run_lanes(e, p, b1, b2, sigmas, D, stage2="affine", inverse="engine")
        acc = e.get_ints(ecm.R_A)
        log = list(e.log)
    with CrossOracles(p, ecm.registers_needed(D, "affine"), lanes=B) as e:
        host = driver.run_lanes(e, p, b1, b2, sigmas, D, stage2="affine")
        acc_host = e.get_ints(ecm.R_A)
        log_host = list(e.log)
    return out, acc, log, host, acc_host, log_host


CASES = [
    # (p, b1, b2, D, sigmas, fallback blocks)
    (3001, 30, 300, 30, [6, 8], 0),
    (10007, 20, 500, 210, [10, 11], 0),
    (3001, 30, 300, 30, [8, 6, 7], 0),               # three lanes: two levels, a lane without a sibling at level 0
    (1009, 20, 104, 210, [7, 12, 8], 1),             # the factor sits in the baby block's Z product: that block goes the host's way
]


@pytest.mark.parametrize("p, b1, b2, D, sigmas, fallbacks", CASES)
def test_the_engine_inverse_gives_what_the_host_inverse_and_the_model_give(p, b1, b2, D, sigmas, fallbacks):
    mp = (1 << p) - 1
    want = [m_run_affine(s, b1, b2, D, mp) for s in sigmas]
    out, acc, log, host, acc_host, log_host = _engine_and_host(p, b1, b2, D, sigmas)
    for res in (out, host):
        assert [(r["g1"], r["g2"]) for r in res] == [w[:2] for w in want]
        assert [r["factors"] for r in res] == [[f for f in w[:2] if 1 < f < mp] for w in want]
        assert all(r["normalised"] == want[0][4] and r["stage2"] == "affine" for r in res)
    assert acc == acc_host == [w[2] for w in want]
    assert all(r["inverse"] == "engine" and r["inverse_fallbacks"] == fallbacks for r in out)
    assert set(out[0]) - set(host[0]) == {"inverse", "inverse_fallbacks"} and set(host[0]) <= set(out[0])
    if fallbacks:
        assert out[1]["g2"] == 3454817 and (fallbacks >= 1) == (not all(w[3] for w in want))
    # the reads and writes of every lane: a24, x0, the start point; the stage-1 Z and the final A zacc -- and a fallback block's pair.
    # The host's way has a pair for every block.
    blocks = want[0][5]
    assert (log.count("set_ints"), log.count("get_ints")) == (3 + fallbacks, 2 + fallbacks + 1)          # (+ 1: this test's own read of R_A)
    assert (log_host.count("set_ints"), log_host.count("get_ints")) == (3 + blocks, 2 + blocks + 1)
    L = lanecross.levels(len(sigmas))
    assert log.count("mul_sibling") == L * (2 * blocks - fallbacks) and log.count("get_int") == blocks and log.count("set_int") == blocks - fallbacks
    assert "mul_sibling" not in log_host
    # products and prepares: a block adds the Z product's pair and lanecross.invert's L prepares and L or 2 L products
    extra = out[0]["products"] - host[0]["products"], out[0]["prepares"] - host[0]["prepares"]
    assert extra == (blocks + 1 + L * (2 * blocks - fallbacks), blocks + 1 + L * blocks)


def test_the_edwards_driver_takes_the_inverse():
    p, b1, b2, D, sigmas = 3001, 30, 300, 30, [6, 8]
    out, acc, log, host, acc_host, _ = _engine_and_host(p, b1, b2, D, sigmas, ecm_edwards)
    assert [(r["g1"], r["g2"]) for r in out] == [(r["g1"], r["g2"]) for r in host] == [(1, 3217073), (1, 1)] and acc == acc_host
    assert out[0]["inverse"] == "engine" and out[0]["inverse_fallbacks"] == 0 and out[0]["curve"] == "edwards" and "inverse" not in host[0]


def test_a_single_run_has_no_levels():
    p, b1, b2, D, sigma = 3001, 30, 300, 30, 6
    want = m_run_affine(sigma, b1, b2, D, (1 << p) - 1)
    assert ecm.registers_needed(D, "affine", lanes=1, inverse="engine") == ecm.registers_needed(D, "affine") + 3
    with CrossOracles(p, ecm.registers_needed(D, "affine", inverse="engine"), lanes=1) as e:
        res = ecm.run(e, p, b1, b2, sigma, D, stage2="affine", inverse="engine")
        assert e.get_int(ecm.R_A) == want[2] and "mul_sibling" not in e.log
    assert (res["g1"], res["g2"], res["normalised"], res["inverse"], res["inverse_fallbacks"]) == (1, 3217073, want[4], "engine", 0)


def test_the_engine_inverse_is_refused_without_affine_and_without_mul_sibling():
    p, D = 1009, 30
    regs = ecm.registers_needed(D, "affine", lanes=2, inverse="engine")
    with CrossOracles(p, regs, lanes=2) as e:
        for driver in (ecm, ecm_edwards):
            with pytest.raises(ValueError, match="affine"):
                driver.run_lanes(e, p, 20, 120, [7, 8], D, inverse="engine")
            with pytest.raises(ValueError, match="inverse"):
                driver.run_lanes(e, p, 20, 120, [7, 8], D, stage2="affine", inverse="device")
        with pytest.raises(ValueError, match="registers"):
            ecm.run_lanes(e, p, 20, 1000, [7, 8], 210, stage2="affine", inverse="engine")
        assert e.log == []
    with LaneOracles(p, regs, lanes=2) as e:                  # no mul_sibling
        for driver in (ecm, ecm_edwards):
            with pytest.raises(ValueError, match="mul_sibling"):
                driver.run_lanes(e, p, 20, 120, [7, 8], D, stage2="affine", inverse="engine")
    with orc.OracleEngine(p, regs) as e, pytest.raises(ValueError, match="mul_sibling"):
        ecm.run(e, p, 20, 120, 7, D, stage2="affine", inverse="engine")
    with pytest.raises(ValueError, match="affine"):
        ecm.ecm(p, 20, 120, inverse="engine")
    with pytest.raises(ValueError, match="affine"):
        ecm.registers_needed(D, inverse="engine")


def test_registers_needed_without_the_new_arguments_is_what_it_was():
    for D in pm1.D_CHOICES:
        J = len(pm1.residues(D))
        assert ecm.registers_needed(D) == ecm.registers_needed(D, "projective") == 2 * J + ecm.FIXED_REGISTERS
        assert ecm.registers_needed(D, "affine") == ecm.registers_needed(D, "affine", lanes=512) == 3 * J + ecm.FIXED_REGISTERS
        for B, L in ((1, 0), (2, 1), (3, 2), (512, 9), (513, 10)):
            assert ecm.registers_needed(D, "affine", lanes=B, inverse="engine") == 3 * J + ecm.FIXED_REGISTERS + L + 3
            assert ecm_edwards.registers_needed(D, "affine", B, "engine") == ecm.registers_needed(D, "affine", B, "engine")
    assert ecm_edwards.registers_needed() == ecm_edwards.FIXED_REGISTERS
    n = 1 << 20
    budget = (ecm.registers_needed(210, "affine") + 1) * 8 * n
    assert ecm.choose_D(n, 20, 1000, budget, "affine") == 210 and ecm.choose_D(n, 20, 1000, budget, "affine", 512, "engine") == 30


def test_the_cli_and_the_entry_point_pass_the_inverse(monkeypatch, capsys):
    seen = {}

    def fake(*a, **kw):
        seen["kw"] = kw
        return {"factors": []}
    monkeypatch.setattr(ecm, "ecm", fake)
    assert ecm.main(["1009", "20", "104", "--stage2", "affine", "--inverse", "engine"]) == 1 and seen["kw"] == {"stage2": "affine", "inverse": "engine"}
    assert ecm.main(["1009", "20", "104", "--stage2", "affine", "--inverse", "host"]) == 1 and seen["kw"] == {"stage2": "affine"}
    with pytest.raises(SystemExit):
        ecm.main(["1009", "20", "104", "--inverse", "device"])
    capsys.readouterr()
    monkeypatch.undo()
    monkeypatch.setattr(E, "Engine", CrossOracles)
    LaneOracles.made = []
    res = ecm.ecm(1009, 20, 104, sigma=12, D=210, lanes=3, seed=5, stage2="affine", inverse="engine", curve="edwards")
    assert LaneOracles.made[-1].reg_count == ecm.registers_needed(210, "affine", 3, "engine") and LaneOracles.made[-1].lanes == 3
    assert 3454817 in res["factors"] and res["batch"][0]["inverse"] == "engine" and res["batch"][0]["inverse_fallbacks"] >= 1
    res = ecm.ecm(3001, 30, 300, sigma=6, D=30, stage2="affine", inverse="engine")
    assert LaneOracles.made[-1].reg_count == ecm.registers_needed(30, "affine", 1, "engine") and LaneOracles.made[-1].lanes == 1
    assert res["factors"] == [3217073] and res["inverse"] == "engine"
