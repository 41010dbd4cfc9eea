"""ECM on twisted Edwards curves (prmers_amd/ecm_edwards.py) on engines with lanes: every lane's stage-1 point against the integer model of
tests/test_ecm_edwards.py, the factors of tests/test_ecm.py, and the on-curve check through Engine.equal_lanes with a fault injected into
one lane (rolled back) and a persistent one (raised).
Needs a real MI355X:  python -m pytest tests -m gpu"""
import math

import pytest

from prmers_amd import ecm
from prmers_amd import ecm_edwards as ed
from test_ecm_edwards import m_stage1

pytestmark = pytest.mark.gpu

B1, CHECK_EVERY = 50, 8


def degenerate_sigma(p):
    """sigma = -5 mod 2^p - 1: u + v = 0, so the inversion fails with g = 2^p - 1 (2^1277 - 1 has no known factor to fail on)"""
    return (1 << p) - 1 - 5


def point(e):
    """X, Y, Z, T of every lane"""
    regs = [e.get_ints(r) for r in ed.POINT]
    return [tuple(col[l] for col in regs) for l in range(e.lanes)]


def add_one(reg, at, lane, times=1):
    left = [times]

    def fault(position, eng):
        if position == at and left[0]:
            left[0] -= 1
            eng.set_int(reg, eng.get_int(reg, lane=lane) + 1, lane=lane)
    return fault


# (p, sigmas, onelaunch, batch)
ENGINES = [
    (1277, [6, 7, 8, 11, degenerate_sigma(1277), 69, 2**31 + 11, 12], True, True),
    (9941, [6, degenerate_sigma(9941), 7, 2**32 - 1], False, False),
]


@pytest.mark.parametrize("p, sigmas, onelaunch, batch", ENGINES, ids=["1277-8lanes-onelaunch-batch", "9941-4lanes"])
def test_every_lane_is_the_models_point_and_a_fault_in_one_lane_is_rolled_back(p, sigmas, onelaunch, batch):
    from prmers_amd import Engine
    mp = (1 << p) - 1
    lanes = len(sigmas)
    bad = [l for l, s in enumerate(sigmas) if s == degenerate_sigma(p)]
    assert len(bad) == 1 and ed.curve(sigmas[bad[0]], mp)[5] == mp
    with Engine(p, ed.FIXED_REGISTERS, lanes=lanes, onelaunch=onelaunch) as e:
        out = ed.run_lanes(e, p, B1, 0, sigmas, check_every=CHECK_EVERY, batch=batch)
        clean = point(e)
        digits = None
        for l, s in enumerate(sigmas):
            if l in bad:
                assert out[l]["g1"] == mp and out[l]["factors"] == []
                continue
            want, digits = m_stage1(s, B1, mp)
            assert clean[l] == tuple(c % mp for c in want), (p, "lane", l)
            assert out[l]["g1"] == math.gcd(want[0], mp) and out[l]["sigma"] == s and out[l]["curve"] == "edwards"
        steps = len(digits) - 1
        assert (out[0]["doublings"], out[0]["rollbacks"], out[0]["checks"]) == (steps, 0, -(-steps // CHECK_EVERY)) and out[0]["fused"]
        assert ("launches" in out[0]) == batch
        # lane 3 alone is corrupted, once: every lane goes back, and the end is the clean run's, bit for bit
        hit = ed.run_lanes(e, p, B1, 0, sigmas, check_every=CHECK_EVERY, batch=batch, fault=add_one(ed.R_Y, 13, 3))
        assert point(e) == clean
        assert all(r["rollbacks"] == 1 and r["checks"] == out[0]["checks"] + 1 for r in hit)
        assert [(r["g1"], r["factors"]) for r in hit] == [(r["g1"], r["factors"]) for r in out]
        # a fault that comes back after the roll-back
        with pytest.raises(ed.EcmCheckError, match="lane 3") as err:
            ed.run_lanes(e, p, B1, 0, sigmas, check_every=CHECK_EVERY, batch=batch, fault=add_one(ed.R_T, 13, 3, times=2))
        assert err.value.lanes == [3] and err.value.position == 16
        if batch:
            assert e.batch_stats()[3] == 0
            e.sync()


def test_known_factors_stage_1_and_stage_2():
    from prmers_amd import Engine
    # 3454817 | 2^1009 - 1 with sigma = 69 at B1 = 50, in one lane of three
    p = 1009
    with Engine(p, ed.FIXED_REGISTERS, lanes=3, onelaunch=True) as e:
        out = ed.run_lanes(e, p, 50, 0, [7, 69, 11], check_every=CHECK_EVERY, batch=True)
    assert [r["factors"] for r in out] == [[], [3454817], []] and all(r["rollbacks"] == 0 for r in out)
    # stage 2 only (tests/test_ecm.py): sigma = 6 finds 3217073 | 2^3001 - 1 with B1 = 30, B2 = 300, D = 30; sigma = 8 finds nothing
    p, D = 3001, 30
    with Engine(p, ed.registers_needed(D), lanes=2) as e:
        out = ed.run_lanes(e, p, 30, 300, [6, 8], D, check_every=CHECK_EVERY)
        plain = ecm.run_lanes(e, p, 30, 300, [6, 8], D)
    assert [(r["g1"], r["g2"]) for r in out] == [(1, 3217073), (1, 1)] == [(r["g1"], r["g2"]) for r in plain]
    assert out[0]["factors"] == [3217073] and out[0]["D"] == D and out[0]["b2"] == 300
