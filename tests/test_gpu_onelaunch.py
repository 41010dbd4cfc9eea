"""One-launch products (plan token `onelaunch`; kernels.hip k_onelaunch): every lane of every case of onelaunch_cases.py against Python
integers mod 2^p - 1, registers and images against the three-launch generic path bit for bit, lanes that share a work-group kept apart,
engines of the largest and the smallest size used in turn, and ECM batches against the CPU oracle.  test_onelaunch_cases.py says what
the cases pin.  Needs a real MI355X:  python -m pytest tests -m gpu"""
import random

import numpy as np
import pytest

import onelaunch_cases as oc
from lane_program import OUT_REGS, REGS, expected_of, inputs, mulmod, run_program
from prmers_amd import ecm
from test_lanes_host import BATCHES, _single

pytestmark = pytest.mark.gpu

SWITCHES = ("MI355_KERNELS", "MI355_TUNE", "MI355_HOST_CARRY")
FIELD = 2**64 - 2**32 + 1


def Engine(*a, **k):
    from prmers_amd import Engine as E
    return E(*a, **k)


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def values(p, count, seed):
    rng = random.Random(104729 * p + seed)
    mp = (1 << p) - 1
    return [rng.getrandbits(p) % mp for _ in range(count)]


def put(e, r, vs):
    e.set(r, 0)
    for l, v in enumerate(vs):
        e.set_int(r, v, lane=l)


def check(e, r, want, what):
    for l in range(e.lanes):
        assert e.get_int(r, lane=l) == want[l], (e.p, what, "lane", l, "of", e.lanes, "register", r)


# ---- the program on every lane of every case ------------------------------------------------------------------------------------

@pytest.mark.parametrize("p, spec, lanes", oc.CASES, ids=[oc.case_id(c) for c in oc.CASES])
def test_program_on_every_lane(p, spec, lanes):
    from prmers_amd.engine import resolve_plan
    ins = inputs(p, lanes=lanes)
    mp = (1 << p) - 1
    assert len(ins) == lanes and ins[0][0] == mp - 1 and ins[-1][0] == mp - 1
    want = expected_of(p, ins)
    with Engine(p, REGS, plan=spec, lanes=lanes, onelaunch=True) as e:
        assert e.lanes == lanes and e.describe() == resolve_plan(p, spec) + ":lanes=%d:onelaunch" % lanes
        run_program(e, ins)
        for l in range(lanes):
            for r in OUT_REGS:
                assert e.get_int(r, lane=l) == want[l][r], (p, spec, lanes, "lane", l, "register", r)


# ---- factors above the fused bound, and an addend that is the destination ----------------------------------------------------

def test_factors_above_the_fused_bound():
    p, spec, lanes, a = oc.FACTOR_CASE
    mp = (1 << p) - 1
    x, y = values(p, lanes, 1), values(p, lanes, 2)
    x[0] = mp - 1
    with Engine(p, 6, plan=spec, lanes=lanes, onelaunch=True) as e:
        put(e, 0, x); put(e, 1, y)
        e.set_multiplicand(2, 1)
        e.square_mul(0, a)
        v = [mulmod(p, u, u, a) for u in x]
        check(e, 0, v, "square_mul, large factor")
        e.square_mul(0, a); e.mul(0, 2, a)                    # carries of the factor pass pending into the next product
        v = [mulmod(p, mulmod(p, u, u, a), w, a) for u, w in zip(v, y)]
        check(e, 0, v, "mul, large factor")
        e.square_mul_prepare(0, 3, a)
        e.mul(1, 3)
        check(e, 0, [mulmod(p, u, u, a) for u in v], "square_mul_prepare, large factor")
        check(e, 1, [mulmod(p, w, u) for u, w in zip(v, y)], "mul by the image it kept")


def test_mul_add_with_the_destination_as_addend():
    p, spec, lanes, _ = oc.FACTOR_CASE
    mp = (1 << p) - 1
    x, y = values(p, lanes, 3), values(p, lanes, 4)
    with Engine(p, 4, plan=spec, lanes=lanes, onelaunch=True) as e:
        put(e, 0, x); put(e, 1, y)
        e.set_multiplicand(2, 1)
        e.square_mul(0, 3)                                   # the addend's run carries are pending
        v = [mulmod(p, u, u, 3) for u in x]
        e.mul_add(0, 2, 0, 3)                                # 0 = 3 (0 y) + 0
        v = [(mulmod(p, u, w, 3) + u) % mp for u, w in zip(v, y)]
        check(e, 0, v, "mul_add, add_src == dst")
        e.mul_add(0, 2, 0)
        check(e, 0, [(mulmod(p, u, w) + u) % mp for u, w in zip(v, y)], "mul_add again")


# ---- the registers and images of the generic path ---------------------------------------------------------------------------

@pytest.mark.parametrize("p", [1277, 4253, 204799])
def test_registers_and_images_are_those_of_the_three_launch_path(p):
    x, y = values(p, 2, 5)
    with Engine(p, 4) as g, Engine(p, 4, onelaunch=True) as o:
        assert o.describe() == g.describe() + ":onelaunch"
        for e in (g, o):
            e.set_int(0, x); e.set_int(2, y)
            e.square_mul(0); e.square_mul(0, 3)
            e.set_multiplicand(1, 2)
            e.mul(0, 1)
        dg, do = g.get_data(0), o.get_data(0)
        assert np.array_equal(dg, do), (p, "digit register", int(np.count_nonzero(dg != do)), "bytes differ")
        ig, io = g.get_data(1), o.get_data(1)
        assert np.array_equal(ig[-8:], io[-8:]) and ig[-8] & 1 == 1 and dg[-8] & 1 == 0       # the tags
        wg, wo = ig[:-8].view("<u8"), io[:-8].view("<u8")
        red = lambda w: np.where(w >= np.uint64(FIELD), w - np.uint64(FIELD), w)
        assert np.array_equal(red(wg), red(wo)), (p, "image words", int(np.count_nonzero(red(wg) != red(wo))), "differ")
        # each engine's image on the other engine
        want = mulmod(p, g.get_int(0), y)
        assert g.set_data(3, io) and o.set_data(3, ig)
        g.mul(0, 3); o.mul(0, 3)
        assert g.get_int(0) == want and o.get_int(0) == want
        assert np.array_equal(g.get_data(0), o.get_data(0))
        with pytest.raises(Exception, match="onelaunch"):
            o.time_square_mul(0, 1)
        g.time_square_mul(0, 1)


# ---- lanes that share a work-group ----------------------------------------------------------------------------------------------

def test_a_write_to_one_lane_leaves_its_neighbours_in_the_group_alone():
    p, lanes = 1277, 9                                       # 8 lanes a group: lanes 0 .. 7 share one, lane 8 has a group to itself
    assert oc.shape(64, lanes)[:3] == (32, 8, 2)
    x, y = values(p, lanes, 6), values(p, lanes, 7)
    with Engine(p, 3, lanes=lanes, onelaunch=True) as e:
        put(e, 0, x)
        e.square_mul(0, 3)                                   # run carries pending on every lane
        v = [mulmod(p, u, u, 3) for u in x]
        for l in (3, 8):
            e.set_int(0, y[l], lane=l)
            v[l] = y[l]
        e.square_mul(0)
        v = [mulmod(p, u, u) for u in v]
        check(e, 0, v, "after a write to lanes 3 and 8")
        e.set_multiplicand(1, 0)
        e.set_int(0, y[0], lane=0)
        e.mul(0, 1)
        v = [mulmod(p, y[0] if l == 0 else u, u) for l, u in enumerate(v)]
        check(e, 0, v, "after a write to lane 0")


def test_the_lane_after_a_full_group_gets_its_own_result():
    for p, n in ((1277, 64), (127, 8)):
        k = oc.shape(n, 100)[1]
        lanes = k + 1
        assert oc.shape(n, lanes)[1:3] == (k, 2)
        x = values(p, lanes, 8)
        with Engine(p, 2, lanes=lanes, onelaunch=True) as e:
            put(e, 0, x)
            e.square_mul(0); e.square_mul(0, 5)
            check(e, 0, [mulmod(p, mulmod(p, u, u), mulmod(p, u, u), 5) for u in x], "B = K + 1")


# ---- two engines in one process ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", [(204799, 127), (127, 204799)], ids=["large-first", "small-first"])
def test_engines_of_the_largest_and_the_smallest_size_in_turn(order):
    engines = [Engine(p, 3, lanes=2, onelaunch=True) for p in order]
    try:
        state = {}
        for e in engines:
            state[e.p] = values(e.p, 2, 9)
            put(e, 0, state[e.p])
        for step in range(3):
            for e in engines:                                # in turn: each launch follows one of the other size
                e.square_mul(0, 1 + step)
                state[e.p] = [mulmod(e.p, u, u, 1 + step) for u in state[e.p]]
        for e in engines:
            check(e, 0, state[e.p], "engines in turn")
    finally:
        for e in engines:
            e.close()


# ---- ECM ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p, b1, b2, D, sigmas, bad, factor", BATCHES, ids=["%d-B1=%d" % (b[0], b[1]) for b in BATCHES])
def test_ecm_batches_give_every_lane_what_the_oracle_gives_that_sigma(p, b1, b2, D, sigmas, bad, factor):
    assert {(b[0], b[1], b[2], b[3], tuple(b[4])) for b in BATCHES} == {(1009, 50, 0, None, (69, 7, 3454817)), (3001, 30, 300, 30, (6, 8, 3217073, 36))}
    with Engine(p, ecm.registers_needed(D) if D else ecm.FIXED_REGISTERS, lanes=len(sigmas), onelaunch=True) as e:
        assert e.describe().endswith(":lanes=%d:onelaunch" % len(sigmas))
        out = ecm.run_lanes(e, p, b1, b2, sigmas, D)
    for l, sigma in enumerate(sigmas):
        ref, _ = _single(p, b1, b2, sigma, D)
        assert (out[l]["g1"], out[l]["g2"]) == (ref["g1"], ref["g2"]) and out[l]["factors"] == ref["factors"], (p, sigma)
    assert out[bad]["g1"] % factor == 0 and sum(bool(r["factors"]) for r in out) >= 2
