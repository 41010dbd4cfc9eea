"""The product across lanes (include/mi355_lanecross.h, Engine.mul_sibling) against Python integers on every lane, on the three-launch
path and on the one-launch path at thread shapes where lanes share a work-group and a wave; inside a batch; on engines with one lane;
its refusals; a sibling lane beyond 4 GiB; and ECM's affine stage 2 with inverse="engine" against the host inverse on the same engine
and the integer model of tests/test_ecm_affine.py.
Needs a real MI355X:  python -m pytest tests -m gpu"""
import random

import pytest

from prmers_amd import ecm, ecm_edwards, lanecross
from test_ecm_affine import m_run_affine

pytestmark = pytest.mark.gpu

DST, SRC, ALT, SRC_COPY, ALT_COPY, BY, BY_COPY, T1, T2 = range(9)
REGS = 9


def Engine(*a, **k):
    from prmers_amd import Engine as E
    return E(*a, **k)


def values(p, lanes, seed):
    rng = random.Random(104729 * p + seed)
    mp = (1 << p) - 1
    return [rng.getrandbits(p) % mp for _ in range(lanes)]


def image(e, reg, vals, by_squaring):
    """the image of vals in reg: by set_multiplicand, or as the by-product of square_mul_prepare on a scratch register"""
    if by_squaring:
        e.set_ints(T1, vals)
        e.square_mul_prepare(T1, reg)
    else:
        e.set_ints(reg, vals)
        e.set_multiplicand(reg, reg)


def expected(d, s, a, level, lanes, mp):
    g = [lanecross.sibling(l, level, lanes) for l in range(lanes)]
    return [d[l] * (a[l] if g[l] is None else s[g[l]]) % mp for l in range(lanes)]


def unchanged(e, s, a, by, mp):
    """src and alt still multiply like their copies and like the integers; the bystander is its copy"""
    w = values(e.p, e.lanes, 99)
    for reg, copy, vals in ((SRC, SRC_COPY, s), (ALT, ALT_COPY, a)):
        e.set_ints(T1, w); e.mul(T1, reg)
        e.set_ints(T2, w); e.mul(T2, copy)
        assert all(e.equal_lanes(T1, T2)) and e.get_ints(T1) == [x * y % mp for x, y in zip(w, vals)]
    assert all(e.equal_lanes(BY, BY_COPY)) and e.get_ints(BY) == by


# three launches at p = 3001; one launch at p = 1277 (n = 64: 32 threads a lane, 8 lanes a work-group, two lanes a wave) and at
# p = 127 (n = 8: 64 lanes a work-group)
SHAPES = [(3001, False), (1277, True), (127, True)]
LANES = [1, 2, 3, 5, 8, 13, 70]                       # 13: a tail group with dead lanes on both one-launch shapes


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("p, onelaunch", SHAPES, ids=["p3001-three", "p1277-one", "p127-one"])
def test_mul_sibling_is_the_rule_on_integers_at_every_level(p, onelaunch, lanes):
    mp = (1 << p) - 1
    L = lanecross.levels(lanes)
    by = values(p, lanes, 5)
    with Engine(p, REGS, lanes=lanes, onelaunch=onelaunch) as e:
        if onelaunch:
            n = e.n
            assert (p, n) in ((1277, 64), (127, 8))
        e.set_ints(BY, by); e.copy(BY_COPY, BY)
        for level in range(L + 2):                     # L + 1: above every lane, all take alt
            for variant in (0, 1):
                d, s = values(p, lanes, 10 * level + variant), values(p, lanes, 10 * level + variant + 2)
                # variant 0: dst with run carries pending (straight after a square_mul), src by set_multiplicand, alt the image of 1
                # variant 1: dst as written, src by square_mul_prepare, alt another value on every lane, so that a wrong choice shows
                a = [1] * lanes if variant == 0 else values(p, lanes, 10 * level + 4)
                image(e, SRC, s, by_squaring=variant == 1); e.copy(SRC_COPY, SRC)
                image(e, ALT, a, by_squaring=False); e.copy(ALT_COPY, ALT)
                e.set_ints(DST, d)
                if variant == 0:
                    e.square_mul(DST)
                    d = [x * x % mp for x in d]
                e.mul_sibling(DST, SRC, ALT, level)
                want = expected(d, s, a, level, lanes, mp)
                assert e.get_ints(DST) == want, (p, lanes, "level", level, "variant", variant)
                if level >= L:
                    assert want == [x * y % mp for x, y in zip(d, a)]
                unchanged(e, s, a, by, mp)
        # the result is a residue like any other: squared with its carries pending, and multiplied across again
        e.square_mul(DST)
        e.mul_sibling(DST, SRC, ALT, 0)
        assert e.get_ints(DST) == expected([x * x % mp for x in want], s, a, 0, lanes, mp)


@pytest.mark.parametrize("p, lanes", [(1277, 13), (127, 70)])
def test_inside_a_batch_the_queue_runs_first(p, lanes):
    mp = (1 << p) - 1
    d, s, a = values(p, lanes, 1), values(p, lanes, 2), values(p, lanes, 3)
    with Engine(p, REGS, lanes=lanes, onelaunch=True) as e:
        image(e, ALT, a, False)
        e.set_ints(DST, d); e.set_ints(T2, s)
        ops0, launches0 = e.batch_stats()[:2]
        with e.batch():
            e.square_mul(DST)
            e.set_multiplicand(SRC, T2)                # the image another work-group's lanes will read: queued, not stored yet
            assert e.batch_stats()[3] == 2 and e.batch_stats()[1] == launches0
            e.mul_sibling(DST, SRC, ALT, 1)
            assert e.batch_stats()[3] == 0 and e.batch_stats()[1] == launches0 + 1       # the queue ran; the product itself is no descriptor
            assert e.batch_stats()[0] == ops0 + 2
            e.square_mul(DST)
            e.mul_sibling(DST, SRC, ALT, 0)
            assert e.batch_stats()[1] == launches0 + 2
        d2 = [x * x % mp for x in d]
        w1 = expected(d2, s, a, 1, lanes, mp)
        assert e.get_ints(DST) == expected([x * x % mp for x in w1], s, a, 0, lanes, mp)
        # and the same calls one by one
        e.set_ints(T1, d)
        e.square_mul(T1); e.mul_sibling(T1, SRC, ALT, 1); e.square_mul(T1); e.mul_sibling(T1, SRC, ALT, 0)
        assert all(e.equal_lanes(T1, DST))


def test_with_one_lane_it_is_mul_by_alt_on_both_families():
    from prmers_amd import CrtEngine
    p = 9941
    mp = (1 << p) - 1
    d, s, a = (values(p, 1, k)[0] for k in (1, 2, 3))
    for make in (lambda: Engine(p, 5), lambda: Engine(p, 5, onelaunch=True), lambda: CrtEngine(p, 9, reg_count=5)):
        with make() as e:
            assert e.lanes == 1
            e.set_int(1, s); e.set_multiplicand(1, 1)
            e.set_int(2, a); e.set_multiplicand(2, 2)
            for level in (0, 1, 31):
                e.set_int(0, d); e.square_mul(0); e.copy(3, 0)
                e.mul_sibling(0, 1, 2, level)
                e.mul(3, 2)
                assert e.is_equal(0, 3) and e.get_int(0) == d * d * a % mp, (e.describe(), level)
            for bad in ((1, 1, 2, 0), (0, 3, 2, 0), (0, 1, 3, 0), (0, 0, 2, 0), (0, 1, 2, 32), (5, 1, 2, 0)):
                with pytest.raises(Exception, match="mul_sibling"):
                    e.mul_sibling(*bad)
            assert e.get_int(0) == d * d * a % mp


@pytest.mark.parametrize("onelaunch", [False, True], ids=["three", "one"])
def test_refusals_come_with_a_message_and_change_nothing(onelaunch):
    from prmers_amd import EngineError
    from prmers_amd.engine import load_library
    p, lanes = 1277, 3
    mp = (1 << p) - 1
    d, s, a, r = (values(p, lanes, k) for k in (1, 2, 3, 4))
    lib = load_library()
    with Engine(p, 5, lanes=lanes, onelaunch=onelaunch) as e:
        e.set_ints(0, d); e.square_mul(0)
        e.set_ints(1, s); e.set_multiplicand(1, 1)
        e.set_ints(2, a); e.set_multiplicand(2, 2)
        e.set_ints(3, r)
        cases = [((1, 1, 2, 0), "dst must differ"), ((0, 0, 2, 0), "dst must differ"), ((0, 1, 0, 0), "dst must differ"),
                 ((4, 1, 2, 0), None), ((0, 3, 2, 0), "not a multiplicand"), ((0, 1, 3, 0), "not a multiplicand"), ((0, 1, 2, 32), "level"),
                 ((5, 1, 2, 0), "out of range"), ((0, 5, 2, 0), "out of range"), ((0, 1, 5, 0), "out of range"), ((0, 1, 2, 2**31), "level")]
        e.set_multiplicand(4, 3)                       # register 4 holds an image: refused as dst
        cases[3] = ((4, 1, 2, 0), "holds a multiplicand image")
        for args, text in cases:
            assert lib.mi355_lanecross_mul_sibling(e.h, *args) == 0
            message = lib.mi355_engine_last_error().decode()
            assert message.startswith("mul_sibling") and text in message, (args, message)
            with pytest.raises(EngineError, match="mul_sibling"):
                e.mul_sibling(*args)
        with pytest.raises(ValueError):
            e.mul_sibling(0, 1, 2, 2**32)              # not a uint32_t: refused before the call
        # nothing changed: dst with its pending carries, both images, the bystander
        assert e.get_ints(0) == [x * x % mp for x in d] and e.get_ints(3) == r
        e.mul(3, 1); assert e.get_ints(3) == [x * y % mp for x, y in zip(r, s)]
        e.mul(3, 2); e.mul(3, 4)
        assert e.get_ints(3) == [x * y % mp * z % mp * x % mp for x, y, z in zip(r, s, a)]
        e.mul_sibling(0, 1, 2, 0)                      # and the engine goes on
        assert e.get_ints(0) == expected([x * x % mp for x in d], s, a, 0, lanes, mp)


def test_a_sibling_lane_four_gibibytes_away():
    """p = 9815459: a lane is 8 n = 4 MiB, so lane 1024 of 1025 starts 2^32 bytes into a slot.  At level 10 lanes 0 and 1 take lane 1024's
    image and lane 1024 takes lane 0's: a sibling offset kept in 32 bits would hand lanes 0 and 1 lane 0's image."""
    from lane_program import mulmod
    from test_gpu_lanes_wide import free_device_memory
    p, lanes = 9815459, 1025
    free = free_device_memory()
    if free < 20 << 30:
        pytest.skip("%.1f GiB of device memory free, the engine of this test takes 16 GiB: needs 20 GiB" % (free / 2**30))
    d, common, alt = values(p, 3, 30)
    own = dict(zip((0, 1, 1024), values(p, 3, 31)))
    with Engine(p, 3, lanes=lanes) as e:
        assert e.n * 8 * 1024 == 1 << 32 and lanecross.levels(lanes) == 11
        e.set_int(0, d)
        e.set_int(1, common)
        for l, v in own.items():
            e.set_int(1, v, lane=l)
        e.set_multiplicand(1, 1)
        e.set_int(2, alt); e.set_multiplicand(2, 2)
        e.mul_sibling(0, 1, 2, 10)
        for l, partner in ((0, 1024), (1024, 0), (1, 1024)):
            assert lanecross.sibling(l, 10, lanes) == partner
            assert e.get_int(0, lane=l) == mulmod(p, d, own[partner]), ("lane", l)


# ---- ECM with the engine inverse ----

ECM_CASES = [
    # (p, b1, b2, D, sigmas, onelaunch, batch, fallback blocks)
    (3001, 30, 300, 30, [6, 8], False, False, 0),
    (1009, 20, 104, 210, [7, 12, 8], True, True, 1),            # the k = 0 factor: the baby block's product has no inverse
    (10007, 20, 500, 210, [10, 11], True, True, 0),             # giant blocks
    (1277, 30, 300, 30, list(range(6, 19)), True, True, 0),     # 13 lanes: four levels, a tail group
]


@pytest.mark.parametrize("p, b1, b2, D, sigmas, onelaunch, batch, fallbacks", ECM_CASES, ids=["p3001", "p1009-k0", "p10007", "p1277-13"])
def test_ecm_with_the_engine_inverse_is_the_host_inverse_and_the_model(p, b1, b2, D, sigmas, onelaunch, batch, fallbacks):
    mp = (1 << p) - 1
    B = len(sigmas)
    want = [m_run_affine(s, b1, b2, D, mp) for s in sigmas]
    drivers = [ecm] + ([ecm_edwards] if p == 10007 else [])
    with Engine(p, ecm.registers_needed(D, "affine", lanes=B, inverse="engine"), lanes=B, onelaunch=onelaunch) as e:
        for driver in drivers:
            out = driver.run_lanes(e, p, b1, b2, sigmas, D, batch=batch, stage2="affine", inverse="engine")
            acc = e.get_ints(ecm.R_A)
            host = driver.run_lanes(e, p, b1, b2, sigmas, D, batch=batch, stage2="affine")
            acc_host = e.get_ints(ecm.R_A)
            for res in (out, host):
                assert [(r["g1"], r["g2"]) for r in res] == [w[:2] for w in want]
                assert [r["factors"] for r in res] == [[f for f in w[:2] if 1 < f < mp] for w in want]
                assert all(r["normalised"] == want[0][4] for r in res)
            assert acc == acc_host == [w[2] for w in want]
            assert all(r["inverse"] == "engine" and r["inverse_fallbacks"] == fallbacks for r in out) and "inverse" not in host[0]
            assert ("launches" in out[0]) == batch
    if fallbacks:
        assert out[1]["factors"] == [3454817]
