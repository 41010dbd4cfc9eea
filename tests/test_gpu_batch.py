"""Batches (include/mi355_batch.h; kernels.hip k_batch): a run of register operations of a one-launch engine as one launch.  The lane
program on every lane of every case of batch_cases.py inside a batch, registers and images against the same calls issued one by one bit
for bit, one launch for a ladder step, a queue that overflows, the refusals, ECM batches against the CPU oracle, and a batched engine
next to a plain one.  test_batch_cases.py says what the cases pin.  Needs a real MI355X:  python -m pytest tests -m gpu"""
import random

import numpy as np
import pytest

import batch_cases as bc
import onelaunch_cases as oc
from lane_program import OUT_REGS, REGS, expected_of, inputs, mulmod, powmod, run_program
from prmers_amd import ecm
from test_lanes_host import BATCHES, _single

pytestmark = pytest.mark.gpu

SWITCHES = ("MI355_KERNELS", "MI355_TUNE", "MI355_HOST_CARRY")
FIELD = 2**64 - 2**32 + 1


def Engine(*a, **k):
    from prmers_amd import Engine as E
    return E(*a, **k)


def EngineError():
    from prmers_amd.engine import EngineError as X
    return X


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def values(p, count, seed):
    rng = random.Random(7919 * p + seed)
    mp = (1 << p) - 1
    return [rng.getrandbits(p) % mp for _ in range(count)]


def put(e, r, vs):
    e.set(r, 0)
    for l, v in enumerate(vs):
        e.set_int(r, v, lane=l)


def check(e, r, want, what):
    for l in range(e.lanes):
        assert e.get_int(r, lane=l) == want[l], (e.p, what, "lane", l, "of", e.lanes, "register", r)


class Counting:
    """an engine whose register operations are counted on their way through"""

    def __init__(self, e):
        self.e, self.calls = e, 0

    def __getattr__(self, name):
        f = getattr(self.e, name)
        if not callable(f) or name in ("square_mul_prepare_is_fused", "mul_sum_is_fused"):
            return f

        def counted(*a, **k):
            self.calls += 1
            return f(*a, **k)
        return counted


def ladder_step(e, a=(ecm.R_XA, ecm.R_ZA), b=(ecm.R_XB, ecm.R_ZB)):
    ecm._Curve(ecm._Ops(e)).ladder_step(a, b)


def seed_ladder(e, p, seed):
    """full-size values in the ladder's registers, a24 and x0 as images"""
    vs = values(p, 6, seed)
    for r, v in zip((ecm.R_A24, ecm.R_X0, ecm.R_XA, ecm.R_ZA, ecm.R_XB, ecm.R_ZB), vs):
        e.set_int(r, v)
    e.set_multiplicand(ecm.R_A24, ecm.R_A24); e.set_multiplicand(ecm.R_X0, ecm.R_X0)


# ---- 1. the program on every lane of every case, inside a batch --------------------------------------------------------------------

@pytest.mark.parametrize("p, spec, lanes", bc.CASES, ids=[bc.case_id(c) for c in bc.CASES])
def test_program_on_every_lane_inside_a_batch(p, spec, lanes):
    ins = inputs(p, lanes=lanes)
    want = expected_of(p, ins)
    with Engine(p, REGS, plan=spec, lanes=lanes, onelaunch=True) as e:
        before = e.batch_stats()
        with e.batch():
            run_program(e, ins)          # its sub, its per-lane writes and its factor 3 ... flush in the middle of the batch
        after = e.batch_stats()
        assert after[0] > before[0] and after[1] > before[1] + 1 and after[3] == 0
        for l in range(lanes):
            for r in OUT_REGS:
                assert e.get_int(r, lane=l) == want[l][r], (p, spec, lanes, "lane", l, "register", r)


# ---- 2. bit for bit the registers of the calls issued one by one -----------------------------------------------------------------

@pytest.mark.parametrize("p", bc.BIT_FOR_BIT_EXPONENTS)
def test_registers_and_images_are_those_of_the_calls_issued_one_by_one(p):
    red = lambda w: np.where(w >= np.uint64(FIELD), w - np.uint64(FIELD), w)
    R_IMG, R_E, R_F = ecm.R_IT, ecm.R_XQ, ecm.R_ZQ
    with Engine(p, ecm.FIXED_REGISTERS, onelaunch=True) as one, Engine(p, ecm.FIXED_REGISTERS, onelaunch=True) as two, \
            Engine(p, ecm.FIXED_REGISTERS, onelaunch=True) as bat:
        def sequence(e):
            ladder_step(e)
            d = ecm.R_XA
            e.mul_add(d, R_IMG, d); e.mul_add(d, R_IMG, d)                       # the addend is the destination, twice in a row
            e.addsub_copy(ecm.R_S, ecm.R_D, R_E, R_F, ecm.R_XA, ecm.R_XB)
        for e in (one, two, bat):
            seed_ladder(e, p, 1)
        sequence(one); sequence(two)
        with bat.batch():
            sequence(bat)
        kinds = []
        for r in range(ecm.FIXED_REGISTERS):
            a, b, c = one.get_data(r), two.get_data(r), bat.get_data(r)
            assert np.array_equal(a[-8:], b[-8:]) and np.array_equal(a[-8:], c[-8:]), (p, "tag of register", r)
            image = bool(a[-8] & 1)
            kinds.append(image)
            if not image:
                assert np.array_equal(a, b), (p, "the two plain engines differ in digit register", r)
                assert np.array_equal(a, c), (p, "digit register", r, int(np.count_nonzero(a != c)), "bytes differ")
            else:
                wa, wb, wc = (x[:-8].view("<u8") for x in (a, b, c))
                assert np.array_equal(red(wa), red(wb)) and np.array_equal(red(wa), red(wc)), (p, "image", r, int(np.count_nonzero(red(wa) != red(wc))), "words differ")
        assert sum(kinds) >= 6 and kinds[R_IMG] and not kinds[ecm.R_XA]           # a24, x0, s, d, dd, dd + a24 t
        assert one.get_int(ecm.R_XA) == bat.get_int(ecm.R_XA) and one.get_int(R_F) == bat.get_int(R_F)


# ---- 3. a ladder step is one launch -----------------------------------------------------------------------------------------------

def test_a_ladder_step_inside_a_batch_is_one_launch():
    p = 1277
    with Engine(p, ecm.FIXED_REGISTERS, lanes=9, onelaunch=True) as e, Engine(p, ecm.FIXED_REGISTERS, lanes=9, onelaunch=True) as ref:
        for x in (e, ref):
            seed_ladder(x, p, 2)
        c = Counting(e)
        q0, l0, cap, pend = e.batch_stats()
        assert pend == 0 and cap >= 32
        with e.batch():
            ladder_step(c)
            assert e.batch_stats() == (q0 + c.calls, l0, cap, c.calls)          # queued, nothing launched yet
        assert 20 <= c.calls <= cap
        assert e.batch_stats() == (q0 + c.calls, l0 + 1, cap, 0)
        ladder_step(ref)
        for r in (ecm.R_XA, ecm.R_ZA, ecm.R_XB, ecm.R_ZB):
            check(e, r, [ref.get_int(r, lane=l) for l in range(9)], "ladder step")
        ladder_step(c)                                                           # outside a batch nothing is queued
        assert e.batch_stats() == (q0 + c.calls // 2, l0 + 1, cap, 0)


# ---- 4. more operations than the queue holds -----------------------------------------------------------------------------------------

def test_a_full_queue_flushes_by_itself_and_goes_on():
    p = bc.CAPACITY_EXPONENT
    with Engine(p, 2, lanes=3, onelaunch=True) as e:
        x = [3, 5, (1 << p) - 2]
        put(e, 0, x)
        q0, l0, cap, _ = e.batch_stats()
        with e.batch():
            for _ in range(cap + 3):
                e.square_mul(0)
            assert e.batch_stats() == (q0 + cap + 3, l0 + 1, cap, 3)
        assert e.batch_stats() == (q0 + cap + 3, l0 + 2, cap, 0)
        check(e, 0, [powmod(p, v, 1 << (cap + 3)) for v in x], "capacity + 3 squarings")
        with e.batch():                                                          # the engine's own loops are queued too
            e.square_mul_n(0, cap + 3)
            e.square_mul_bits(0, 3, bytes([0b10100000]), 3)
        assert e.batch_stats() == (q0 + 2 * cap + 9, l0 + 4, cap, 0)
        want = [powmod(p, v, 1 << (2 * cap + 6)) for v in x]
        want = [mulmod(p, powmod(p, v, 8), powmod(p, 3, 0b101)) for v in want]
        check(e, 0, want, "square_mul_n and square_mul_bits")


# ---- 5. what is refused ------------------------------------------------------------------------------------------------------------------

def test_refusals_name_the_batch():
    p = 1277
    with Engine(p, 2) as plain:
        with pytest.raises(EngineError(), match="batch"):
            with plain.batch():
                pass
        with pytest.raises(EngineError(), match="batch.*onelaunch"):
            plain._ok(plain.L.mi355_batch_begin(plain.h))
        assert plain.batch_stats()[:2] == (0, 0)
    from prmers_amd import CrtEngine
    with CrtEngine(9941, 9) as crt:
        with pytest.raises(EngineError(), match="batch.*crt"):
            with crt.batch():
                pass
    with Engine(p, 4, onelaunch=True) as e:
        with pytest.raises(EngineError(), match="batch_end"):
            e._ok(e.L.mi355_batch_end(e.h))
        with e.batch():
            with pytest.raises(EngineError(), match="batch_begin.*already"):
                with e.batch():
                    pass
            e.square_mul(0)
            assert e.batch_stats()[3] == 1                                       # the refused batch_begin left the open batch as it was
        assert e.batch_stats()[3] == 0
        with pytest.raises(EngineError(), match="batch_end"):                    # and its batch_end has closed it
            e._ok(e.L.mi355_batch_end(e.h))


def test_a_refused_call_inside_a_batch_raises_there_and_what_was_queued_still_runs():
    p = 1277
    x, y = values(p, 2, 3)
    with Engine(p, 4, onelaunch=True) as e:
        e.set_int(0, x); e.set_int(1, y)
        q0, l0, _, _ = e.batch_stats()
        with pytest.raises(EngineError(), match="not a multiplicand"):
            with e.batch():
                e.square_mul(0, 3)
                e.copy(2, 0)
                e.mul(0, 1)                   # register 1 holds no image
        assert e.batch_stats()[:2] == (q0 + 2, l0 + 1) and e.batch_stats()[3] == 0
        v = mulmod(p, x, x, 3)
        assert e.get_int(0) == v and e.get_int(2) == v and e.get_int(1) == y
        with e.batch():
            e.set_multiplicand(1, 1)
            with pytest.raises(EngineError(), match="range"):
                e.copy(9, 0)
            e.mul(0, 1)
        assert e.get_int(0) == mulmod(p, v, y)


# ---- 6. ECM -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p, b1, b2, D, sigmas, bad, factor", BATCHES, ids=["%d-B1=%d" % (b[0], b[1]) for b in BATCHES])
def test_ecm_in_batches_gives_every_lane_what_the_oracle_gives_that_sigma(p, b1, b2, D, sigmas, bad, factor):
    regs = ecm.registers_needed(D) if D else ecm.FIXED_REGISTERS
    with Engine(p, regs, lanes=len(sigmas), onelaunch=True) as e:
        out = ecm.run_lanes(e, p, b1, b2, sigmas, D, batch=True)
        launches = e.batch_stats()[1]
    with Engine(p, regs, lanes=len(sigmas), onelaunch=True) as e:
        plain = ecm.run_lanes(e, p, b1, b2, sigmas, D)
        assert e.batch_stats()[:2] == (0, 0)
    for l, sigma in enumerate(sigmas):
        ref, _ = _single(p, b1, b2, sigma, D)
        assert (out[l]["g1"], out[l]["g2"]) == (ref["g1"], ref["g2"]) and out[l]["factors"] == ref["factors"], (p, sigma)
        assert (out[l]["squarings"], out[l]["products"], out[l]["prepares"]) == (plain[l]["squarings"], plain[l]["products"], plain[l]["prepares"])
        assert out[l]["launches"] == launches and "launches" not in plain[l]
    assert out[bad]["g1"] % factor == 0 and sum(bool(r["factors"]) for r in out) >= 2
    total = out[0]["squarings"] + out[0]["products"] + out[0]["prepares"]
    assert 1 <= launches < total // 8                                            # far fewer launches than products


# ---- 7. a batched engine next to a plain one of another size ----------------------------------------------------------------------

@pytest.mark.parametrize("order", bc.NEIGHBOURS, ids=["batched-large", "batched-small"])
def test_a_batched_engine_and_a_plain_engine_of_another_size_in_turn(order):
    for first in (0, 1):                                                         # both orders of use
        engines = [Engine(order[0], 3, lanes=2, onelaunch=True), Engine(order[1], 3, lanes=2)]
        try:
            state = {}
            for e in engines:
                state[e.p] = values(e.p, 2, 4 + first)
                put(e, 0, state[e.p])
            bat = engines[0]
            for step in range(3):
                for e in (engines if first == 0 else engines[::-1]):
                    if e is bat:
                        with e.batch():
                            e.square_mul(0, 1 + step); e.copy(1, 0); e.add(0, 1)
                        state[e.p] = [2 * mulmod(e.p, u, u, 1 + step) % ((1 << e.p) - 1) for u in state[e.p]]
                    else:
                        e.square_mul(0, 1 + step)
                        state[e.p] = [mulmod(e.p, u, u, 1 + step) for u in state[e.p]]
            for e in engines:
                check(e, 0, state[e.p], "engines in turn")
        finally:
            for e in engines:
                e.close()
