"""Every back sweep at its fused factor bound (plan.hpp fused_factor_limit -> a_fast), on operands with every digit at its maximum,
against Python integers mod 2^p - 1 (never the oracle, which restates the same 64-bit carry).  The cases, operands and sequences are
those of factor_bound_cases.py; test_factor_bound_cases.py has run every one of them through the exact chain (chain_model.py) and found
every term inside its word, so a wrong value here is a kernel's fault.  Per case: every entry that takes a factor at a_fast - 1, a_fast
and a_fast + 1 (the last one leaves the fused path: factor 1 plus k_scale), each followed by two squarings and a mul that consume the
large carry words it leaves pending, with nothing read in between; chains of six at a_fast; on one-launch engines the same inside a
batch, and with one lane the registers bit for bit.  Needs a real MI355X:  python -m pytest tests -m gpu"""
import numpy as np
import pytest

import factor_bound_cases as fc

pytestmark = pytest.mark.gpu

SWITCHES = ("MI355_KERNELS", "MI355_TUNE", "MI355_HOST_CARRY")
FIELD = 2**64 - 2**32 + 1
IDS = [fc.case_id(c) for c in fc.CASES]


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


def make(c, monkeypatch, lanes=None):
    if c.kernels:
        monkeypatch.setenv("MI355_KERNELS", c.kernels)
    e = Engine(c.p, fc.REGS, plan=c.spec, lanes=c.lanes if lanes is None else lanes, onelaunch=c.onelaunch)
    assert e.n == c.n and e.lanes == (c.lanes if lanes is None else lanes)
    return e


def put(e, r, values):
    """values in [0, 2^p - 1] as words, one per lane: 2^p - 1 is the all-ones register (set_int would reduce it to 0)"""
    if e.lanes > 1:
        e.set(r, 0)
    for l, v in enumerate(values):
        w = np.frombuffer(v.to_bytes(e.word_count * 4, "little"), dtype="<u4")
        e.set_words(r, w, None if e.lanes == 1 else l)


def read(e, r):
    return e.get_ints(r) if e.lanes > 1 else [e.get_int(r)]


def load(e, lanes):
    """x, y (and its image) and the addend of every lane; the other registers zero"""
    for r in (fc.R_COPY, fc.R_PREP):
        e.set(r, 0)
    put(e, fc.R_X, [x for _, x, _, _ in lanes])
    put(e, fc.R_Y, [y for _, _, y, _ in lanes])
    put(e, fc.R_ADD, [z for _, _, _, z in lanes])
    e.set_multiplicand(fc.R_YIMG, fc.R_Y)


def expected(c, lanes, ops):
    mp = (1 << c.p) - 1
    return [fc.run_ints(c.p, {fc.R_X: x % mp, fc.R_YIMG: y % mp, fc.R_ADD: z % mp}, ops) for _, x, y, z in lanes]


def check(e, c, lanes, want, regs, what):
    for r in regs:
        got = read(e, r)
        for l in range(len(lanes)):
            assert got[l] == want[l][r], (fc.case_id(c), what, "lane", l, fc.KINDS[lanes[l][0]], "register", r)


@pytest.mark.parametrize("c", fc.CASES, ids=IDS)
def test_every_entry_at_the_bound(c, monkeypatch):
    with make(c, monkeypatch) as e:
        for lanes in fc.rounds(c):
            for a in fc.factors(c):
                for entry in fc.ENTRIES:
                    ops, what = fc.sequence(entry, a), (entry, a - c.a_fast)
                    if fc.refused(c, entry, a):                    # mul_add onto itself above the bound: refused, nothing changed
                        load(e, lanes)
                        with pytest.raises(EngineError(), match="fused"):
                            fc.run_engine(e, ops[:1])
                        mp = (1 << c.p) - 1
                        assert read(e, fc.R_X) == [x % mp for _, x, _, _ in lanes], (fc.case_id(c), what, "changed by a refused call")
                        continue
                    want = expected(c, lanes, ops)
                    load(e, lanes)
                    fc.run_engine(e, ops)
                    check(e, c, lanes, want, fc.outputs(entry), what)
                    if c.onelaunch:
                        load(e, lanes)
                        before = e.batch_stats()
                        with e.batch():
                            fc.run_engine(e, ops)
                        after = e.batch_stats()
                        assert after[0] >= before[0] + len(fc.FOLLOW) and after[1] > before[1] and after[3] == 0, (fc.case_id(c), what)
                        check(e, c, lanes, want, fc.outputs(entry), what + ("batch",))


@pytest.mark.parametrize("c", fc.CASES, ids=IDS)
def test_chains_at_the_bound(c, monkeypatch):
    """six products at a_fast in a row, each on the pending carry words of the one before, read once at the end"""
    lanes = fc.rounds(c)[0]                                         # lane 0: 2^p - 2
    with make(c, monkeypatch) as e:
        for onto_itself in (False, True):
            if onto_itself and not fc.fused_back(c):
                continue
            ops = fc.chain_ops(c, onto_itself)
            want = expected(c, lanes, ops)
            for batch in ((False, True) if c.onelaunch else (False,)):
                load(e, lanes)
                if batch:
                    queued = e.batch_stats()[0]
                    with e.batch():
                        fc.run_engine(e, ops)
                    assert e.batch_stats()[0] == queued + len(ops)
                else:
                    fc.run_engine(e, ops)
                check(e, c, lanes, want, (fc.R_X,), ("chain", onto_itself, batch))


@pytest.mark.parametrize("c", fc.ONELAUNCH, ids=[fc.case_id(c) for c in fc.ONELAUNCH])
def test_one_lane_in_a_batch_is_bit_for_bit_the_calls_issued_one_by_one(c, monkeypatch):
    red = lambda w: np.where(w >= np.uint64(FIELD), w - np.uint64(FIELD), w)
    lanes = fc.rounds(c)[0][:1]
    with make(c, monkeypatch, lanes=1) as one, make(c, monkeypatch, lanes=1) as bat:
        for a in fc.factors(c):
            for entry in fc.ENTRIES:
                if fc.refused(c, entry, a):
                    continue
                ops = fc.sequence(entry, a)
                load(one, lanes); load(bat, lanes)
                fc.run_engine(one, ops)
                with bat.batch():
                    fc.run_engine(bat, ops)
                for r in range(fc.REGS):
                    x, y = one.get_data(r), bat.get_data(r)
                    assert np.array_equal(x[-8:], y[-8:]), (fc.case_id(c), entry, a, "tag of register", r)
                    if x[-8] & 1:
                        assert np.array_equal(red(x[:-8].view("<u8")), red(y[:-8].view("<u8"))), (fc.case_id(c), entry, a, "image", r)
                    else:
                        assert np.array_equal(x, y), (fc.case_id(c), entry, a, "digit register", r)
