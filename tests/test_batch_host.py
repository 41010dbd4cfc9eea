"""Host side of the ECM driver's batches (no GPU): ecm.run(..., batch=True) on a stand-in that records batch_begin / batch_end and every
read-back around the CPU engine test_ecm.py and test_lanes_host.py use -- results identical to batch=False, every batch closed, nothing
read back inside an open one -- and ecm.ecm's refusal of batch without onelaunch before any engine is made."""
import contextlib

import pytest

import orc
from prmers_amd import ecm
from prmers_amd import engine as E
from test_lanes_host import LaneOracles

CASES = [(1009, 50, 0, None, 69), (3001, 30, 300, 30, 6), (3001, 30, 300, 30, 8)]      # stage 1 alone (finds 3454817), stages 1 and 2


class Recording:
    """orc.OracleEngine with Engine.batch() / batch_stats(): a batch here only counts; what it opens, closes and sees is recorded"""

    def __init__(self, p, reg_count):
        self.o = orc.OracleEngine(p, reg_count)
        self.p, self.n, self.reg_count = p, self.o.n, reg_count
        self.depth = self.begun = self.ended = self.queued = self.launches = 0
        self.pending = 0
        self.reads_inside = []
        self.writes_inside = 0

    def close(self): self.o.close()
    def __enter__(self): return self
    def __exit__(self, *a): self.close()

    @contextlib.contextmanager
    def batch(self):
        assert self.depth == 0, "a second batch_begin"
        self.depth += 1; self.begun += 1
        try:
            yield self
        finally:
            self.depth -= 1; self.ended += 1
            self._flush()

    def batch_stats(self):
        return (self.queued, self.launches, 256, self.pending)

    def _flush(self):
        if self.pending:
            self.launches += 1
            self.pending = 0

    def _queued(self, name, *a):
        if self.depth:
            self.queued += 1; self.pending += 1
        return getattr(self.o, name)(*a)

    def _flushing(self, name, *a):
        if self.depth:
            self.writes_inside += 1
        self._flush()
        return getattr(self.o, name)(*a)

    def copy(self, dst, src): self._queued("copy", dst, src)
    def square_mul(self, src, a=1): self._queued("square_mul", src, a)
    def set_multiplicand(self, dst, src): self._queued("set_multiplicand", dst, src)
    def mul(self, dst, src, a=1): self._queued("mul", dst, src, a)
    def add(self, dst, src): self._queued("add", dst, src)
    def sub_reg(self, dst, src): self._queued("sub_reg", dst, src)
    def set(self, dst, a): self._flushing("set", dst, a)
    def set_int(self, dst, v): self._flushing("set_int", dst, v)

    def get_int(self, src):
        if self.depth:
            self.reads_inside.append(src)
        self._flush()
        return self.o.get_int(src)


def _regs(D):
    return ecm.registers_needed(D) if D else ecm.FIXED_REGISTERS


@pytest.mark.parametrize("p, b1, b2, D, sigma", CASES, ids=["%d-B1=%d-B2=%d-sigma%d" % (c[0], c[1], c[2], c[4]) for c in CASES])
def test_run_with_batches_gives_the_results_of_run_without(p, b1, b2, D, sigma):
    with Recording(p, _regs(D)) as plain, Recording(p, _regs(D)) as batched:
        want = ecm.run(plain, p, b1, b2, sigma, D)
        got = ecm.run(batched, p, b1, b2, sigma, D, batch=True)
        point = [(e.get_int(ecm.R_XQ), e.get_int(ecm.R_ZQ)) for e in (plain, batched)]
        assert (plain.begun, plain.queued, plain.launches) == (0, 0, 0) and "launches" not in want
        # identical but for the launches, which only a batched run reports
        assert got.pop("launches") == batched.launches >= 1
        assert got == want and point[0] == point[1]
        assert want["squarings"] > 0 and (want["factors"] or b2)
        # every batch_begin is closed, and there is one batch per stage that ran
        stage2 = b2 > b1 and want["g1"] != (1 << p) - 1
        assert batched.begun == batched.ended == (2 if stage2 else 1) and batched.depth == 0 and batched.pending == 0
        assert batched.reads_inside == []                       # Z, the accumulator: read after their batch has ended
        assert batched.queued >= want["squarings"] + want["products"] + want["prepares"]
        assert batched.writes_inside == (3 if stage2 and min(ecm.stage2_pairs(b1, b2, D)) == 0 else 1 if stage2 else 0)   # constants of stage 2: they flush


def test_a_batch_is_closed_when_the_ladder_raises():
    p = 1009

    class Failing(Recording):
        def mul(self, dst, src, a=1):
            if self.queued > 40:
                raise RuntimeError("refused")
            Recording.mul(self, dst, src, a)
    with Failing(p, ecm.FIXED_REGISTERS) as eng:
        with pytest.raises(RuntimeError, match="refused"):
            ecm.run(eng, p, 50, 0, 69, batch=True)
        assert eng.begun == eng.ended == 1 and eng.depth == 0


def test_on_an_object_without_batches_the_driver_runs_as_before():
    p, b1, sigma = 1009, 50, 69
    with orc.OracleEngine(p, ecm.FIXED_REGISTERS) as a, orc.OracleEngine(p, ecm.FIXED_REGISTERS) as b:
        assert not hasattr(a, "batch")
        want, got = ecm.run(a, p, b1, 0, sigma), ecm.run(b, p, b1, 0, sigma, batch=True)
    assert got == want and "launches" not in got
    with LaneOracles(p, ecm.FIXED_REGISTERS, lanes=2) as eng:
        out = ecm.run_lanes(eng, p, b1, 0, [sigma, 7], batch=True)
    assert all("launches" not in r for r in out) and out[0]["factors"] == want["factors"]


def test_ecm_refuses_batch_without_onelaunch_before_any_engine_is_made(monkeypatch):
    monkeypatch.setattr(E, "Engine", LaneOracles)
    LaneOracles.made = []
    for lanes in (1, 3):
        with pytest.raises(ValueError, match="onelaunch"):
            ecm.ecm(1009, 20, 0, sigma=7, lanes=lanes, batch=True)
        with pytest.raises(ValueError, match="onelaunch"):
            ecm.ecm(1009, 20, 0, sigma=7, lanes=lanes, plan="m2=4", batch=True)
    assert LaneOracles.made == []
    res = ecm.ecm(1009, 20, 0, sigma=7, lanes=3, onelaunch=True, batch=True)          # the stand-in has no batches: as without
    assert len(LaneOracles.made) == 1 and "launches" not in res


def test_the_command_line_passes_the_option(monkeypatch):
    seen = {}

    def fake(*a, **k):
        seen["args"], seen["kw"] = a, k
        return {"factors": [1]}
    monkeypatch.setattr(ecm, "ecm", fake)
    assert ecm.main(["1009", "50", "--onelaunch", "--batch"]) == 0 and seen["args"][-1] is True and seen["kw"] == {"batch": True}
    assert ecm.main(["1009", "50", "--onelaunch"]) == 0 and seen["kw"] == {}
    monkeypatch.undo()
    with pytest.raises(ValueError, match="onelaunch"):
        ecm.main(["1009", "50", "--batch"])
