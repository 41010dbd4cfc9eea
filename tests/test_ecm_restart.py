"""ECM that stops and goes on (no GPU): stage-1 checkpoints of prmers_amd/ecm.py and ecm_edwards.py, the resume lines they save and the
stage 2 that starts from them, on the CPU oracle and the stand-ins of the other ECM tests (one oracle a lane, batches that only count).
A run that is stopped anywhere and resumed on a fresh engine object must end in the canonical residues and the results of the run that
was never stopped: the arithmetic is exact modulo 2^p - 1, so nothing less than equality is asked."""
import contextlib
import json
import os

import pytest

import orc
from prmers_amd import ecm, ecm_files, ecm_edwards as ed
from prmers_amd import engine as E
from test_batch_host import Recording
from test_lanecross_host import CrossOracles
from test_lanes_host import LaneOracles

# sigma 6 finds 3217073 in stage 2 and nothing in stage 1, 8 and 7 find nothing (tests/test_ecm.py, tests/test_ecm_affine.py)
P, B1, B2, D = 3001, 30, 300, 30
SIGMAS = [6, 8, 7]
STEPS = ecm.stage1_exponent(B1).bit_length() - 1          # ladder steps; the NAF has one digit more or as many
EVERY = 8
CHECK_EVERY = 4
COUNTS = ("squarings", "products", "prepares")
FORMS = {"montgomery": (ecm, {}, (ecm.R_XQ, ecm.R_ZQ)), "edwards": (ed, {"check_every": CHECK_EVERY}, ed.POINT)}


class LaneRecording(LaneOracles):
    """LaneOracles with batch() / batch_stats() that only count, and a record of what is read while a batch is open"""

    def __init__(self, p, reg_count, device=0, plan=None, lanes=1):
        LaneOracles.__init__(self, p, reg_count, lanes=lanes)
        self.depth = self.begun = self.ended = 0
        self.reads_inside = []

    @contextlib.contextmanager
    def batch(self):
        assert self.depth == 0
        self.depth += 1; self.begun += 1
        try:
            yield self
        finally:
            self.depth -= 1; self.ended += 1

    def batch_stats(self):
        return (0, self.ended, 256, 0)

    def get_int(self, src, lane=None):
        if self.depth:
            self.reads_inside.append(src)
        return LaneOracles.get_int(self, src, lane)


def make(lanes, batch, regs):
    if lanes == 1:
        return Recording(P, regs) if batch else orc.OracleEngine(P, regs)
    return (LaneRecording if batch else LaneOracles)(P, regs, lanes=lanes)


def go(form, lanes, batch, eng, **kw):
    mod, more, _ = FORMS[form]
    if lanes == 1:
        return [mod.run(eng, P, B1, B2, SIGMAS[0], D, batch=batch, **more, **kw)]
    return mod.run_lanes(eng, P, B1, B2, SIGMAS[:lanes], D, batch=batch, **more, **kw)


def point(form, lanes, eng):
    regs = FORMS[form][2]
    if lanes == 1:
        return [[eng.get_int(r) for r in regs]]
    return [[eng.get_int(r, lane=l) for r in regs] for l in range(lanes)]


def outcome(results):
    return [(r["sigma"], r["g1"], r["g2"], r["factors"]) for r in results]


def steps_of(form):
    return STEPS if form == "montgomery" else len(ed.naf(ecm.stage1_exponent(B1))) - 1


@pytest.fixture(scope="module")
def uninterrupted():
    out = {}
    for form in FORMS:
        for lanes in (1, 3):
            with make(lanes, False, ecm.registers_needed(D)) as eng:
                res = go(form, lanes, False, eng)
                out[(form, lanes)] = (outcome(res), point(form, lanes, eng))
    return out


def test_the_uninterrupted_runs_are_worth_comparing_with(uninterrupted):
    for (form, lanes), (res, pts) in uninterrupted.items():
        assert res[0] == (6, 1, 3217073, [3217073]) and all(r[1:] == (1, 1, []) for r in res[1:]) and len(res) == lanes
        assert all(all(pt) for pt in pts)
    assert uninterrupted[("montgomery", 3)][1][0] == uninterrupted[("montgomery", 1)][1][0]
    assert STEPS > 2 * EVERY and steps_of("edwards") in (STEPS, STEPS + 1)


@pytest.mark.parametrize("k", ["first", "middle", "multiple", "last"])
@pytest.mark.parametrize("batch", [False, True], ids=["plain", "batch"])
@pytest.mark.parametrize("lanes", [1, 3])
@pytest.mark.parametrize("form", list(FORMS))
def test_a_run_stopped_at_step_k_and_resumed_on_a_fresh_engine_ends_as_the_uninterrupted_one(form, lanes, batch, k, uninterrupted, tmp_path):
    steps = steps_of(form)
    k = {"first": 1, "middle": steps // 2 + 1, "multiple": 2 * EVERY, "last": steps}[k]
    assert 1 <= k <= steps and (steps // 2 + 1) % CHECK_EVERY            # the middle step is no step of a check or of a checkpoint
    ck = str(tmp_path / "stage1.ckpt")
    regs = ecm.registers_needed(D)
    with make(lanes, batch, regs) as eng:
        with pytest.raises(ecm.EcmStopped) as stop:
            go(form, lanes, batch, eng, checkpoint=ck, checkpoint_every=EVERY, stop_after=k)
        if batch:
            assert eng.begun == eng.ended and eng.depth == 0 and eng.reads_inside == []      # the registers are read between two batches
    assert (stop.value.path, stop.value.step) == (ck, k) and str(k) in str(stop.value)
    header, values = ecm_files.read_checkpoint(ck)
    assert (header["next"], header["curve"], header["sigmas"], header["lanes"]) == (k + 1, form, SIGMAS[:lanes], lanes)
    assert (header["p"], header["b1"], header["b2"], header["D"], header["group"], header["substitutes"]) == (P, B1, B2, D, 0, [])
    assert (header["scalar_bits"], header["scalar_sha256"]) == ecm_files.scalar_digest(ecm.stage1_exponent(B1)) and len(values) == 4
    with make(lanes, batch, regs) as eng:                        # a fresh engine object: nothing of the first run is left but the file
        res = go(form, lanes, batch, eng, checkpoint=ck, checkpoint_every=EVERY, stop_after=k)     # the same call again goes on and ends
        pts = point(form, lanes, eng)
        if batch:
            assert eng.begun == eng.ended and eng.depth == 0 and eng.reads_inside == []
    want, want_pts = uninterrupted[(form, lanes)]
    assert outcome(res) == want and pts == want_pts
    assert all(r["resumed_at"] == k for r in res) and not os.path.exists(ck)


def test_checkpoints_on_the_way_are_written_every_so_many_steps_and_any_of_them_resumes(uninterrupted, tmp_path, monkeypatch):
    ck = str(tmp_path / "stage1.ckpt")
    written = []
    write = ecm_files.write_checkpoint

    def recording(path, header, registers):
        written.append(header["next"] - 1)
        write(path, header, registers)
        write(path + ".%d" % (header["next"] - 1), header, registers)
    monkeypatch.setattr(ecm_files, "write_checkpoint", recording)
    with orc.OracleEngine(P, ecm.FIXED_REGISTERS) as eng:
        res = ecm.run(eng, P, B1, 0, 6, checkpoint=ck, checkpoint_every=6)
    assert written == list(range(6, STEPS, 6)) and "resumed_at" not in res and not os.path.exists(ck)      # a normal end removes the file
    # Edwards: only behind a check, so 6 becomes 8 with a check every 4 digits
    del written[:]
    with orc.OracleEngine(P, ecm.FIXED_REGISTERS) as eng:
        clean = ed.run(eng, P, B1, 0, 6, check_every=CHECK_EVERY)
        want = [eng.get_int(r) for r in ed.POINT]
    with orc.OracleEngine(P, ecm.FIXED_REGISTERS) as eng:
        res = ed.run(eng, P, B1, 0, 6, check_every=CHECK_EVERY, checkpoint=ck, checkpoint_every=6)
    assert written == list(range(8, steps_of("edwards"), 8)) and (res["checks"], res["doublings"]) == (clean["checks"], clean["doublings"])
    monkeypatch.undo()
    # the one of step 16, taken behind a passed check, goes on to the same point with the checks behind the same digits
    os.rename(ck + ".16", ck)
    with orc.OracleEngine(P, ecm.FIXED_REGISTERS) as eng:
        res = ed.run(eng, P, B1, 0, 6, check_every=CHECK_EVERY, checkpoint=ck)
        assert [eng.get_int(r) for r in ed.POINT] == want
    assert res["resumed_at"] == 16 and res["checks"] == clean["checks"] - 4 and res["doublings"] == clean["doublings"] - 16


def test_edwards_checkpoints_need_checks_on_the_way(tmp_path):
    ck = str(tmp_path / "stage1.ckpt")
    with orc.OracleEngine(P, ecm.FIXED_REGISTERS) as eng:
        for kw in ({"checkpoint_every": 8}, {"stop_after": 5}, {}):
            with pytest.raises(ValueError, match="passed the on-curve check"):
                ed.run(eng, P, B1, 0, 6, checkpoint=ck, **kw)
    assert not os.path.exists(ck)


def test_the_keywords_are_checked(tmp_path):
    ck = str(tmp_path / "stage1.ckpt")
    with orc.OracleEngine(P, ecm.FIXED_REGISTERS) as eng:
        for mod, more in ((ecm, {}), (ed, {"check_every": 4})):
            for kw in ({"stop_after": 5}, {"checkpoint_every": 8}, {"checkpoint": ck, "stop_after": -1}, {"checkpoint": ck, "checkpoint_every": -8}):
                with pytest.raises(ValueError, match="checkpoint"):
                    mod.run(eng, P, B1, 0, 6, **more, **kw)
    with pytest.raises(ValueError, match="checkpoint"):
        ecm.ecm(P, B1, 0, sigma=6, stop_after=5)


@pytest.mark.parametrize("form", list(FORMS))
def test_a_checkpoint_of_another_run_is_refused_and_the_engine_is_left_alone(form, tmp_path):
    mod, more, _ = FORMS[form]
    ck = str(tmp_path / "stage1.ckpt")
    regs = ecm.FIXED_REGISTERS
    with LaneOracles(P, regs, lanes=3) as eng, pytest.raises(ecm.EcmStopped):
        mod.run_lanes(eng, P, B1, 0, SIGMAS, checkpoint=ck, stop_after=9, **more)
    before = open(ck, "rb").read()
    other = "edwards" if form == "montgomery" else "montgomery"

    def filled(eng, lanes):
        for r in range(regs):
            for l in range(lanes):
                eng.set_int(r, 1000 * r + l + 1, lane=l)
        return eng

    def untouched(eng, lanes):
        return all(eng.get_int(r, lane=l) == 1000 * r + l + 1 for r in range(regs) for l in range(lanes))
    for what, call in (
        ("sigmas", lambda e: mod.run_lanes(e, P, B1, 0, [6, 8, 9], checkpoint=ck, **more)),
        ("sigmas", lambda e: mod.run_lanes(e, P, B1, 0, [8, 6, 7], checkpoint=ck, **more)),
        ("B1", lambda e: mod.run_lanes(e, P, B1 + 1, 0, SIGMAS, checkpoint=ck, **more)),
        ("group", lambda e: mod.run_lanes(e, P, B1, 0, SIGMAS, checkpoint=ck, group=1, **more)),
        ("curve form", lambda e: FORMS[other][0].run_lanes(e, P, B1, 0, SIGMAS, checkpoint=ck, **FORMS[other][1])),
    ):
        with LaneOracles(P, regs, lanes=3) as eng:
            filled(eng, 3)
            with pytest.raises(ecm_files.CheckpointError, match="another run"):
                call(eng)
            assert untouched(eng, 3), what
    with LaneOracles(P, regs, lanes=2) as eng:                   # another lane count
        filled(eng, 2)
        with pytest.raises(ecm_files.CheckpointError, match="sigmas"):
            mod.run_lanes(eng, P, B1, 0, SIGMAS[:2], checkpoint=ck, **more)
        assert untouched(eng, 2)
    with LaneOracles(P, regs, lanes=3) as eng:                   # a damaged file
        filled(eng, 3)
        with open(ck, "wb") as f:
            f.write(before[:-3])
        with pytest.raises(ecm_files.CheckpointError, match="short file"):
            mod.run_lanes(eng, P, B1, 0, SIGMAS, checkpoint=ck, **more)
        assert untouched(eng, 3)
    with open(ck, "wb") as f:
        f.write(before)
    with LaneOracles(P, regs, lanes=3) as eng:                   # and the file itself is still good for its own run
        assert all(r["resumed_at"] == 9 for r in mod.run_lanes(eng, P, B1, 0, SIGMAS, checkpoint=ck, **more))


def test_the_scalar_of_a_run_with_b1_below_11_and_a_stage_2_is_part_of_the_match(tmp_path):
    """B1 = 7 with a stage 2 over D = 210... has no prime to add; B1 = 3 over D = 30 adds 5: a checkpoint of the stage-1-only run is another's"""
    ck = str(tmp_path / "stage1.ckpt")
    with orc.OracleEngine(1009, ecm.registers_needed(30)) as eng:
        with pytest.raises(ecm.EcmStopped):
            ecm.run(eng, 1009, 3, 0, 7, checkpoint=ck, stop_after=1)
        with pytest.raises(ecm_files.CheckpointError, match="scalar"):
            ecm.run(eng, 1009, 3, 100, 7, 30, checkpoint=ck)
        assert ecm.run(eng, 1009, 3, 0, 7, checkpoint=ck)["resumed_at"] == 1


# ---- the feature costs no call when it is off ----

class Logged:
    """the oracle behind a wrapper that writes down every call"""

    def __init__(self, p, regs):
        self.o = orc.OracleEngine(p, regs)
        self.p, self.n, self.reg_count = p, self.o.n, regs
        self.log = []

    def __enter__(self): return self
    def __exit__(self, *a): self.o.close()

    def __getattr__(self, name):
        f = getattr(self.o, name)
        if not callable(f):
            return f

        def call(*a):
            self.log.append((name,) + a)
            return f(*a)
        return call


@pytest.mark.parametrize("form", list(FORMS))
def test_without_the_keywords_and_with_a_checkpoint_that_is_never_due_the_calls_are_the_same(form, tmp_path):
    mod, more, _ = FORMS[form]
    ck = str(tmp_path / "never.ckpt")
    logs = []
    for kw in ({}, {"checkpoint": ck, "checkpoint_every": 0, "stop_after": 0}, {"checkpoint": ck, "stop_after": 10 ** 6}):
        with Logged(P, ecm.registers_needed(D)) as eng:
            res = mod.run(eng, P, B1, B2, 6, D, **more, **kw)
            logs.append(eng.log)
        assert res["g2"] == 3217073 and "resumed_at" not in res and "x" not in res and not os.path.exists(ck)
    assert logs[0] == logs[1] == logs[2] and len(logs[0]) > 1000
    assert not hasattr(Logged(P, 1), "batch") and not hasattr(Logged(P, 1), "addsub")


# ---- stage-1 results out and in ----

@pytest.fixture(scope="module")
def full_runs():
    """g2 of run() with both stages, for the sigmas the saved lines are made of"""
    out = {}
    for sigma in (6, 8, 7, 9, 10):
        with orc.OracleEngine(P, ecm.registers_needed(D)) as eng:
            res = ecm.run(eng, P, B1, B2, sigma, D)
        assert res["g1"] == 1
        out[sigma] = res["g2"]
    assert out[6] == 3217073
    return out


def test_run_saved_on_the_line_of_a_stage_1_only_run_gives_the_g2_of_the_full_run(full_runs, tmp_path):
    path = str(tmp_path / "lines.p95")
    mp = (1 << P) - 1
    with orc.OracleEngine(P, ecm.FIXED_REGISTERS) as eng:
        res = ecm.run(eng, P, B1, 0, 6, save=path)
        xq, zq = eng.get_int(ecm.R_XQ), eng.get_int(ecm.R_ZQ)
    assert res["factors"] == [] and res["x"] * zq % mp == xq                   # the factor needs stage 2; x = X_Q / Z_Q
    lines = ecm_files.read_resume_file(path)
    assert lines == [{"p": P, "sigma": 6, "b1": B1, "x": res["x"]}]
    for mode in ("projective", "affine"):
        with orc.OracleEngine(P, ecm.registers_needed(D, mode)) as eng:
            out = ecm.run_saved(eng, lines, B2, D, stage2=mode)
        assert len(out) == 1 and (out[0]["g1"], out[0]["g2"], out[0]["factors"]) == (1, full_runs[6], [3217073])
        assert (out[0]["p"], out[0]["b1"], out[0]["b2"], out[0]["D"], out[0]["sigma"]) == (P, B1, B2, D, 6)
        assert ("stage2" in out[0]) == (mode == "affine")
    # the Edwards driver saves the line of the same curve
    path2 = str(tmp_path / "edwards.p95")
    with orc.OracleEngine(P, ecm.FIXED_REGISTERS) as eng:
        assert ed.run(eng, P, B1, 0, 6, save=path2)["x"] == res["x"]
    assert ecm_files.read_resume_file(path2) == lines


def test_run_lanes_saves_a_line_for_every_lane_that_has_one_and_run_saved_takes_them(full_runs, tmp_path):
    """lane 1 finds 3454817 in stage 1 (p = 1009, sigma 69, B1 = 50: tests/test_ecm.py) and lane 2 fails in the inversion of its start"""
    p, b1, f = 1009, 50, 3454817
    path = str(tmp_path / "lanes.p95")
    sigmas = [7, 69, f, 11]
    for inverse, cls in (("host", LaneOracles), ("engine", CrossOracles)):
        with cls(p, ecm.registers_needed(30, "affine", 4, inverse), lanes=4) as eng:
            res = ecm.run_lanes(eng, p, b1, 0, sigmas, save=path, stage2="affine", inverse=inverse)
            pts = [(eng.o[l].get_int(ecm.R_XQ), eng.o[l].get_int(ecm.R_ZQ)) for l in range(4)]
        assert [r["g1"] for r in res[:2]] == [1, f] and res[2]["g1"] % f == 0 and ["x" in r for r in res] == [True, False, False, True]
        for l in (0, 3):
            assert res[l]["x"] * pts[l][1] % ((1 << p) - 1) == pts[l][0]
    lines = ecm_files.read_resume_file(path)
    assert [l["sigma"] for l in lines] == [7, 11, 7, 11] and lines[:2] == lines[2:]         # host and engine inverses write the same lines
    with LaneOracles(p, ecm.registers_needed(30), lanes=2) as eng:
        out = ecm.run_saved(eng, lines[:2], 300, 30)
        with pytest.raises(ValueError, match="one line per lane"):
            ecm.run_saved(eng, lines[:1], 300, 30)
        with pytest.raises(ValueError, match="B2"):
            ecm.run_saved(eng, lines[:2], b1, 30)
        with pytest.raises(ValueError, match="one p"):
            ecm.run_saved(eng, [lines[0], dict(lines[1], b1=51)], 300, 30)
    want = []
    for s in (7, 11):
        with orc.OracleEngine(p, ecm.registers_needed(30)) as eng:
            want.append(ecm.run(eng, p, b1, 300, s, 30)["g2"])
    assert [r["g2"] for r in out] == want and [r["sigma"] for r in out] == [7, 11]


def test_ecm_saved_pads_a_short_last_group_and_drops_the_padding(full_runs, tmp_path, monkeypatch):
    path = str(tmp_path / "five.p95")
    with LaneOracles(P, ecm.FIXED_REGISTERS, lanes=5) as eng:
        res = ecm.run_lanes(eng, P, B1, 0, [6, 8, 7, 9, 10], save=path)
    assert all("x" in r for r in res)
    with open(path, "a") as f:                                                   # a line of another exponent: a group, and an engine, of its own
        f.write("# another exponent\n")
    with orc.OracleEngine(1009, ecm.FIXED_REGISTERS) as eng:
        ecm.run(eng, 1009, 50, 0, 7, save=path)
    monkeypatch.setattr(E, "Engine", LaneOracles)
    LaneOracles.made = []
    ran = []
    run_saved = ecm.run_saved
    monkeypatch.setattr(ecm, "run_saved", lambda eng, lines, *a, **k: ran.append([l["sigma"] for l in lines]) or run_saved(eng, lines, *a, **k))
    out = ecm.ecm_saved(path, B2, lanes=3, D=D)
    assert ran == [[6, 8, 7], [9, 10, 9], [7, 7, 7]]                           # padded by the group's first line
    assert [(e.p, e.lanes, e.reg_count) for e in LaneOracles.made] == [(P, 3, ecm.registers_needed(D)), (1009, 3, ecm.registers_needed(D))]
    assert out["curves"] == 6 and [r["sigma"] for r in out["results"]] == [6, 8, 7, 9, 10, 7]
    assert [r["g2"] for r in out["results"][:5]] == [full_runs[s] for s in (6, 8, 7, 9, 10)] and out["factors"] == [3217073]
    assert json.dumps(out)
    one = ecm.ecm_saved(path, B2, lanes=1, D=D, stage2="affine")                # no padding at all
    assert [r["g2"] for r in one["results"]] == [r["g2"] for r in out["results"]] and len(LaneOracles.made) == 4
    with pytest.raises(ValueError, match="onelaunch"):
        ecm.ecm_saved(path, B2, lanes=3, batch=True)


def test_save_is_refused_where_the_scalar_holds_more_than_b1_says(tmp_path):
    path = str(tmp_path / "no.p95")
    with orc.OracleEngine(1009, ecm.registers_needed(30)) as eng:
        for mod, more in ((ecm, {}), (ed, {})):
            with pytest.raises(ValueError, match="B1 = 3 < 11"):
                mod.run(eng, 1009, 3, 100, 7, 30, save=path, **more)           # 5 divides D = 30 and lies in (3, 100]
        assert not os.path.exists(path)
        res = ecm.run(eng, 1009, 3, 0, 7, save=path)                           # stage 1 alone describes its B1
        lines = ecm_files.read_resume_file(path)
        assert lines == [{"p": 1009, "sigma": 7, "b1": 3, "x": res["x"]}]
        with pytest.raises(ValueError, match="prime 5"):                       # ... and stage 2 over D = 30 cannot make up for the 5
            ecm.run_saved(eng, lines, 100, 30)


# ---- ecm() and the command line ----

def test_ecm_resumes_the_group_it_stopped_in_and_skips_the_groups_before(tmp_path, monkeypatch):
    monkeypatch.setattr(E, "Engine", LaneOracles)
    ck = str(tmp_path / "ecm.ckpt")
    kw = dict(sigma=7, curves=6, lanes=3, seed=1)
    want = ecm.ecm(1009, 20, 0, **kw)
    assert len(want["sigmas"]) == 6 and not want["factors"]
    with pytest.raises(ecm.EcmStopped):                                         # stops in the first group ...
        ecm.ecm(1009, 20, 0, checkpoint=ck, stop_after=5, **kw)
    assert ecm_files.read_checkpoint(ck)[0]["group"] == 0
    with pytest.raises(ecm.EcmStopped):                                         # ... which then ends; the second group stops at its own step 5
        ecm.ecm(1009, 20, 0, checkpoint=ck, stop_after=5, **kw)
    header = ecm_files.read_checkpoint(ck)[0]
    assert header["group"] == 1 and header["sigmas"] == want["sigmas"][3:] and header["next"] == 6
    for other in (dict(kw, seed=2), dict(kw, lanes=2), dict(kw, curves=3)):     # other sigmas, other lanes, no such group
        with pytest.raises(ecm_files.CheckpointError, match="another run"):
            ecm.ecm(1009, 20, 0, checkpoint=ck, **other)
    LaneOracles.made = []
    calls = []
    run_lanes = ecm.run_lanes
    monkeypatch.setattr(ecm, "run_lanes", lambda *a, **k: calls.append(k["group"]) or run_lanes(*a, **k))
    got = ecm.ecm(1009, 20, 0, checkpoint=ck, stop_after=5, **kw)
    assert calls == [1] and not os.path.exists(ck)                              # the first group is not run again
    assert got.pop("resumed_at") == 5 and all(r.pop("resumed_at") == 5 for r in got["batch"])
    for r in [got, want] + got["batch"] + want["batch"]:                        # a resumed run counts the operations from its checkpoint on
        for key in COUNTS:
            r.pop(key)
    assert got["sigmas"] == want["sigmas"] and got["batch"] == want["batch"] and got == want


def test_the_command_line_passes_the_options_and_has_an_exit_code_for_a_stop(monkeypatch, capsys, tmp_path):
    seen = {}

    def fake(*a, **k):
        seen["args"], seen["kw"] = a, k
        if k.get("stop_after"):
            raise ecm.EcmStopped(k["checkpoint"], k["stop_after"])
        return {"factors": []}
    monkeypatch.setattr(ecm, "ecm", fake)
    assert ecm.main(["1009", "50"]) == 1 and seen["kw"] == {}
    assert ecm.main(["1009", "50", "--save", "a.p95", "--checkpoint", "a.ckpt", "--checkpoint-every", "1000"]) == 1
    assert seen["kw"] == {"save": "a.p95", "checkpoint": "a.ckpt", "checkpoint_every": 1000} and seen["args"][:3] == (1009, 50, 0)
    capsys.readouterr()
    assert ecm.main(["1009", "50", "--checkpoint", "a.ckpt", "--stop-after", "7"]) == ecm.EXIT_STOPPED == 3
    assert json.loads(capsys.readouterr().out) == {"stopped_at": 7, "checkpoint": "a.ckpt"}
    monkeypatch.setattr(ecm, "ecm_saved", lambda *a: seen.update(saved=a) or {"factors": [3], "curves": 1, "results": []})
    assert ecm.main(["--resume-file", "a.p95", "5000", "--lanes", "4", "--D", "30", "--stage2", "affine"]) == 0
    assert seen["saved"][:4] == ("a.p95", 5000, 4, 30) and seen["saved"][-2:] == ("affine", "host")
    for bad in (["--resume-file", "a.p95", "5000", "1009"], ["--resume-file", "a.p95", "x"], ["--resume-file", "a.p95", "5000", "--save", "b"], []):
        with pytest.raises(SystemExit) as err:
            ecm.main(bad)
        assert err.value.code == 2
    capsys.readouterr()


def test_the_command_line_stops_and_goes_on(monkeypatch, capsys, tmp_path):
    monkeypatch.setattr(E, "Engine", LaneOracles)
    ck, lines = str(tmp_path / "cli.ckpt"), str(tmp_path / "cli.p95")
    args = ["1009", "50", "--sigma", "7", "--checkpoint", ck, "--stop-after", "20", "--save", lines]
    assert ecm.main(args) == 3 and os.path.exists(ck) and not os.path.exists(lines)
    assert json.loads(capsys.readouterr().out) == {"stopped_at": 20, "checkpoint": ck}
    assert ecm.main(args) == 1 and not os.path.exists(ck)
    res = json.loads(capsys.readouterr().out)
    assert ecm.main(["1009", "50", "--sigma", "7"]) == 1
    want = json.loads(capsys.readouterr().out)
    assert [res.pop(key) < want.pop(key) for key in COUNTS] == [True] * 3       # counted from the checkpoint on
    assert res.pop("resumed_at") == 20 and res.pop("x") == ecm_files.read_resume_file(lines)[0]["x"] and res == want
    assert ecm.main(["--resume-file", lines, "300", "--D", "30"]) == 1
    out = json.loads(capsys.readouterr().out)
    with orc.OracleEngine(1009, ecm.registers_needed(30)) as eng:
        assert out["results"][0]["g2"] == ecm.run(eng, 1009, 50, 300, 7, 30)["g2"] and out["curves"] == 1
