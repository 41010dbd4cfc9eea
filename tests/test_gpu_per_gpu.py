"""`launch.run_sharded(per_gpu > 1)` on the engine: several entries of one rank run concurrently from Python threads, one engine and stream
each, on one device.  No process group here (one rank); the launcher's bookkeeping under a process group is tests/test_sharding_gloo.py.
Verdicts come from Python integers, the final res64 of M11213 from the reference's known answers.  This path is tested for results, not
for throughput.  Needs a real MI355X:  python -m pytest tests -m gpu"""
import json
import os
import threading
import time

import pytest

import orc

pytestmark = pytest.mark.gpu

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_known_answers.json")))
WORKTODO = ["PRP=1,2,9941,-1", "PRP=1,2,9949,-1", "Test=2203", "PRP=1,2,11213,-1", "Test=607"]
ENTRIES = [("prp", 9941), ("prp", 9949), ("ll", 2203), ("prp", 11213), ("ll", 607)]
ITERATIONS = 9941 + 9949 + 2201 + 11213 + 605      # PRP: p squarings, LL: p - 2
PLAN = "marin-hip:n=512:m1=8:m2=32:c=4"             # 9941, 9949 and 11213 by default; 2203 and 607 are smaller


def make_engine(p):
    from prmers_amd import Engine, prp
    e = Engine(p, prp.REGISTERS)
    if p > 9000:
        assert e.describe() == PLAN, (p, e.describe())
    return e


@pytest.fixture(scope="module")
def verdicts():
    """is 2^p - 1 prime, by Python integers: 3^(2^p) = 9 for the PRP entries, the Lucas-Lehmer sequence for the others"""
    out = {}
    for mode, p in ENTRIES:
        m = (1 << p) - 1
        if mode == "prp":
            x = 3
            for _ in range(p):
                x = orc.mers_reduce(x * x, p)
            out[p] = x == 9
        else:
            s = 4
            for _ in range(p - 2):
                s = orc.mers_reduce(s * s + m - 2, p)
            out[p] = s == 0
        assert out[p] == (p in GOLD["prime_exponents"])     # (the reference's own list agrees)
    return out


def run(per_gpu=2, lines=WORKTODO, **kw):
    from prmers_amd import launch
    kw.setdefault("checklevel", 1)
    return launch.run_sharded(lines, make_engine, per_gpu=per_gpu, **kw)


def check_complete(res, status, verdicts, entries=ENTRIES):
    assert len(res) == len(entries)                                  # one result per entry
    by_p = {r["exponent"]: r for r in res}
    for mode, p in entries:
        r = by_p[p]
        assert r["mode"] == mode and r["complete"] and not r.get("error"), r
        assert r["is_prime"] == verdicts[p], p
        assert r["iterations"] == (p if mode == "prp" else p - 2)
    if 11213 in by_p:
        assert by_p[11213]["res64"].upper() == GOLD["m11213_final"]["res64"].upper()
    assert status["check_boundary_reductions"] is False


def test_two_entries_at_a_time(verdicts):
    t0 = time.time()
    seen = []
    res, status = run(2, on_status=seen.append)
    check_complete(res, status, verdicts)
    assert status["iterations"] == ITERATIONS and status["all_ok"] == 1 and status["gerbicz_errors"] == 0
    assert len(seen) == 1                                            # no process group: the reduction at exit only
    print("per_gpu=2, five entries: %.2f s" % (time.time() - t0))


def test_more_threads_than_entries(verdicts):
    """per_gpu = 3 on two entries: two threads, and each entry runs once"""
    made, lock, peak = [], threading.Lock(), [0, 0]

    def counting(p):
        e = make_engine(p)
        with lock:
            made.append(p)
            peak[0] += 1
            peak[1] = max(peak)
        close = e.close

        def closing():
            with lock:
                peak[0] -= 1
            close()
        e.close = closing
        return e
    from prmers_amd import launch
    res, status = launch.run_sharded(["PRP=1,2,9941,-1", "Test=2203"], counting, per_gpu=3, checklevel=1)
    check_complete(res, status, verdicts, [("prp", 9941), ("ll", 2203)])
    assert sorted(made) == [2203, 9941] and peak[1] <= 2
    assert status["iterations"] == 9941 + 2201 and status["all_ok"] == 1


def test_an_injected_error_in_every_long_entry(verdicts):
    """erroriter = 9000: the three PRP entries longer than that each meet one failed Gerbicz-Li check, roll back and still end on the
    right residue; the Lucas-Lehmer entries are shorter and have no check"""
    msgs = []
    res, status = run(2, erroriter=9000, log=msgs.append)
    check_complete(res, status, verdicts)
    by_p = {r["exponent"]: r for r in res}
    assert [by_p[p]["gerbicz_errors"] for _, p in ENTRIES] == [1, 1, 0, 1, 0]
    assert status["gerbicz_errors"] == 3 and status["all_ok"] == 0
    assert status["iterations"] == ITERATIONS                        # every entry reports the iteration it ended on
    assert sum("Check FAILED" in m for m in msgs) == 3 and sum("Injected error" in m for m in msgs) == 3


def test_interrupt_and_resume(verdicts, tmp_path):
    """should_stop turns true after a number of polls (one per entry started and one per run of plain iterations): the entries running then
    checkpoint and return, the rest are skipped; a second launch resumes from the checkpoints and gives the base case's results"""
    polls, lock = [0], threading.Lock()

    def stop():
        with lock:
            polls[0] += 1
            return polls[0] > 40
    res1, st1 = run(2, should_stop=stop, ckpt_dir=str(tmp_path))
    assert len(res1) == len(ENTRIES) and st1["all_ok"] == 1
    interrupted = [r for r in res1 if r.get("interrupted")]
    assert len(interrupted) == len(ENTRIES) and not any(r["complete"] for r in res1)   # 40 polls end inside the first two entries
    started = [r for r in interrupted if r["iterations"] > 0]
    assert len(started) == 2 and {r["exponent"] for r in started} == {9941, 9949}
    assert all(os.path.exists(os.path.join(str(tmp_path), "m_%d.ckpt" % r["exponent"])) for r in started)
    assert 0 < st1["iterations"] == sum(r["iterations"] for r in started) < 9941 + 9949
    msgs = []
    res, status = run(2, ckpt_dir=str(tmp_path), log=msgs.append)
    check_complete(res, status, verdicts)
    assert sum("Resuming from a checkpoint" in m for m in msgs) == 2
    assert status["iterations"] == ITERATIONS and status["all_ok"] == 1 and status["gerbicz_errors"] == 0
