"""ECM that stops and goes on, on the engine: the stage 1 of the reference's published resume line for 2^149 - 1 on a lane of a batched
one-launch engine, stage-1 checkpoints that resume on a fresh Engine (also on one of another plan: the payload is canonical words),
Edwards checkpoints behind a passed check, stage 2 from saved lines, and the command line in child processes.
Needs a real MI355X:  python -m pytest tests -m gpu"""
import json
import os
import subprocess
import sys

import pytest

from prmers_amd import ecm, ecm_files, ecm_edwards

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ecm_resume_p149.p95")


def sigmas_for(count, first=()):
    return list(first) + [1000003 + 17 * i for i in range(count - len(first))]


def outcome(results):
    return [(r["sigma"], r["g1"], r["g2"], r["factors"]) for r in results]


def point(e):
    return e.get_ints(ecm.R_XQ), e.get_ints(ecm.R_ZQ)


def test_the_fixture_s_curve_in_lane_0_ends_in_the_fixture_s_line(tmp_path):
    from prmers_amd import Engine
    want = ecm_files.parse_resume_line(open(FIXTURE).read())
    p, b1, sigma = want["p"], want["b1"], want["sigma"]
    assert (p, b1) == (149, 20000)
    path = str(tmp_path / "p149.p95")
    with Engine(p, ecm.FIXED_REGISTERS, lanes=3, onelaunch=True) as e:
        res = ecm.run_lanes(e, p, b1, 0, [sigma, 7, 11], batch=True, save=path)
    assert res[0]["g1"] == 1 and res[0]["x"] == want["x"] and res[0]["launches"] > 0
    lines = ecm_files.read_resume_file(path)
    assert lines[0] == want
    text = open(path).readline()
    assert "X=0x%x; CHECKSUM=%d;" % (want["x"], ecm_files.checksum(b1, sigma, (1 << p) - 1, want["x"])) in text
    assert "CHECKSUM=1732255967;" in text and len(lines) == sum("x" in r for r in res)


@pytest.fixture(scope="module")
def at_1277():
    """64 lanes, one-launch, batched, B1 = 300: the uninterrupted run, and a checkpoint of a middle step"""
    from prmers_amd import Engine
    import tempfile
    p, b1, sigmas = 1277, 300, sigmas_for(64)
    steps = ecm.stage1_exponent(b1).bit_length() - 1
    k = steps // 2 + 3
    ck = os.path.join(tempfile.mkdtemp(), "p1277.ckpt")
    with Engine(p, ecm.FIXED_REGISTERS, lanes=64, onelaunch=True) as e:
        want = ecm.run_lanes(e, p, b1, 0, sigmas, batch=True)
        pt = point(e)
    with Engine(p, ecm.FIXED_REGISTERS, lanes=64, onelaunch=True) as e:
        with pytest.raises(ecm.EcmStopped) as stop:
            ecm.run_lanes(e, p, b1, 0, sigmas, batch=True, checkpoint=ck, checkpoint_every=100, stop_after=k)
    assert stop.value.step == k and ecm_files.read_checkpoint(ck)[0]["next"] == k + 1
    return p, b1, sigmas, k, open(ck, "rb").read(), outcome(want), pt


@pytest.mark.parametrize("plan", ["onelaunch", "three launches"])
def test_a_checkpoint_of_a_middle_step_resumes_on_a_fresh_engine_of_either_plan(plan, at_1277, tmp_path):
    from prmers_amd import Engine
    p, b1, sigmas, k, image, want, pt = at_1277
    ck = str(tmp_path / "p1277.ckpt")
    with open(ck, "wb") as f:
        f.write(image)
    one = plan == "onelaunch"
    with Engine(p, ecm.FIXED_REGISTERS, lanes=64, onelaunch=one) as e:
        res = ecm.run_lanes(e, p, b1, 0, sigmas, batch=one, checkpoint=ck)
        got = point(e)
    assert outcome(res) == want and got == pt and all(r["resumed_at"] == k for r in res) and not os.path.exists(ck)
    assert all(pt[1]) and len(set(pt[0])) == 64


def test_stop_and_resume_on_a_three_launch_engine_with_five_lanes(tmp_path):
    from prmers_amd import Engine
    p, b1, b2, D, sigmas = 3001, 30, 300, 30, [6, 8, 7, 9, 10]
    ck = str(tmp_path / "p3001.ckpt")
    with Engine(p, ecm.registers_needed(D), lanes=5) as e:
        want = ecm.run_lanes(e, p, b1, b2, sigmas, D)
        pt = point(e)
    with Engine(p, ecm.registers_needed(D), lanes=5) as e, pytest.raises(ecm.EcmStopped):
        ecm.run_lanes(e, p, b1, b2, sigmas, D, checkpoint=ck, stop_after=17)
    with Engine(p, ecm.registers_needed(D), lanes=5) as e:
        res = ecm.run_lanes(e, p, b1, b2, sigmas, D, checkpoint=ck)
        assert point(e) == pt
    assert outcome(res) == outcome(want) and res[0]["factors"] == [3217073] and all(r["resumed_at"] == 17 for r in res)


def test_an_edwards_checkpoint_behind_a_passed_check_resumes_to_the_same_point(tmp_path):
    from prmers_amd import Engine
    p, b1, sigmas = 1277, 300, sigmas_for(64)
    ck = str(tmp_path / "edwards.ckpt")
    kw = dict(check_every=32, batch=True)
    with Engine(p, ecm_edwards.FIXED_REGISTERS, lanes=64, onelaunch=True) as e:
        want = ecm_edwards.run_lanes(e, p, b1, 0, sigmas, **kw)
        pt = [e.get_ints(r) for r in ecm_edwards.POINT]
    with Engine(p, ecm_edwards.FIXED_REGISTERS, lanes=64, onelaunch=True) as e, pytest.raises(ecm.EcmStopped) as stop:
        ecm_edwards.run_lanes(e, p, b1, 0, sigmas, checkpoint=ck, checkpoint_every=100, stop_after=200, **kw)
    assert stop.value.step == 200 and ecm_files.read_checkpoint(ck)[0]["curve"] == "edwards"
    with Engine(p, ecm_edwards.FIXED_REGISTERS, lanes=64, onelaunch=True) as e:
        res = ecm_edwards.run_lanes(e, p, b1, 0, sigmas, checkpoint=ck, **kw)
        assert [e.get_ints(r) for r in ecm_edwards.POINT] == pt
    assert outcome(res) == outcome(want) and all(r["rollbacks"] == 0 and r["resumed_at"] == 200 for r in res)


@pytest.mark.parametrize("mode", ["projective", "affine"])
def test_stage_2_from_saved_lines_gives_the_g2_of_the_full_run(mode, tmp_path):
    from prmers_amd import Engine
    p, b1, b2, D, sigmas = 1277, 300, 5000, 210, sigmas_for(64)
    path = str(tmp_path / "p1277.p95")
    regs = ecm.registers_needed(D, mode)
    with Engine(p, regs, lanes=64, onelaunch=True) as e:
        full = ecm.run_lanes(e, p, b1, b2, sigmas, D, batch=True, stage2=mode)
    with Engine(p, regs, lanes=64, onelaunch=True) as e:
        first = ecm.run_lanes(e, p, b1, 0, sigmas, batch=True, save=path)
    lines = ecm_files.read_resume_file(path)
    assert all(r["g1"] == 1 for r in full) and len(lines) == 64 and [l["x"] for l in lines] == [r["x"] for r in first]
    with Engine(p, regs, lanes=64, onelaunch=True) as e:
        out = ecm.run_saved(e, lines, b2, D, stage2=mode, batch=True)
    assert [(r["sigma"], r["g2"]) for r in out] == [(r["sigma"], r["g2"]) for r in full]


def test_the_command_line_stops_and_the_same_command_goes_on(tmp_path):
    """two child processes, each under a time limit of its own, the second only after the first has ended as it should"""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    args = ["timeout", "-k", "10", "120", sys.executable, "-m", "prmers_amd.ecm", "1277", "300", "--sigma", "1000003", "--lanes", "4", "--curves", "4",
            "--onelaunch", "--batch", "--checkpoint", "cli.ckpt", "--stop-after", "150", "--save", "cli.p95"]
    first = subprocess.run(args, capture_output=True, text=True, cwd=str(tmp_path), env=env)
    assert first.returncode == ecm.EXIT_STOPPED, first.stdout + first.stderr
    assert json.loads(first.stdout) == {"stopped_at": 150, "checkpoint": "cli.ckpt"} and (tmp_path / "cli.ckpt").exists()
    second = subprocess.run(args, capture_output=True, text=True, cwd=str(tmp_path), env=env)
    assert second.returncode == 1, second.stdout + second.stderr
    res = json.loads(second.stdout)
    assert res["resumed_at"] == 150 and res["factors"] == [] and len(res["batch"]) == 4 and not (tmp_path / "cli.ckpt").exists()
    lines = ecm_files.read_resume_file(str(tmp_path / "cli.p95"))
    assert [l["sigma"] for l in lines] == res["sigmas"] and [l["x"] for l in lines] == [r["x"] for r in res["batch"]]
