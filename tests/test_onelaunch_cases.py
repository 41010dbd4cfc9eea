"""Host side of the one-launch products (no GPU): the plan token `onelaunch` through resolve_plan, what make_plan refuses, and the case
list of test_gpu_onelaunch.py (onelaunch_cases.py) -- which work-group shapes, transform families and run lengths it reaches, from the
shape rule itself (plan.hpp onelaunch_shape through tests/host/onelaunch_shape.cpp) and its restatement side by side.  Also ecm.ecm's
option on the stand-in engine of test_lanes_host.py."""
import os
import random
import subprocess
import tempfile

import pytest

import onelaunch_cases as oc
from prmers_amd import ecm
from prmers_amd import engine as E
from prmers_amd.engine import resolve_plan
from test_lanes_host import LaneOracles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the token ----

def test_the_token_round_trips_and_follows_the_lanes():
    assert resolve_plan(9941, "lanes=4,onelaunch") == "marin-hip:n=512:m1=8:m2=32:c=4:lanes=4:onelaunch"
    assert resolve_plan(9941, "onelaunch,lanes=4") == "marin-hip:n=512:m1=8:m2=32:c=4:lanes=4:onelaunch"
    assert resolve_plan(9941, "onelaunch") == "marin-hip:n=512:m1=8:m2=32:c=4:onelaunch"      # a plain engine: after c=
    assert resolve_plan(9941, "lanes=1,onelaunch") == resolve_plan(9941, "onelaunch")
    assert resolve_plan(9941, "m2=16,c=2,lanes=65535,onelaunch") == "marin-hip:n=512:m1=16:m2=16:c=2:lanes=65535:onelaunch"
    for p, spec, lanes in oc.CASES:
        text = resolve_plan(p, oc.token(spec, lanes))
        assert text == resolve_plan(p, spec) + ":lanes=%d:onelaunch" % lanes
        assert resolve_plan(p, text) == text


def test_without_the_token_every_description_is_what_it_was():
    assert resolve_plan(9941) == "marin-hip:n=512:m1=8:m2=32:c=4"
    assert resolve_plan(9941, "lanes=4") == "marin-hip:n=512:m1=8:m2=32:c=4:lanes=4"
    assert resolve_plan(127) == "marin-hip:n=8:m1=1:m2=4:c=4"
    assert resolve_plan(204800) == "marin-hip:n=10240:m1=80:m2=64:c=4"
    assert resolve_plan(110503, "split5") == "marin-hip:n=5120:m1=40:m2=64:c=1:split5"
    for p, spec, lanes in oc.CASES:
        assert "onelaunch" not in resolve_plan(p, spec) and "onelaunch" not in resolve_plan(p, (spec + "," if spec else "") + "lanes=%d" % lanes)


@pytest.mark.parametrize("p, spec", oc.REFUSED, ids=["%d-%s" % c for c in oc.REFUSED])
def test_refusals_name_the_token(p, spec):
    with pytest.raises(E.EngineError, match="onelaunch"):
        resolve_plan(p, spec)
    resolve_plan(p, spec.replace(",onelaunch", "") if "," in spec else None)        # the same plan without the token exists


def test_the_refusals_are_the_ones_that_were_asked_for():
    assert {(p, s) for p, s in oc.REFUSED} >= {(204800, "onelaunch"), (9941, "c=1,onelaunch"), (9941, "crt:9,onelaunch")}
    assert any("split5" in s for _, s in oc.REFUSED)
    assert oc.fields(resolve_plan(oc.FIRST_REFUSED_P))["n"] == 10240 and oc.FIRST_REFUSED_P == oc.LARGEST_P + 1


def test_the_largest_exponent_is_accepted():
    assert resolve_plan(oc.LARGEST_P, "onelaunch") == "marin-hip:n=8192:m1=32:m2=128:c=4:onelaunch"
    assert oc.fields(resolve_plan(oc.LARGEST_P, "lanes=2,onelaunch"))["n"] == oc.MAX_N


# ---- the shapes the cases reach ----

@pytest.fixture(scope="module")
def shapes():
    """(p, spec, lanes) -> the fields of one line of tests/host/onelaunch_shape.cpp"""
    exe = os.path.join(tempfile.mkdtemp(), "onelaunch_shape")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "prmers_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "onelaunch_shape.cpp")])
    lines = subprocess.check_output([exe] + ["%d:%d%s" % (p, lanes, ":" + spec if spec else "") for p, spec, lanes in oc.CASES]).decode().splitlines()
    assert len(lines) == len(oc.CASES)
    out = {}
    for case, line in zip(oc.CASES, lines):
        out[case] = {k: int(v) for k, v in (t.split("=") for t in line.split())}
        assert out[case]["p"] == case[0] and out[case]["lanes"] == case[2]
    return out


def test_the_list_has_no_duplicates_and_the_restated_rule_is_the_rule(shapes):
    assert len(oc.CASES) == len(set(oc.CASES))
    for case, f in shapes.items():
        p, spec, lanes = case
        g = oc.fields(resolve_plan(p, oc.token(spec, lanes)))
        assert (g["n"], g["m1"], g["m2"], g["c"]) == (f["n"], f["m1"], f["m2"], f["c"]) and f["n"] == 2 * f["m1"] * f["m2"] <= oc.MAX_N
        assert (f["tl"], f["k"], f["groups"], f["lds"]) == oc.shape(f["n"], lanes), case
        # what the kernel relies on: whole lanes in a group of at most 1024 threads, inside the LDS of a CU, teams that divide evenly
        m, r5 = f["n"] // 2, f["r5"]
        assert f["k"] * f["tl"] <= 1024 and f["lds"] == f["k"] * m * 32 <= oc.LDS_BYTES and f["groups"] * f["k"] >= lanes > (f["groups"] - 1) * f["k"]
        assert f["tl"] % r5 == 0 and f["tl"] // r5 & (f["tl"] // r5 - 1) == 0 and m % f["tl"] == 0
        tiles, cteams, rteams = f["m2"] // f["c"], min(f["m2"] // f["c"], f["tl"] // r5), min(f["m1"], f["tl"])
        assert tiles % cteams == 0 and f["tl"] % cteams == 0 and f["m1"] % rteams == 0 and f["tl"] % rteams == 0
        assert f["c"] >= 2


def test_the_rule_at_its_edges():
    assert oc.shape(8, 512) == (4, 64, 8, 64 * 4 * 32) and oc.shape(8, 3) == (4, 4, 1, 4 * 4 * 32) and oc.shape(8, 1) == (4, 1, 1, 128)
    assert oc.shape(64, 512) == (32, 8, 64, 8 * 32 * 32) and oc.shape(64, 9) == (32, 8, 2, 8 * 32 * 32)
    assert oc.shape(40, 5) == (20, 8, 1, 8 * 20 * 32) and oc.shape(40, 100) == (20, 12, 9, 12 * 20 * 32)
    assert oc.shape(512, 300) == (256, 1, 300, 8192) and oc.shape(1024, 2) == (512, 1, 2, 16384)
    assert oc.shape(5120, 3) == (640, 1, 3, 80 * 1024) and oc.shape(8192, 2) == (1024, 1, 2, 128 * 1024)


def test_the_cases_reach_every_shape_that_was_asked_for(shapes):
    by = lambda pred: [c for c, f in shapes.items() if pred(c, f)]
    assert by(lambda c, f: f["k"] > 1 and c[2] > f["k"] and c[2] % f["k"])               # a tail group with dead lanes
    assert by(lambda c, f: c[2] < f["k"])                                               # fewer lanes than a group holds
    assert by(lambda c, f: f["k"] > 1 and c[2] == f["k"] + 1)                           # the last lane alone in its group
    assert by(lambda c, f: f["k"] == 1)
    assert by(lambda c, f: f["m1"] == 1 and c[0] == 127 and f["n"] == 8 and f["m2"] == f["c"])   # one tile
    for p, n in oc.BARE_RADIX5.items():
        assert by(lambda c, f: c[0] == p and f["n"] == n and f["m1"] == 5 and f["r5"] == 5), p
    for p, n in oc.RADIX5_WITH_POW2.items():
        assert by(lambda c, f: c[0] == p and f["n"] == n and f["r5"] == 5 and f["m1"] > 5), p
    assert by(lambda c, f: f["tl"] == 640) and by(lambda c, f: f["tl"] == 1024)
    assert by(lambda c, f: c[0] == oc.LARGEST_P and f["n"] == oc.MAX_N and f["sum_fast"] == 0 and f["lds"] == 128 * 1024)
    assert by(lambda c, f: f["sum_fast"] == 1 and f["k"] > 1) and by(lambda c, f: f["sum_fast"] == 1 and f["k"] == 1)   # mul_sum as one product
    for p in oc.SMALL_EXPONENTS:
        for count in oc.SMALL_LANE_COUNTS:
            assert (p, None, count) in shapes, (p, count)
    for (p, spec), c in oc.RUN_LENGTHS.items():
        assert by(lambda k, f: k[:2] == (p, spec) and f["c"] == c and c != 4), (p, spec)
    assert by(lambda c, f: f["m2"] // f["c"] > f["tl"] // f["r5"])                        # more tiles than column teams: two trips through the column phases
    assert by(lambda c, f: f["m1"] > f["tl"])                                             # more rows than row teams: two trips through the row phase
    assert by(lambda c, f: f["m1"] * f["m2"] > f["tl"] and f["m1"] <= f["tl"])            # more pairs than threads, one trip


def test_no_case_needs_more_than_a_gibibyte_of_registers(shapes):
    for (p, spec, lanes), f in shapes.items():
        assert oc.register_bytes(f["n"], lanes) < oc.BUDGET_BYTES, (p, spec, lanes)


def test_the_large_factor_is_above_the_fused_bound_of_its_plan():
    p, spec, lanes, a = oc.FACTOR_CASE
    exe = os.path.join(tempfile.mkdtemp(), "plan_query")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "prmers_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "plan_query.cpp")])
    line = subprocess.check_output([exe, "%d:%s" % (p, oc.token(spec, lanes))]).decode()
    f = dict(t.split("=") for t in line.split())
    assert int(f["p"]) == p and 3 <= int(f["a_fast"]) < a < 2**32


# ---- the ECM driver's option ----

def test_ecm_passes_the_token_in_the_plan_and_draws_the_same_sigmas(monkeypatch):
    monkeypatch.setattr(E, "Engine", LaneOracles)
    LaneOracles.made = []
    plans = []
    init = LaneOracles.__init__

    def recording(self, p, reg_count, device=0, plan=None, lanes=1):
        plans.append(plan)
        init(self, p, reg_count, device, plan, lanes)
    monkeypatch.setattr(LaneOracles, "__init__", recording)
    with_token = ecm.ecm(1009, 20, 0, sigma=7, curves=5, lanes=3, seed=1, onelaunch=True)
    without = ecm.ecm(1009, 20, 0, sigma=7, curves=5, lanes=3, seed=1)
    assert plans == ["onelaunch", None] and [e.lanes for e in LaneOracles.made] == [3, 3]
    assert with_token["sigmas"] == without["sigmas"] and with_token["factors"] == without["factors"]
    rng = random.Random(1)
    drawn = [7] + [rng.randrange(ecm.SIGMA_MIN, 1 << 32) for _ in range(5)]
    assert with_token["sigmas"] == drawn[:len(with_token["sigmas"])]
    plans.clear()
    ecm.ecm(1009, 20, 0, sigma=7, plan="m2=4", onelaunch=True)
    ecm.ecm(1009, 20, 0, sigma=7)
    assert plans == ["m2=4,onelaunch", None]


def test_the_command_line_has_the_option(monkeypatch):
    seen = {}

    def fake(*a):
        seen["args"] = a
        return {"factors": [1]}
    monkeypatch.setattr(ecm, "ecm", fake)
    assert ecm.main(["1009", "50", "--onelaunch", "--lanes", "3"]) == 0 and seen["args"][-2:] == (3, True)
    assert ecm.main(["1009", "50"]) == 0 and seen["args"][-2:] == (1, False)
