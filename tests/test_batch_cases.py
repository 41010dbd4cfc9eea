"""Host side of the batch tests (no GPU): every case of batch_cases.py pins what it says it pins, by the shape rule itself (plan.hpp
onelaunch_shape through tests/host/onelaunch_shape.cpp) and its restatement (onelaunch_cases.shape) side by side; the three symbols of
include/mi355_batch.h through header, binding and library."""
import ctypes
import os
import re
import subprocess
import tempfile

import pytest

import batch_cases as bc
import onelaunch_cases as oc
from prmers_amd import engine as E
from prmers_amd.engine import resolve_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def shapes():
    exe = os.path.join(tempfile.mkdtemp(), "onelaunch_shape")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "prmers_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "onelaunch_shape.cpp")])
    lines = subprocess.check_output([exe] + ["%d:%d%s" % (p, lanes, ":" + spec if spec else "") for p, spec, lanes in bc.CASES]).decode().splitlines()
    assert len(lines) == len(bc.CASES)
    return {case: {k: int(v) for k, v in (t.split("=") for t in line.split())} for case, line in zip(bc.CASES, lines)}


def test_the_restated_rule_is_the_rule_for_every_case(shapes):
    assert len(bc.CASES) == len(set(bc.CASES)) == 9 and set(bc.PINS) == set(bc.CASES)
    for (p, spec, lanes), f in shapes.items():
        g = oc.fields(resolve_plan(p, oc.token(spec, lanes)))
        assert (g["n"], g["m1"], g["m2"], g["c"]) == (f["n"], f["m1"], f["m2"], f["c"]) and f["n"] <= oc.MAX_N
        assert (f["tl"], f["k"], f["groups"], f["lds"]) == oc.shape(f["n"], lanes), (p, spec, lanes)
        assert f["k"] * f["tl"] <= 1024 and f["lds"] <= oc.LDS_BYTES and f["c"] >= 2
        assert oc.register_bytes(f["n"], lanes) < oc.BUDGET_BYTES
        # what a copy inside a batch relies on: a lane's digits are a whole number of 16-byte pieces
        assert (4 * f["n"]) % 16 == 0


def claim(name, case, f):
    p, spec, lanes = case
    tiles, runs = f["m2"] // f["c"], f["m1"] * (f["m2"] // f["c"])
    return {
        "dead_lane_inside_the_only_group": lambda: (f["k"], f["groups"]) == (4, 1) and lanes == 3,
        "tail_group_of_one_live_lane": lambda: f["k"] == 8 and f["groups"] == 2 and lanes == f["k"] + 1,
        "lane_is_a_group_of_256_threads": lambda: (f["tl"], f["k"]) == (256, 1) and f["groups"] == lanes,
        "lane_is_a_group_of_1024_threads": lambda: (f["tl"], f["k"]) == (1024, 1) and f["groups"] == lanes,
        "bare_radix5": lambda: f["r5"] == 5 and f["m1"] == 5,
        "radix5_with_a_power_of_two_part": lambda: f["r5"] == 5 and f["m1"] > 5 and f["m1"] % 5 == 0,
        "largest_size": lambda: p == oc.LARGEST_P and f["n"] == oc.MAX_N and f["lds"] == 128 * 1024 and f["sum_fast"] == 0,
        # more tiles than column teams, and more runs than the lane has threads: two trips through the column phases and the run-wise loop
        "a_team_makes_two_trips": lambda: tiles > f["tl"] // f["r5"] and runs > f["tl"],
        "runs_of_four_digits": lambda: f["c"] == 2,
    }[name]()


def test_every_case_pins_what_it_says(shapes):
    for case, f in shapes.items():
        assert claim(bc.PINS[case], case, f), (case, bc.PINS[case], f)
    assert len(set(bc.PINS.values())) == len(bc.CASES)
    # the other cases fuse mul_sum into one product; between them the cases have groups of several lanes and of one
    assert any(f["sum_fast"] == 1 for f in shapes.values())
    assert any(f["k"] > 1 for f in shapes.values()) and any(f["k"] == 1 for f in shapes.values())
    for p in bc.BIT_FOR_BIT_EXPONENTS + (bc.CAPACITY_EXPONENT,):
        assert "onelaunch" in resolve_plan(p, "onelaunch")
    assert {p for pair in bc.NEIGHBOURS for p in pair} == {oc.LARGEST_P, 127}


def test_batch_symbols_are_declared_bound_and_exported_and_stay_out_of_the_engine_header():
    header = open(os.path.join(ROOT, "include", "mi355_batch.h")).read()
    declared = sorted(set(re.findall(r"\b(mi355_batch_[a-z0-9_]+)\s*\(", header)))
    assert declared == sorted(E.BATCH_EXPORTS) == ["mi355_batch_begin", "mi355_batch_end", "mi355_batch_stats"]
    lib = ctypes.CDLL(E.LIB_PATH)
    for name in declared:
        getattr(lib, name)
    engine_header = open(os.path.join(ROOT, "include", "mi355_engine.h")).read()
    assert "mi355_batch_" not in engine_header and not set(declared) & set(E.EXPORTS + E.LANE_EXPORTS)
    for name in declared:
        assert "chain" not in name and "coop" not in name
    L = E.load_library()
    assert L.mi355_batch_begin(None) == 0 and b"null" in L.mi355_engine_last_error()
    assert L.mi355_batch_end(None) == 0 and L.mi355_batch_stats(None, (ctypes.c_uint64 * 4)()) == 0
    capi = open(os.path.join(ROOT, "prmers_amd", "csrc", "capi.cpp")).read()
    for name in declared:
        assert re.search(r"\b%s\(" % name, capi)
