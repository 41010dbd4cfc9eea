"""The case list of the wide lane tests (lane_cases.py) stays complete: every tile whose work-group size a lane count changes appears with
lane counts on both sides of its switch, the thread shapes only a lane engine reaches are all reached, the lane counts ECM is meant to
run at occur at small exponents, and no case needs more than 1 GiB of registers.  The grids come from resolve_plan, the thread counts
from the restated rule (kernels.hip block_for_small): if that rule changes, this says which cases to move.  CPU only."""
import os
import subprocess
import tempfile

import pytest

import lane_cases as lc
from prmers_amd.engine import resolve_plan


def grid(p, spec):
    return lc.grid_of(resolve_plan(p, spec))


def lanes_of(p, spec):
    return sorted(b for q, s, b in lc.CASES if (q, s) == (p, spec))


def test_the_list_has_no_duplicates_and_resolves():
    assert len(lc.CASES) == len(set(lc.CASES))
    for p, spec, lanes in lc.CASES:
        n, m1, m2, c = grid(p, spec)
        assert n == 2 * m1 * m2 and m2 % c == 0 and 1 < lanes < 65536
        assert resolve_plan(p, (spec + "," if spec else "") + "lanes=%d" % lanes) == resolve_plan(p, spec) + ":lanes=%d" % lanes


@pytest.mark.parametrize("p, spec, sweep, pairs, groups, low, high", lc.TABLE, ids=["%d-%s" % (r[0], r[2]) for r in lc.TABLE])
def test_every_row_of_the_table_has_lane_counts_on_both_sides_of_its_switch(p, spec, sweep, pairs, groups, low, high):
    n, m1, m2, c = grid(p, spec)
    assert lc.sweeps(m1, m2, c)[sweep] == (pairs, groups)
    last_below = lc.GROUP_SWITCH // groups                      # the largest B with B x groups <= 256
    assert last_below * groups <= lc.GROUP_SWITCH < (last_below + 1) * groups
    have = lanes_of(p, spec)
    assert last_below in have, "%d %s: no case at %d lanes, the last count below the switch (have %s)" % (p, sweep, last_below, have)
    assert last_below + 1 in have, "%d %s: no case at %d lanes, the first count beyond the switch (have %s)" % (p, sweep, last_below + 1, have)
    assert lc.threads(pairs, groups, 1) == lc.threads(pairs, groups, last_below) == low
    assert lc.threads(pairs, groups, last_below + 1) == lc.threads(pairs, groups, max(have)) == high
    assert low != high                                          # the single-lane engine of this shape never runs `high`


def test_the_thread_shapes_only_lanes_reach_are_all_reached():
    lanes_only = set()
    for p, spec, lanes in lc.CASES:
        n, m1, m2, c = grid(p, spec)
        for pairs, groups in lc.sweeps(m1, m2, c).values():
            t = lc.threads(pairs, groups, lanes)
            if t != lc.threads(pairs, groups, 1):
                lanes_only.add((pairs, t))
    assert lc.SHAPES_BEYOND <= lanes_only, lc.SHAPES_BEYOND - lanes_only


def test_the_restated_rule_at_its_edges():
    assert [lc.block_for(w) for w in (0, 1, 64, 65, 128, 129, 511, 512, 513, 5000)] == [64, 64, 64, 128, 128, 256, 512, 512, 512, 512]
    assert [lc.threads(pairs, 1, 1) for pairs in (4, 64, 65, 320, 1024, 1280, 5120)] == [64, 64, 128, 512, 1024, 1024, 1024]
    assert lc.threads(128, 64, 4) == 128 and lc.threads(128, 64, 5) == 64       # 256 groups is still the first form
    assert lc.threads(4, 1, 512) == 64                                           # a tile of fewer than four pairs


def test_the_lane_counts_ecm_runs_at_occur_at_small_exponents():
    for count in lc.SMALL_LANE_COUNTS:
        assert [p for p, spec, lanes in lc.CASES if lanes == count and p <= lc.SMALL_P], count


def test_no_case_needs_more_than_a_gibibyte_of_registers():
    for p, spec, lanes in lc.CASES:
        n = grid(p, spec)[0]
        assert lc.register_bytes(n, lanes) <= lc.BUDGET_BYTES, (p, spec, lanes, lc.register_bytes(n, lanes))


def test_the_large_factors_are_above_the_fused_bound_of_their_plans():
    """a_fast from the plan itself (tests/host/plan_query.cpp)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(tempfile.mkdtemp(), "plan_query")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(root, "prmers_amd", "csrc"), "-o", exe,
                           os.path.join(root, "tests", "host", "plan_query.cpp")])
    shapes = sorted(lc.A_FAST, key=str)
    lines = subprocess.check_output([exe] + ["%d%s" % (p, ":" + s if s else "") for p, s in shapes]).decode().splitlines()
    for (p, spec), line in zip(shapes, lines):
        f = dict(t.split("=") for t in line.split())
        assert int(f["p"]) == p and int(f["a_fast"]) == lc.A_FAST[(p, spec)], line
    assert {(p, s) for p, s, _, _ in lc.FACTOR_CASES} == set(lc.A_FAST)
    for p, spec, lanes, a in lc.FACTOR_CASES:
        assert lc.SMALL_FACTOR <= lc.A_FAST[(p, spec)] < a < 2**32 and lanes > 1
    assert min(a for _, _, _, a in lc.FACTOR_CASES) == 16       # one past the bound of runs of two digits
