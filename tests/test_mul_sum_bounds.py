"""Host side of the fused multiply-by-sum (no GPU): the capacity bit plan.sum_fast against a restatement of its worst-case model, the
kernels the GPU cases reach, and gf::add_lazy_any through its host form."""
import os
import subprocess
import tempfile

import pytest

from mul_sum_cases import CASES, ROW_KERNELS, sum_product_ok
from test_operand_bounds import P_MAX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prmers_amd", "csrc")


@pytest.fixture(scope="module")
def host_tool():
    td = tempfile.mkdtemp()

    def run(src, *args):
        exe = os.path.join(td, os.path.splitext(src)[0])
        if not os.path.exists(exe):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "host", src)])
        return subprocess.check_output([exe, *map(str, args)]).decode().splitlines()
    return run


def _fields(line):
    return {k: int(v) for k, v in (t.split("=") for t in line.split())}


def test_sum_fast_matches_the_worst_case_model_at_the_top_of_every_size(host_tool):
    args = []
    for n, p in P_MAX.items():
        args += [p, p - n]          # the largest digit width of the size, and one below
    seen = set()
    for line in host_tool("sum_query.cpp", *args):
        f = _fields(line)
        assert f["p"] in args and f["q"] == f["p"] // f["n"]
        assert bool(f["sum_fast"]) == sum_product_ok(f["q"], f["n"], f["c"]), line
        # the crude form errs on the safe side only: whatever it admits, the model admits
        if 2 * (f["q"] + 1) + 1 + (f["n"].bit_length() - 1) + (1 if f["n"] & (f["n"] - 1) else 0) < 64:
            assert f["sum_fast"] == 1, line
        seen.add(f["sum_fast"])
    assert seen == {0, 1}


def test_sum_fast_of_the_baseline_exponents_and_the_gpu_cases(host_tool):
    lines = host_tool("sum_query.cpp", 9815459, 136279841, 205271257, *["%d:%s" % (p, s) if s else p for p, s in CASES])
    got = [_fields(l) for l in lines]
    # crude form 2 (q + 1) + 1 + log2 n: 59 at C2 (q = 18, n = 2^19), 58 at C3 (q = 16, n = 2^23), 64.3 at C4 (q = 19, n = 5 2^21)
    assert [g["sum_fast"] for g in got[:3]] == [1, 1, 0]
    for g in got:
        assert bool(g["sum_fast"]) == sum_product_ok(g["q"], g["n"], g["c"]), g
    assert {g["sum_fast"] for g in got[3:]} == {0, 1}   # the GPU cases run both paths of mul_sum


def test_gpu_cases_reach_every_row_kernel(host_tool):
    lines = host_tool("plan_query.cpp", *["k:%d%s" % (p, ":" + s if s else "") for p, s in CASES])
    rows = {dict(t.split("=") for t in l.split()[2:])["rows"] for l in lines}
    assert rows == ROW_KERNELS, rows


def test_lazy_sum_primitive_on_the_host(host_tool):
    assert host_tool("test_lazy_sum.cpp") == ["OK"]
