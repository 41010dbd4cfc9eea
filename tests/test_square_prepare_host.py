"""Host side of square_mul_prepare (no GPU): the symbol through header, binding and adapter, the argument checks of the default
composition in RegisterMachine (a stub machine compiled from tests/host), and the kernels the GPU cases reach."""
import os
import re
import subprocess
import tempfile

import pytest

from mul_sum_cases import CASES, ROW_KERNELS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prmers_amd", "csrc")
NEW = ["mi355_engine_square_mul_prepare", "mi355_engine_square_mul_prepare_is_fused"]


@pytest.fixture(scope="module")
def host_tool():
    td = tempfile.mkdtemp()

    def run(src, *args):
        exe = os.path.join(td, os.path.splitext(src)[0])
        if not os.path.exists(exe):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "host", src)])
        return subprocess.check_output([exe, *map(str, args)]).decode().splitlines()
    return run


def test_exports_equal_the_declared_symbols():
    import prmers_amd.engine as E
    header = open(os.path.join(ROOT, "include", "mi355_engine.h")).read()
    declared = sorted(set(re.findall(r"\b(mi355_(?:engine|crt)_[a-z0-9_]+)\s*\(", header)))
    assert sorted(E.EXPORTS) == declared and len(declared) == 51
    assert "51 symbols" in header
    capi = open(os.path.join(CSRC, "capi.cpp")).read()
    adapter = open(os.path.join(ROOT, "include", "mi355", "engine_hip.h")).read()
    for name in NEW:
        assert name in declared and re.search(r"\bint %s\(" % name, capi) and '"%s"' % name in adapter
    for cls in (E.Engine, E.CrtEngine):
        assert callable(cls.square_mul_prepare) and callable(cls.square_mul_prepare_is_fused)


def test_default_composition_checks_before_it_runs(host_tool):
    assert host_tool("square_prepare_stub.cpp") == ["OK"]


def test_gpu_cases_reach_every_row_kernel(host_tool):
    lines = host_tool("plan_query.cpp", *["k:%d%s" % (p, ":" + s if s else "") for p, s in CASES])
    rows = {dict(t.split("=") for t in l.split()[2:])["rows"] for l in lines}
    assert rows == ROW_KERNELS, rows
