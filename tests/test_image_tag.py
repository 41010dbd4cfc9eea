"""The tag word of a raw register image (plan.hpp layout_tag / register_tag; no GPU): a fingerprint of everything the bytes depend on, so
that set_data can refuse what another layout wrote.  Through tests/host/tag_query.cpp: digits tags are one-to-one with the layouts of
the SMALL_CASES plans, do not move with the switches that leave the layout alone, and an image's tag follows the kernels that define its
form."""
import itertools
import os
import subprocess
import tempfile

import pytest

from test_gpu_parity import SMALL_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prmers_amd", "csrc")
SELECTIONS = [None, "v2", "generic", "v2rows", "v2cols"]


@pytest.fixture(scope="module")
def tag_query():
    exe = os.path.join(tempfile.mkdtemp(), "tag_query")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "host", "tag_query.cpp")])

    def run(args, env=None):
        out = subprocess.check_output([exe, *args], env=dict(os.environ, **(env or {}))).decode().splitlines()
        assert len(out) == len(args)
        rows = []
        for line in out:
            f = dict(t.split("=") for t in line.split()[2:])
            rows.append({k: int(v, 16 if k in ("digits", "image") else 10) for k, v in f.items()})
        return rows
    return run


def arg(p, plan, sel=None):
    return "%d%s%s" % (p, ":" + plan if plan else "", "@" + sel if sel else "")


def layout(r):
    return (r["m1"], r["m2"], r["c"], r["split5"])


def test_a_tag_is_never_the_bare_kind_of_earlier_versions(tag_query):
    for r in tag_query([arg(p, plan) for p, plan in SMALL_CASES]):
        assert r["digits"] & 1 == 0 and r["image"] & 1 == 1          # bit 0: what the register holds
        assert r["digits"] >> 63 == 1 and r["image"] >> 63 == 1      # a fingerprint is never zero
        assert r["digits"] < 1 << 64 and r["image"] < 1 << 64


def test_digits_tags_are_one_to_one_with_the_layouts_of_an_exponent(tag_query):
    rows = tag_query([arg(p, plan) for p, plan in SMALL_CASES])
    by_p = {}
    for (p, plan), r in zip(SMALL_CASES, rows):
        by_p.setdefault(p, []).append((plan, r))
    compared = 0
    for p, group in by_p.items():
        for (pa, a), (pb, b) in itertools.combinations(group, 2):
            assert (a["digits"] == b["digits"]) == (layout(a) == layout(b)), (p, pa, pb)
            assert (a["image"] == b["image"]) == (layout(a) == layout(b)), (p, pa, pb)
            compared += layout(a) != layout(b)
    assert compared >= 60       # the list does hold many plans per exponent (300007 alone has eleven)
    # and across exponents: the size of an image is 8 n + 8 for every exponent of a transform size, so p is part of the tag
    every = {}
    for (p, plan), r in zip(SMALL_CASES, rows):
        assert every.setdefault(r["digits"], (p,) + layout(r)) == (p,) + layout(r), (p, plan)
    a, b = tag_query(["300007:m2=4096", "301447:m2=4096"])
    assert layout(a) == layout(b) and a["digits"] != b["digits"] and a["image"] != b["image"]


def test_switches_that_leave_the_layout_alone_leave_the_tags_alone(tag_query):
    args = [arg(p, plan) for p, plan in SMALL_CASES]
    plain = tag_query(args, env={"MI355_TUNE": "0", "MI355_HOST_CARRY": "0"})
    for env in ({"MI355_TUNE": "1"}, {"MI355_TUNE": "32"}, {"MI355_TUNE": "33", "MI355_HOST_CARRY": "1"}, {"MI355_HOST_CARRY": "1"}):
        assert tag_query(args, env=env) == plain, env


def test_an_image_tag_follows_the_kernels_that_define_its_form(tag_query):
    """MI355_KERNELS never moves a digits tag (the register layout is the plan's).  An image tag is the same exactly where the row kernel
    is (the form of the stored words) and, on a transform with a radix-5 stage, the column kernel too (each has its own order of the
    rows there; the column kernels of a power-of-two transform all leave them bit-reversed)"""
    shapes = [(300007, "m2=4096"), (300007, "m2=8,c=4"), (300007, "m2=1024"), (300007, "m2=8192"), (300007, "m2=2048"), (600011, "m2=2048,c=2"),
              (400063, "m2=8,c=4"), (800283, "m2=8,c=2"), (800283, "m2=16,c=4"), (86243, "m2=8,c=4"), (9941, "m2=16,c=4"),
              (3200123, "m2=4096,split5"), (30402457, "m2=4096"), (9815459, "m2=1024")]
    differing_rows = differing_cols5 = differing_cols2 = 0
    for p, plan in shapes:
        rows = tag_query([arg(p, plan, sel) for sel in SELECTIONS])
        assert len({r["digits"] for r in rows}) == 1 and len({layout(r) for r in rows}) == 1, (p, plan)
        for a, b in itertools.combinations(rows, 2):
            same = a["rows"] == b["rows"] and (a["r5"] == 1 or a["cols"] == b["cols"])
            assert (a["image"] == b["image"]) == same, (p, plan, a, b)
            differing_rows += a["rows"] != b["rows"]
            differing_cols5 += a["r5"] == 5 and a["cols"] != b["cols"] and a["rows"] == b["rows"]
            differing_cols2 += a["r5"] == 1 and a["cols"] != b["cols"] and a["rows"] == b["rows"]
    assert differing_rows >= 20 and differing_cols5 >= 4 and differing_cols2 >= 4      # every kind of difference was met


def test_second_family_tags(tag_query):
    """digits: exponent, size and radix; an image also the row split and the row kernel (crt_engine.hip data_tag)"""
    base, other_p, other_n, other_odd, other_split, generic = tag_query(
        ["crt:1300021:36864:9:1:10:1", "crt:1300027:36864:9:1:10:1", "crt:1300021:73728:9:2:10:1", "crt:1300021:49152:3:3:10:1",
         "crt:1300021:36864:9:2:9:1", "crt:1300021:36864:9:1:10:0"])
    for r in (other_p, other_n, other_odd):
        assert r["digits"] != base["digits"] and r["image"] != base["image"]
    for r in (other_split, generic):      # the digits are in logical order whatever the kernels are; the packed spectrum is not
        assert r["digits"] == base["digits"] and r["image"] != base["image"]
    first = tag_query(["9941"])[0]      # the family is part of the tag: the same exponent and size in the first family
    assert tag_query(["crt:9941:512:1:0:0:0"])[0]["digits"] != first["digits"]
