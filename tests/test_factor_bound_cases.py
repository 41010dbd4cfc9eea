"""The fused factor bound against the exact chain (no GPU): chain_model.py against plain integers, then everything that
test_gpu_factor_bound.py runs through it -- every coefficient below the field prime, every 64-bit term of every carry chain and carry-in
below 2^64, every digit a front sweep doubles below 2^31 -- so that a failure on the GPU is a kernel's fault and not an input outside
the design.  Also: how close to 2^64 the cases are, the first factor at which the exact chain does overflow, the input class that the
bound does NOT cover (2^(q+1) - 1 on every digit), and the exponents of the 5 2^odd sizes in the case list."""
import os
import random
import subprocess
import tempfile

import pytest

import chain_model as cm
import factor_bound_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prmers_amd", "csrc")
IDS = [fc.case_id(c) for c in fc.CASES]


@pytest.fixture(scope="module")
def plan_query():
    exe = os.path.join(tempfile.mkdtemp(), "plan_query")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "host", "plan_query.cpp")])

    def run(*args):
        return subprocess.check_output([exe, *map(str, args)]).decode().splitlines()
    return run


def _fields(line):
    return dict(t.split("=") for t in line.split() if t.count("=") == 1 and ":" not in t)


def _configs():
    """the distinct (p, n, C, a_fast, fused back sweep) of the cases: all the model depends on"""
    seen = {}
    for c in fc.CASES:
        seen.setdefault((c.p, c.n, c.c, c.a_fast, fc.fused_back(c)), c)
    return list(seen.values())


CONFIGS = _configs()
CONFIG_IDS = ["%d-n%d-c%d" % (c.p, c.n, c.c) for c in CONFIGS]
CONFIG_PARAMS = [pytest.param(c, id=i, marks=[pytest.mark.slow] if c.n >= 16384 else []) for c, i in zip(CONFIGS, CONFIG_IDS)]
_memo = {}           # (p, n, C) -> the products already computed, shared by the tests below
_all_max = {}        # (p, n) -> the coefficients of (2^p - 2)^2
_traced = {}         # the cases already traced, for the cases that differ in their kernels alone


def all_max_coefficients(p, n):
    if (p, n) not in _all_max:
        x = cm.to_digits(p, n, (1 << p) - 2)
        _all_max[p, n] = cm.coefficients_fast(p, n, x, x)
    return _all_max[p, n]


def overflows(s):
    return max(s.max_r, s.max_carry) >= cm.LIM


def first_overflow(p, n, C, z, addend=None):
    """the first factor whose exact chain over z leaves 64 bits (the terms rise with the factor), None: none below 2^32"""
    if not overflows(cm.back_sweep(p, n, C, z, 2**32 - 1, addend)):
        return None
    lo, hi = 1, 2**32 - 1
    while lo < hi:
        mid = (lo + hi) // 2
        if overflows(cm.back_sweep(p, n, C, z, mid, addend)):
            hi = mid
        else:
            lo = mid + 1
    return lo


# ---- the list itself ----

def test_the_list_is_what_the_plans_say(plan_query):
    assert len(set(fc.CASES)) == len(fc.CASES) == len(set(IDS))
    lines = plan_query(*["%d:%s" % (c.p, fc.token(c)) for c in fc.CASES])
    kinds = plan_query(*["k:%d:%s%s" % (c.p, fc.token(c), "@" + c.kernels if c.kernels else "") for c in fc.CASES])
    for c, line, kind in zip(fc.CASES, lines, kinds):
        f, k = _fields(line), _fields(kind)
        assert (int(f["p"]), int(f["n"]), int(f["c"]), int(f["a_fast"])) == (c.p, c.n, c.c, c.a_fast), (c, line)
        assert (k["cols"], k["rows"]) == (c.cols, c.rows) and int(k["split5"]) == (c.cols == "split"), (c, kind)
        assert 2 <= len(fc.factors(c)) <= 3 and (c.a_fast + 1 in fc.factors(c)) == (c.a_fast < 2**32 - 1)
        assert not c.onelaunch or c.n <= 8192
    got = {(c.cols, c.rows) for c in fc.PLAIN}
    assert {c for c, _ in got} >= {"generic", "split", "radix8-1024", "radix4-planes", "radix5-1280", "radix5-2560"}
    assert {r for _, r in got} >= {"generic", "radix4-planes", "rows2048-one", "rows4096", "rows8192"}
    assert any(c.kernels == "generic" and c.cols == "generic" for c in fc.PLAIN)
    assert sum(c.a_fast == 2**32 - 1 for c in fc.ONELAUNCH) == 2


def test_the_exponents_are_the_tops_of_their_ranges(plan_query):
    """every case but the two 5 2^odd ones sits on the last exponent of its size (the two with a_fast = 2^32 - 1 are there for their
    narrow digits, q = 16 and q = 19, not for the edge)"""
    wide_carry = {132049, 9941}
    tops = [c for c in fc.CASES if c.p not in (fc.P_40960, fc.P_2560) and c.p not in wide_carry]
    for c, line in zip(tops, plan_query(*["ts:%d" % (c.p + 1) for c in tops])):
        assert int(_fields(line)["n"]) > c.n, (c, line)
    for p, q in ((132049, 16), (9941, 19)):
        assert [c.p // c.n for c in fc.CASES if c.p == p] == [q]


def test_every_kind_of_operand_is_on_some_lane_and_lanes_differ():
    for c in fc.CASES:
        rs = fc.rounds(c)
        assert {k for r in rs for k, _, _, _ in r} == set(range(len(fc.KINDS))), c
        mp = (1 << c.p) - 1
        for r in rs:
            assert len(r) == c.lanes and all(0 <= v <= mp for lane in r for v in lane[1:])
            assert len({lane[1:] for lane in r}) == len(r), c            # no two lanes of a round with the same operands
            assert all(z in (mp, mp - 1) for _, _, _, z in r)             # the addend: all-maximum


# ---- (a) the model against plain integers ----

@pytest.mark.parametrize("c", CONFIG_PARAMS)
def test_value_identity(c):
    p, n, C = c.p, c.n, c.c
    mp = (1 << p) - 1
    rng = random.Random(p + C)
    edge = [mp - 1, mp, mp - 1 - (1 << (p // 3)), 0, 1]
    pairs = [(rng.getrandbits(p - 1), rng.getrandbits(p - 1), rng.getrandbits(p - 1), rng.randrange(1, 2**32)) for _ in range(2)]
    pairs += [(edge[i], edge[(i + 1) % 5], edge[(i + 2) % 5], a) for i, a in enumerate((c.a_fast, 1, max(1, c.a_fast - 1), 2**32 - 1, 3))]
    pairs += [(mp - 1, mp - 1, None, c.a_fast), (mp, mp, mp, c.a_fast)]
    for x, y, z, a in pairs:
        xd, yd = cm.to_digits(p, n, x), cm.to_digits(p, n, y)
        ad = cm.to_digits(p, n, z) if z is not None else None
        s = cm.back_sweep(p, n, C, cm.coefficients_fast(p, n, xd, yd), a, ad)
        want = fc.red(p, fc.mulmod(p, fc.red(p, x), fc.red(p, y), a) + fc.red(p, z or 0))
        assert cm.value(p, n, C, s.digits, s.carries) == want, (p, C, a)
        t = cm.carry_in(p, n, C, s.digits, s.carries)                      # the carry-in keeps the value
        assert cm.value(p, n, C, t.digits) == want, (p, C, a, "carry-in")


@pytest.mark.parametrize("p, n", [(239, 8), (1159, 40), (2239, 80), (13823, 512), (9941, 512), (1280, 80), (4480, 160)])
def test_the_fast_coefficients_are_the_sums_as_they_are_written(p, n):
    """coefficients(), the O(n^2) sum over the pairs with the weight exponent's carry, against coefficients_fast(); the last two
    exponents share a factor with n (the digit widths repeat with a shorter period)"""
    rng = random.Random(p)
    mp = (1 << p) - 1
    for x, y in ((mp - 1, mp - 1), (mp, mp - 1), (rng.getrandbits(p) % mp, rng.getrandbits(p) % mp)):
        xd, yd = cm.to_digits(p, n, x), cm.to_digits(p, n, y)
        assert cm.coefficients(p, n, xd, yd) == cm.coefficients_fast(p, n, xd, yd)
    big = [rng.randrange(1 << 31) for _ in range(n)]                      # digits as a carry-in may leave them
    assert cm.coefficients(p, n, big, big) == cm.coefficients_fast(p, n, big, big)


@pytest.mark.slow
@pytest.mark.parametrize("p, n", [(102399, 4096), (127999, 5120)])
def test_the_fast_coefficients_at_a_size_of_the_cases(p, n):
    x = cm.to_digits(p, n, (1 << p) - 2)
    y = cm.to_digits(p, n, random.Random(p).getrandbits(p - 1))
    assert cm.coefficients(p, n, x, y) == cm.coefficients_fast(p, n, x, y)


# ---- (b) everything the GPU test runs is inside the design ----

def _trace_case(c):
    """every sequence of test_gpu_factor_bound.py for this case through the model: the Trace over all of them; the model's values are
    compared with the plain integers on the way"""
    memo = _memo.setdefault((c.p, c.n, c.c), {})
    same = (c.p, c.n, c.c, c.a_fast, fc.fused_back(c), c.lanes)                # what the sequences and the model depend on
    if same in _traced:
        return _traced[same]
    total = _traced[same] = cm.Trace()
    for number, lanes in enumerate(fc.rounds(c)):
        for kind, x, y, z in lanes:
            todo = [(entry, a, fc.sequence(entry, a)) for a in fc.factors(c) for entry in fc.ENTRIES if not fc.refused(c, entry, a)]
            todo += [("chain", c.a_fast, fc.chain_ops(c, False))] if number == 0 else []             # the chains: the first round's lanes
            todo += [("chain onto itself", c.a_fast, fc.chain_ops(c, True))] if number == 0 and fc.fused_back(c) else []
            for entry, a, ops in todo:
                m = fc.machine(c, memo)
                for r, v in ((fc.R_X, x), (fc.R_Y, y), (fc.R_ADD, z)):
                    m.set(r, v)
                images = {fc.R_YIMG: m.operand(fc.R_Y)}
                fc.run_model(m, images, ops)
                mp = (1 << c.p) - 1
                want = fc.run_ints(c.p, {fc.R_X: x % mp, fc.R_YIMG: y % mp, fc.R_ADD: z % mp}, ops)
                assert m.get(fc.R_X) == want[fc.R_X], (c, fc.KINDS[kind], entry, a)
                assert m.trace.inside(), (c, fc.KINDS[kind], entry, a, vars(m.trace))
                for k, v in vars(m.trace).items():
                    setattr(total, k, max(getattr(total, k), v))
    return total


@pytest.mark.slow
@pytest.mark.parametrize("c", fc.CASES, ids=IDS)
def test_every_sequence_of_the_gpu_test_is_inside_the_design(c, record_property):
    t = _trace_case(c)
    assert t.max_z < cm.FIELD and max(t.max_r, t.max_carry, t.max_sum) < cm.LIM and t.max_digit < cm.DIGIT_LIM
    record_property("max z / field prime", round(t.max_z / cm.FIELD, 4))
    record_property("max 64-bit term / 2^64", round(max(t.max_r, t.max_carry, t.max_sum) / cm.LIM, 4))
    record_property("max digit after carry-in / 2^31", round(t.max_digit / cm.DIGIT_LIM, 6))


# ---- (c) the cases are at the edge, (d) the first factor that overflows is above a_fast ----

@pytest.mark.parametrize("c", CONFIG_PARAMS)
def test_the_edge_and_the_first_exact_overflow(c, record_property):
    p, n, C = c.p, c.n, c.c
    z = all_max_coefficients(p, n)
    assert max(z) < cm.FIELD
    s = cm.back_sweep(p, n, C, z, c.a_fast)
    assert not overflows(s), (c, s.max_r / cm.LIM, s.max_carry / cm.LIM)
    record_property("carry word at a_fast / 2^64", round(s.max_carry / cm.LIM, 4))
    at_the_top = c.p not in (fc.P_40960, fc.P_2560, 132049, 9941)
    if at_the_top and n >= fc.EDGE_MIN_N and C >= 2:
        assert s.max_carry >= fc.EDGE_FRACTION * cm.LIM, (c, s.max_carry / cm.LIM)
    # with mul_add's all-maximum addend, and with the all-ones words (every digit at its maximum, digit 0 included)
    ones = cm.to_digits(p, n, (1 << p) - 1)
    for zz, ad in ((z, ones), (cm.coefficients_fast(p, n, ones, ones), None), (cm.coefficients_fast(p, n, ones, ones), ones)):
        first = first_overflow(p, n, C, zz, ad)
        assert first is None or first > c.a_fast, (c, first)
    first = first_overflow(p, n, C, z)
    record_property("first factor that overflows", first)
    if C >= 2 and c.a_fast < 2**32 - 1:
        assert first is not None and first > c.a_fast, (c, first)
        assert first < 1.01 * c.a_fast or not at_the_top or n < fc.EDGE_MIN_N, (c, first)    # the bound gives away less than 1 %


# ---- (e) what the bound does not cover ----

@pytest.mark.parametrize("p", fc.ALL_WIDE_OVERFLOWS)
def test_the_wide_maximum_on_every_digit_overflows_at_a_fast(p, plan_query):
    """2^(q+1) - 1 on EVERY digit, the input that the comment on carry_chain_ok used to name as covered: the carry word passes 2^64 at
    a_fast.  Canonical digits (each below 2^w_j of its own width) do not: the bound holds for them and for the run-head excess alone."""
    f = _fields(plan_query(p)[0])
    n, q, C, a = int(f["n"]), int(f["q"]), int(f["c"]), int(f["a_fast"])
    wide = [(1 << (q + 1)) - 1] * n
    s = cm.back_sweep(p, n, C, cm.coefficients_fast(p, n, wide, wide), a)
    assert s.max_carry >= cm.LIM, (p, s.max_carry / cm.LIM)
    canon = cm.back_sweep(p, n, C, all_max_coefficients(p, n), a)
    assert not overflows(canon) and canon.max_z < cm.FIELD, (p, canon.max_carry / cm.LIM)


# ---- the 5 2^odd sizes ----

def _in_field(p, n):
    return max(all_max_coefficients(p, n)) < cm.FIELD


@pytest.mark.slow
@pytest.mark.parametrize("n, p_case", [(2560, fc.P_2560), (40960, fc.P_40960)])
def test_the_exponents_of_the_five_odd_cases_are_the_bisection_s(n, p_case):
    top, first = fc.FIVE_ODD[n]
    assert not _in_field(top, n) and _in_field(first, n)
    lo, hi = first, top
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if _in_field(mid, n):
            lo = mid
        else:
            hi = mid - 1
    assert lo == p_case and _in_field(p_case, n) and not _in_field(p_case + 1, n)


@pytest.mark.parametrize("n", [40, 160, 640, 2560, 10240, 40960])
def test_past_the_field_prime_the_device_value_must_differ(n):
    """at the top of a 5 2^odd range the largest coefficient of (2^p - 2)^2 is 1.2 times the field prime: the device holds it mod the
    prime, and the chain over those words gives another value than 1 (test_gpu_operand_edges' strict xfail holds these sizes)"""
    p = fc.FIVE_ODD[n][0]
    z = all_max_coefficients(p, n)
    assert 1.2 < max(z) / cm.FIELD < 1.25
    s = cm.back_sweep(p, n, 1, [v % cm.FIELD for v in z], 1)   # (the value does not depend on the run length)
    assert cm.value(p, n, 1, s.digits, s.carries) != 1


@pytest.mark.parametrize("n, p", [(80, 2239), (5120, 127999), (20480, 491519)])
def test_the_five_even_sizes_stay_inside_the_field(n, p):
    assert 0.6 < max(all_max_coefficients(p, n)) / cm.FIELD < 0.63
