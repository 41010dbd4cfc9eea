"""Several engines alive in one process on one device: what `launch.run_sharded(per_gpu=2)` does to the library.  The engines share
process-wide state that depends on the plan of whichever was constructed last -- configure_kernels / configure_split set the dynamic-LDS
attribute of the generic kernels to the constructing engine's own sizes (kernels.hip) -- and the constructors run with no lock.  Part A
creates and uses two engines in turn on one thread, in both orders, on the smallest shapes at which that state differs; part B drives
two and three engines from threads that construct them at the same moment.  Every value read is compared with Python integers.
(When these tests were written every case passed on an MI355X as the library stood: a kernel whose attribute a later engine had set to
64 KiB still launched with 128 KiB of dynamic LDS, as the HIP header's remark that AMD devices ignore the attribute suggests.  The
tests pin that; should a runtime start to enforce the attribute, configure_kernels / configure_split have to keep a running maximum.)
Lane engines (plan token lanes=B) launch the same generic kernels with the lanes as grid.y and set the same attribute; they appear in both parts, beside a
plain engine of the same plan and beside a lane engine of another tile size and lane count, and run the program of lane_program.py, every
lane compared with its integer model.
One engine used from two threads is not a supported pattern and is not tested.
Needs a real MI355X:  python -m pytest tests -m gpu"""
import threading
import time

import numpy as np
import pytest

import orc
from lane_program import OUT_REGS, REGS, expected_of, inputs, mulmod, run_program

pytestmark = pytest.mark.gpu

SWITCHES = ("MI355_KERNELS", "MI355_TUNE", "MI355_HOST_CARRY", "MI355_CRT_KERNELS", "MI355_CRT_TUNE")
CRT_9941 = "crt-hip:n=288:odd=9:m=32:h1=1:h2=16:generic"


def G(p, plan, text):
    """a first-family engine of four registers whose plan must read `text`"""
    def make():
        from prmers_amd import Engine
        e = Engine(p, 4, plan=plan)
        assert e.describe() == text, (p, plan, e.describe())
        return e
    make.p = p
    return make


def CRT(p, odd, text):
    def make():
        from prmers_amd import CrtEngine
        e = CrtEngine(p, odd, reg_count=4)
        assert e.describe() == text, (p, odd, e.describe())
        return e
    make.p = p
    return make


def L(p, plan, lanes):
    """an engine of REGS registers and `lanes` lanes (1: a plain engine) that runs the program of lane_program.py"""
    def make():
        from prmers_amd import Engine
        from prmers_amd.engine import resolve_plan
        e = Engine(p, REGS, plan=plan, lanes=lanes)
        assert e.lanes == lanes and e.describe() == resolve_plan(p, plan) + (":lanes=%d" % lanes if lanes > 1 else ""), (p, plan, lanes, e.describe())
        return e
    make.p, make.lanes = p, lanes
    make.inputs = inputs(p, lanes=lanes)
    return make


def set_switches(monkeypatch, **values):
    for name in SWITCHES:
        if name in values: monkeypatch.setenv(name, values[name])
        else: monkeypatch.delenv(name, raising=False)


def residue(p, seed):
    rng = np.random.default_rng([p, seed])
    return int.from_bytes(rng.bytes((p + 7) // 8), "little") % ((1 << p) - 1)


def red(v, p):
    return orc.mers_reduce(v + ((1 << p) - 1) if v < 0 else v, p)


# ---- A: created and used in turn on one thread -------------------------------------------------------------------------------

# what they share -> (MI355_KERNELS, first, second); each pair runs in both orders
PAIRS = {
    "generic rows, LDS 128 KiB vs 64 KiB": ("generic", G(300007, "m2=8192", "marin-hip:n=16384:m1=1:m2=8192:c=16"),
                                            G(300007, "m2=4096", "marin-hip:n=16384:m1=2:m2=4096:c=16")),
    "generic columns, LDS 128 KiB vs 80 KiB": ("generic", G(300007, "m2=8,c=8", "marin-hip:n=16384:m1=1024:m2=8:c=8"),
                                               G(400063, "m2=8,c=4", "marin-hip:n=20480:m1=1280:m2=8:c=4")),
    "split sweeps, LDS 128 KiB vs 64 KiB": (None, G(3200123, "m2=8,split5", "marin-hip:n=163840:m1=10240:m2=8:c=1:split5"),
                                            G(1600589, "m2=8,split5", "marin-hip:n=81920:m1=5120:m2=8:c=1:split5")),
    "same exponent, different kernel sets and tables": (None, G(300007, "m2=4096", "marin-hip:n=16384:m1=2:m2=4096:c=16"),
                                                        G(300007, "m2=8,c=4", "marin-hip:n=16384:m1=1024:m2=8:c=4")),
    "same kernels, different exponent": (None, G(300007, "m2=4096", "marin-hip:n=16384:m1=2:m2=4096:c=16"),
                                         G(301447, "m2=4096", "marin-hip:n=16384:m1=2:m2=4096:c=16")),
    "both families": (None, G(9941, None, "marin-hip:n=512:m1=8:m2=32:c=4"), CRT(9941, 9, CRT_9941)),
    # lane engines: an 80 KiB column tile beside the plain engine of the same plan (radix-5 resident columns), and beside a lane engine of
    # another tile size (20 KiB) and lane count
    "lanes beside a plain engine of the same plan": (None, L(1600589, "m2=32,c=4", 2), L(1600589, "m2=32,c=4", 1)),
    "lanes beside lanes, LDS 80 KiB vs 20 KiB": (None, L(1600589, "m2=32,c=4", 2), L(3021377, None, 5)),
}


def check_program(e, want, what):
    for l in range(e.lanes):
        for r in OUT_REGS:
            assert e.get_int(r, lane=l) == want[l][r], (what, e.p, "lane", l, "register", r)


def program_in_turn(make_first, make_second):
    """in_turn for engines that run the program of lane_program.py (with lanes, or lane 0 of a plain engine)"""
    pf = make_first.p
    want_first, want_second = expected_of(pf, make_first.inputs), expected_of(make_second.p, make_second.inputs)
    first = make_first()
    try:
        run_program(first, make_first.inputs)
        second = make_second()          # the process-wide attributes are now the second engine's
        try:
            run_program(second, make_second.inputs)
            check_program(second, want_second, "second engine")
            # back on the first one, with the second alive: what it holds, then both row modes and a back sweep with a copy
            check_program(first, want_first, "first engine, second alive")
            first.square_mul_copy(0, 1, 3)
            first.mul(4, 3)
            y = [v[1] for v in make_first.inputs]
            for l in range(first.lanes):
                sq = mulmod(pf, want_first[l][0], want_first[l][0], 3)
                assert first.get_int(0, lane=l) == first.get_int(1, lane=l) == sq, ("first engine, squared", "lane", l)
                assert first.get_int(4, lane=l) == mulmod(pf, want_first[l][4], y[l]), ("first engine, multiplied", "lane", l)
            check_program(second, want_second, "second engine, after the first ran")
        finally:
            second.close()
        first.square_mul(5)
        for l in range(first.lanes):
            assert first.get_int(5, lane=l) == mulmod(pf, want_first[l][5], want_first[l][5]), ("first engine, second closed", "lane", l)
    finally:
        first.close()


def in_turn(make_first, make_second):
    pf, ps = make_first.p, make_second.p
    first = make_first()
    try:
        x = residue(pf, 1)
        first.set_int(0, x)
        for _ in range(2):
            first.square_mul(0); x = red(x * x, pf)
        second = make_second()          # the process-wide attributes are now the second engine's
        try:
            y, z = residue(ps, 2), residue(ps, 3)
            second.set_int(0, y)
            second.square_mul(0, 3); y = red(red(y * y, ps) * 3, ps)
            second.set_int(1, z)
            second.set_multiplicand(2, 1)
            second.mul(0, 2); y = red(y * z, ps)
            assert second.get_int(0) == y, "second engine"
            # back on the first one, with the second alive
            w = residue(pf, 4)
            first.square_mul(0); x = red(x * x, pf)
            first.sub(0, 2); x = red(x - 2, pf)
            first.square_mul(0); x = red(x * x, pf)
            first.set_int(1, w)
            first.set_multiplicand(2, 1)
            first.mul(0, 2); x = red(x * w, pf)
            first.copy(3, 0)
            assert first.is_equal(0, 3)            # (the canonical-form buffers are allocated here, lazily)
            first.set_int(1, w)
            assert not first.is_equal(0, 1)
            assert first.res64(0) == x & 0xFFFFFFFFFFFFFFFF, "res64 of the first engine"
            assert first.get_int(0) == x, "first engine, second alive"
            assert second.res64(0) == y & 0xFFFFFFFFFFFFFFFF and second.get_int(0) == y, "second engine, after the first ran"
        finally:
            second.close()
        first.square_mul(0); x = red(x * x, pf)
        assert first.get_int(0) == x, "first engine, second closed"
    finally:
        first.close()


@pytest.mark.parametrize("order", ["first-then-second", "second-then-first"])
@pytest.mark.parametrize("shared", list(PAIRS))
def test_two_engines_created_and_used_in_turn(shared, order, monkeypatch):
    kernels, a, b = PAIRS[shared]
    set_switches(monkeypatch, **({"MI355_KERNELS": kernels} if kernels else {}))
    t0 = time.time()
    turn = program_in_turn if hasattr(a, "lanes") else in_turn
    turn(a, b) if order == "first-then-second" else turn(b, a)
    print("in turn, %s, %s: %.2f s" % (shared, order, time.time() - t0))


# ---- B: driven from threads at once ---------------------------------------------------------------------------------------------

ROUNDS, PER_ROUND = 40, 5


def chain_model(p, seed):
    """x0 and, after every tenth round of PER_ROUND squarings, the value: the last one is what get_int reads"""
    x0 = residue(p, seed)
    x, marks = x0, []
    for r in range(ROUNDS):
        for _ in range(PER_ROUND):
            x = red(x * x, p)
        if r % 10 == 9:
            marks.append(x)
    return x0, marks


def run_threads(targets, timeout=120):
    """every target(i) on a thread of its own, released together; exceptions are re-raised here, a thread left alive fails"""
    barrier = threading.Barrier(len(targets))
    errors = []

    def body(i, fn):
        try:
            barrier.wait(timeout=60)
            fn(i)
        except BaseException as exc:   # noqa: B902 -- collected for the main thread
            errors.append((i, exc))
    threads = [threading.Thread(target=body, args=(i, fn), daemon=True) for i, fn in enumerate(targets)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=timeout)
    assert not [i for i, t in enumerate(threads) if t.is_alive()], "a thread is still running after %d s" % timeout
    if errors:
        raise AssertionError("thread %d: %r" % errors[0]) from errors[0][1]


def chain_on(make, x0, marks, own_error=None):
    """the engine is constructed here, on the calling thread, after the barrier: the constructors overlap"""
    def fn(i):
        with make() as e:
            e.set_int(0, x0)
            seen = 0
            for r in range(ROUNDS):
                e.square_mul_n(0, PER_ROUND)
                if r % 10 == 9:
                    want = marks[seen]; seen += 1
                    assert e.res64(0) == want & 0xFFFFFFFFFFFFFFFF, (i, r)
                    e.copy(1, 0)
                    assert e.is_equal(0, 1), (i, r)
                    if own_error:
                        own_error(e)
            assert e.get_int(0) == marks[-1], i
            assert e.get_int(1) == marks[-1], i
    return fn


PROGRAM_ROUNDS = 8


def program_on(make, want):
    """chain_on for an engine that runs the program of lane_program.py: PROGRAM_ROUNDS times, every lane checked after each"""
    def fn(i):
        with make() as e:
            for r in range(PROGRAM_ROUNDS):
                run_program(e, make.inputs)
                check_program(e, want, "thread %d, round %d" % (i, r))
    return fn


P4096 = G(300007, "m2=4096", "marin-hip:n=16384:m1=2:m2=4096:c=16")
THREADED = {
    "the same exponent and plan twice": [P4096, P4096],
    "300007 m2=4096 with m2=1024": [P4096, G(300007, "m2=1024", "marin-hip:n=16384:m1=8:m2=1024:c=4")],
    "radix-8 with radix-5 columns": [G(300007, "m2=8,c=4", "marin-hip:n=16384:m1=1024:m2=8:c=4"), G(400063, "m2=8,c=4", "marin-hip:n=20480:m1=1280:m2=8:c=4")],
    "both families": [G(9941, None, "marin-hip:n=512:m1=8:m2=32:c=4"), CRT(9941, 9, CRT_9941)],
    "three threads": [G(9941, None, "marin-hip:n=512:m1=8:m2=32:c=4"), G(9949, None, "marin-hip:n=512:m1=8:m2=32:c=4"),
                      G(11213, None, "marin-hip:n=512:m1=8:m2=32:c=4")],
    "a lane engine with a plain engine of its plan": [L(301447, None, 9), L(301447, None, 1)],
}


@pytest.mark.parametrize("case", list(THREADED))
def test_engines_constructed_and_driven_from_threads_at_once(case, monkeypatch):
    set_switches(monkeypatch)
    makers = THREADED[case]
    # the models before the threads start
    if hasattr(makers[0], "lanes"):
        targets = [program_on(m, expected_of(m.p, m.inputs)) for m in makers]
    else:
        models = [chain_model(m.p, 10 + i) for i, m in enumerate(makers)]
        targets = [chain_on(m, x0, marks) for m, (x0, marks) in zip(makers, models)]
    t0 = time.time()
    run_threads(targets)
    print("threads, %s: %.2f s" % (case, time.time() - t0))


def test_a_refused_call_on_one_thread_reports_there_and_disturbs_nobody(monkeypatch):
    """thread 0 computes; thread 1 makes calls that are refused before any launch and must read its own message each time (the last
    error is thread-local in capi.cpp); thread 0 has a refusal of its own every tenth round, with a message thread 1 never causes"""
    from prmers_amd import EngineError
    set_switches(monkeypatch)
    x0, marks = chain_model(300007, 20)
    done = threading.Event()

    def own_error(e):
        with pytest.raises(EngineError, match="not a multiplicand"):
            e.mul(0, 1)

    def compute(i):
        try:
            chain_on(P4096, x0, marks, own_error)(i)
        finally:
            done.set()

    def refused(i):
        y = residue(300007, 21)
        with P4096() as e:
            e.set_int(0, y)
            e.set_int(1, y)
            e.set_multiplicand(1, 1)
            calls = [(lambda: e.square_mul(4), "register index out of range"), (lambda: e.square_mul(0, 0), "factor must be >= 1"),
                     (lambda: e.square_mul(1), "holds a multiplicand image")]
            turns = 0
            while turns < 30 or (not done.is_set() and turns < 100000):
                for call, message in calls:
                    with pytest.raises(EngineError, match=message):
                        call()
                turns += 1
            assert e.get_int(0) == y      # a refused call changes nothing

    run_threads([compute, refused])
