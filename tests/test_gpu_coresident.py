"""Several engines alive in one process on one device: what `launch.run_sharded(per_gpu=2)` does to the library.  The engines share
process-wide state that depends on the plan of whichever was constructed last -- configure_kernels / configure_split set the dynamic-LDS
attribute of the generic kernels to the constructing engine's own sizes (kernels.hip) -- and the constructors run with no lock.  Part A
creates and uses two engines in turn on one thread, in both orders, on the smallest shapes at which that state differs; part B drives
two and three engines from threads that construct them at the same moment.  Every value read is compared with Python integers.
(When these tests were written every case passed on an MI355X as the library stood: a kernel whose attribute a later engine had set to
64 KiB still launched with 128 KiB of dynamic LDS, as the HIP header's remark that AMD devices ignore the attribute suggests.  The
tests pin that; should a runtime start to enforce the attribute, configure_kernels / configure_split have to keep a running maximum.)
One engine used from two threads is not a supported pattern and is not tested.
Needs a real MI355X:  python -m pytest tests -m gpu"""
import threading
import time

import numpy as np
import pytest

import orc

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
}


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
    in_turn(a, b) if order == "first-then-second" else in_turn(b, a)
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


P4096 = G(300007, "m2=4096", "marin-hip:n=16384:m1=2:m2=4096:c=16")
THREADED = {
    "the same exponent and plan twice": [P4096, P4096],
    "300007 m2=4096 with m2=1024": [P4096, G(300007, "m2=1024", "marin-hip:n=16384:m1=8:m2=1024:c=4")],
    "radix-8 with radix-5 columns": [G(300007, "m2=8,c=4", "marin-hip:n=16384:m1=1024:m2=8:c=4"), G(400063, "m2=8,c=4", "marin-hip:n=20480:m1=1280:m2=8:c=4")],
    "both families": [G(9941, None, "marin-hip:n=512:m1=8:m2=32:c=4"), CRT(9941, 9, CRT_9941)],
    "three threads": [G(9941, None, "marin-hip:n=512:m1=8:m2=32:c=4"), G(9949, None, "marin-hip:n=512:m1=8:m2=32:c=4"),
                      G(11213, None, "marin-hip:n=512:m1=8:m2=32:c=4")],
}


@pytest.mark.parametrize("case", list(THREADED))
def test_engines_constructed_and_driven_from_threads_at_once(case, monkeypatch):
    set_switches(monkeypatch)
    makers = THREADED[case]
    models = [chain_model(m.p, 10 + i) for i, m in enumerate(makers)]     # before the threads start
    t0 = time.time()
    run_threads([chain_on(m, x0, marks) for m, (x0, marks) in zip(makers, models)])
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
