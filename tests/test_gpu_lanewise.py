"""Lane-wise reads (include/mi355_lanewise.h; canon.hip with the lanes as grid.y): equal_lanes and get_ints on every lane of an engine in one
launch sequence per chunk of lanes, against the per-lane reads get_int(lane=l) as Python integers.  Pairs that are the same residue in
different digits (pending run carries, sums in either order, x - x and 2^p - 1 against 0, a carry that ripples through every digit), pairs
that differ in one lane only, the host-carry engine, engines without lanes, batches, every refusal, and more lanes than one chunk.
Needs a real MI355X:  python -m pytest tests -m gpu"""
import ctypes as C
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LANES = 9
# (p, onelaunch): n = 64 (one partial scan block), 512, 8192 (two scan blocks), 5 * 2^11, 2^14 (three launches only above p = 204799)
CASES = [(1277, False), (1277, True), (9941, False), (9941, True), (132049, False), (132049, True), (216091, False), (301447, False)]
(R_A, R_B, R_C, R_D, R_I, R_J) = range(6)
REGS = 6


def values(p, count, seed):
    rng = random.Random(seed * 1000003 + p)
    mp = (1 << p) - 1
    return [rng.getrandbits(p) % mp for _ in range(count)]


def put(e, r, vs):
    e.set(r, 0)
    for l, v in enumerate(vs):
        e.set_int(r, v, lane=l)


def all_ones(e):
    return np.frombuffer(((1 << e.p) - 1).to_bytes(e.word_count * 4, "little"), dtype="<u4")


def compare(e, a, b, what):
    """equal_lanes first (the registers as they stand, pending carries included), then both registers lane by lane as integers"""
    out = e.equal_lanes(a, b)
    want = [e.get_int(a, lane=l) == e.get_int(b, lane=l) for l in range(e.lanes)]
    assert out == want, (e.p, what, out, want)
    return out


@pytest.mark.parametrize("p, onelaunch", CASES, ids=["%d%s" % (p, "-onelaunch" if o else "") for p, o in CASES])
def test_equal_lanes_on_pairs_that_are_equal_as_residues_and_on_pairs_that_differ_in_one_lane(p, onelaunch):
    from prmers_amd import Engine
    mp = (1 << p) - 1
    x, y, s, t = (values(p, LANES, k) for k in range(4))
    yes = [True] * LANES
    with Engine(p, REGS, lanes=LANES, onelaunch=onelaunch) as e:
        # x y against y x, both with pending run carries
        put(e, R_A, x); put(e, R_I, y); e.set_multiplicand(R_I, R_I); e.mul(R_A, R_I)
        put(e, R_B, y); put(e, R_J, x); e.set_multiplicand(R_J, R_J); e.mul(R_B, R_J)
        assert compare(e, R_A, R_B, "xy = yx") == yes
        assert e.get_ints(R_A) == [a * b % mp for a, b in zip(x, y)]
        # s + t against t + s
        put(e, R_A, s); put(e, R_C, t); put(e, R_B, t); put(e, R_D, s)
        e.add(R_A, R_C); e.add(R_B, R_D)
        assert compare(e, R_A, R_B, "s + t = t + s") == yes
        # x - x against 0, and 2^p - 1 against 0
        put(e, R_A, x); put(e, R_C, x); e.sub_reg(R_A, R_C); e.set(R_B, 0)
        assert compare(e, R_A, R_B, "x - x = 0") == yes
        e.set_words(R_A, all_ones(e))
        assert compare(e, R_A, R_B, "2^p - 1 = 0") == yes and e.get_ints(R_A) == [0] * LANES
        # (2^(p-1) - 1) + 1: the carry ripples through every digit
        e.set_int(R_A, (1 << (p - 1)) - 1); e.set(R_C, 1); e.add(R_A, R_C); e.set_int(R_B, 1 << (p - 1))
        assert compare(e, R_A, R_B, "ripple") == yes
        # one lane differs, in the lowest and in the highest bit; a product with pending carries on one side
        put(e, R_A, x); put(e, R_I, y); e.set_multiplicand(R_I, R_I); e.mul(R_A, R_I)
        prod = [a * b % mp for a, b in zip(x, y)]
        for lane, bit in ((0, 0), (LANES - 1, 0), (4, p - 1), (LANES - 1, p - 1)):
            other = list(prod)
            other[lane] ^= 1 << bit
            assert other[lane] != mp
            put(e, R_B, other)
            assert compare(e, R_A, R_B, "lane %d bit %d" % (lane, bit)) == [l != lane for l in range(LANES)]
        # mi355_engine_equal stays refused with lanes
        from prmers_amd import EngineError
        with pytest.raises(EngineError, match="not with lanes"):
            e.is_equal(R_A, R_B)


@pytest.mark.parametrize("p, onelaunch", [(1277, True), (132049, False)])
def test_get_ints_equals_the_per_lane_reads(p, onelaunch):
    from prmers_amd import Engine
    x = values(p, LANES, 7)
    with Engine(p, 3, lanes=LANES, onelaunch=onelaunch) as e:
        put(e, 0, x)
        e.set_words(0, all_ones(e), lane=3)                 # 2^p - 1 reads as 0
        e.square_mul(0, 3)                                  # pending run carries
        got = e.get_ints(0)
        assert got == [e.get_int(0, lane=l) for l in range(LANES)]
        assert got == [0 if l == 3 else 3 * v * v % ((1 << p) - 1) for l, v in enumerate(x)]
        put(e, 1, x)
        e.set_words(1, all_ones(e), lane=3)
        assert e.get_ints(1)[3] == 0 == e.get_int(1, lane=3)
        w = e.words_lanes(1)
        assert w.shape == (LANES, e.word_count) and all(np.array_equal(w[l], e.words(1, lane=l)) for l in range(LANES))


@pytest.mark.parametrize("p", [1277, 132049])
def test_an_engine_made_under_host_carry_agrees(p, monkeypatch):
    from prmers_amd import Engine
    mp = (1 << p) - 1
    x, y = values(p, LANES, 11), values(p, LANES, 12)
    other = list(x)
    other[5] ^= 1 << (p - 1)
    answers = []
    for host in (False, True):
        if host:
            monkeypatch.setenv("MI355_HOST_CARRY", "1")
        with Engine(p, 4, lanes=LANES) as e:
            put(e, 0, x); put(e, 2, y); e.set_multiplicand(2, 2); e.mul(0, 2)
            put(e, 1, other); e.mul(1, 2)
            out = compare(e, 0, 1, "host carry %s" % host)
            e.set_words(1, all_ones(e), lane=2)
            answers.append((out, e.get_ints(0), e.get_ints(1)))
    assert answers[0] == answers[1] and answers[0][0] == [l != 5 for l in range(LANES)]
    assert answers[0][1] == [a * b % mp for a, b in zip(x, y)] and answers[0][2][2] == 0


def test_engines_without_lanes_answer_with_one_lane():
    from prmers_amd import CrtEngine, Engine
    p = 9941
    for make in (lambda: Engine(p, 3), lambda: Engine(p, 3, onelaunch=True), lambda: CrtEngine(p, 9, reg_count=3)):
        with make() as e:
            assert e.lanes == 1
            e.set_int(0, 3**700); e.set_int(1, 3**700); e.set_int(2, 3**700 + 1)
            e.square_mul(0); e.square_mul(1); e.square_mul(2)
            assert e.equal_lanes(0, 1) == [True] == [e.is_equal(0, 1)] and e.equal_lanes(0, 2) == [False]
            assert e.get_ints(0) == [e.get_int(0)] == [pow(3, 1400, (1 << p) - 1)]
            e.set_words(1, all_ones(e)); e.set(2, 0)
            assert e.equal_lanes(1, 2) == [True] and e.get_ints(1) == [0]


def test_inside_a_batch_the_queue_runs_first():
    from prmers_amd import Engine
    p = 9941
    mp = (1 << p) - 1
    x, y = values(p, LANES, 21), values(p, LANES, 22)
    with Engine(p, 4, lanes=LANES, onelaunch=True) as e:
        put(e, 0, x); put(e, 1, x); put(e, 2, y); e.set_multiplicand(2, 2)
        with e.batch():
            e.mul(0, 2); e.mul(1, 2); e.square_mul(0); e.square_mul(1)
            assert e.batch_stats()[3] == 4
            assert e.equal_lanes(0, 1) == [True] * LANES and e.batch_stats()[3] == 0
            e.square_mul(1)
            assert e.batch_stats()[3] == 1
            got = e.get_ints(1)
            assert e.batch_stats()[3] == 0
            e.square_mul(0)
            assert e.equal_lanes(0, 1) == [True] * LANES
        assert got == [pow(a * b, 4, mp) for a, b in zip(x, y)] == e.get_ints(0)


def test_refusals():
    from prmers_amd import Engine, EngineError
    from prmers_amd.engine import load_library
    L = load_library()
    p = 1277
    with Engine(p, 3, lanes=LANES) as e:
        e.set(0, 5); e.set(1, 5); e.set(2, 5); e.set_multiplicand(2, 2)
        out = (C.c_uint8 * (LANES + 1))()
        words = (C.c_uint32 * ((LANES + 1) * e.word_count))()

        def refused(rc, text):
            assert rc == 0 and text in L.mi355_engine_last_error().decode(), L.mi355_engine_last_error()
        refused(L.mi355_lanewise_equal(None, 0, 1, out, LANES), "null")
        refused(L.mi355_lanewise_get_words(None, 0, words, LANES * e.word_count), "null")
        refused(L.mi355_lanewise_equal(e.h, 0, 1, None, LANES), "null")
        refused(L.mi355_lanewise_get_words(e.h, 0, None, LANES * e.word_count), "null")
        for count in (LANES - 1, LANES + 1, 0):
            refused(L.mi355_lanewise_equal(e.h, 0, 1, out, count), "count")
        for count in (LANES * e.word_count - 1, e.word_count, (LANES + 1) * e.word_count):
            refused(L.mi355_lanewise_get_words(e.h, 0, words, count), "count")
        for a, b in ((3, 0), (0, 3)):
            refused(L.mi355_lanewise_equal(e.h, a, b, out, LANES), "out of range")
        refused(L.mi355_lanewise_get_words(e.h, 3, words, LANES * e.word_count), "out of range")
        for a, b in ((2, 0), (0, 2)):
            refused(L.mi355_lanewise_equal(e.h, a, b, out, LANES), "multiplicand image")
        refused(L.mi355_lanewise_get_words(e.h, 2, words, LANES * e.word_count), "multiplicand image")
        with pytest.raises(EngineError, match="multiplicand image"):
            e.equal_lanes(0, 2)
        with pytest.raises(EngineError, match="out of range"):
            e.get_ints(3)
        assert e.equal_lanes(0, 1) == [True] * LANES and e.get_ints(0) == [5] * LANES      # and the engine works on
    with Engine(p, 2) as e:
        e.set(0, 5); e.set(1, 5)
        out = (C.c_uint8 * 2)()
        assert L.mi355_lanewise_equal(e.h, 0, 1, out, 2) == 0 and "count" in L.mi355_engine_last_error().decode()


def test_more_lanes_than_a_chunk():
    """p = 132049 with 600 lanes: a chunk is 511 lanes, so lanes 510 and 511 lie on either side of the boundary"""
    from prmers_amd import Engine
    from prmers_amd.engine import load_library
    p, lanes = 132049, 600
    mp = (1 << p) - 1
    with Engine(p, 2, lanes=lanes) as e:
        chunk = load_library().mi355_lanewise_chunk_lanes(e.n, lanes)
        assert e.n == 8192 and chunk == 511
        v = values(p, 3, 31)
        e.set_int(0, v[0]); e.set_int(1, v[0])
        e.square_mul(0); e.square_mul(1)                    # pending run carries on every lane
        sq = v[0] * v[0] % mp
        e.set_int(1, v[1], lane=chunk - 1); e.set_int(1, v[2], lane=chunk)
        e.set_words(0, all_ones(e), lane=lanes - 1); e.set_int(1, 0, lane=lanes - 1)        # equal in the last, partial chunk: 2^p - 1 and 0
        assert e.equal_lanes(0, 1) == [l not in (chunk - 1, chunk) for l in range(lanes)]
        a, b = e.get_ints(0), e.get_ints(1)
        assert a == [sq] * (lanes - 1) + [0]
        assert b == [v[1] if l == chunk - 1 else v[2] if l == chunk else 0 if l == lanes - 1 else sq for l in range(lanes)]
        for l in (0, chunk - 2, chunk - 1, chunk, chunk + 1, lanes - 1):
            assert (a[l], b[l]) == (e.get_int(0, lane=l), e.get_int(1, lane=l))
