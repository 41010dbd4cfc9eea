"""The lane-wise write (include/mi355_lanewise.h mi355_lanewise_set_words; canon.hip k_unpack_words with the lanes as grid.y): set_words_lanes
and set_ints on every lane of an engine in one upload and one launch per chunk of lanes, against the per-lane writes and Python integers.
The shapes are those of tests/test_gpu_lanewise.py.  Targets that held an image or pending run carries, the host-carry engine, engines
without lanes, batches, every refusal, and more lanes than one chunk.
Needs a real MI355X:  python -m pytest tests -m gpu"""
import ctypes as C
import random

import numpy as np
import pytest

from test_gpu_lanewise import CASES, LANES, values

pytestmark = pytest.mark.gpu

(R_A, R_B, R_C, R_D) = range(4)
REGS = 4


def to_words(v, wc):
    return np.frombuffer(int(v).to_bytes(wc * 4, "little"), dtype="<u4")


def lane_words(p, wc, seed):
    """(an array of LANES x wc words, the residues they stand for): random residues, 0, 1, Mp - 1, the all-ones words of Mp itself (reads
    0) and a value with bits at and above p in its top word (folded back in: 2^p = 1)"""
    mp = (1 << p) - 1
    x = values(p, LANES, seed)
    high = (1 << (32 * wc - p)) - 1                        # every bit of the top word above p, and bit p itself
    raw = [x[0], 0, 1, mp - 1, mp, (x[5] >> 1) | (high << p), x[6], x[7] | (1 << p), x[8]]
    assert raw[5] >> p and all(v < 1 << (32 * wc) for v in raw)
    return np.stack([to_words(v, wc) for v in raw]), [v % mp for v in raw]


@pytest.mark.parametrize("p, onelaunch", CASES, ids=["%d%s" % (p, "-onelaunch" if o else "") for p, o in CASES])
def test_every_lane_is_written_as_the_per_lane_writes_write_it(p, onelaunch):
    from prmers_amd import Engine
    mp = (1 << p) - 1
    with Engine(p, REGS, lanes=LANES, onelaunch=onelaunch) as e:
        w, want = lane_words(p, e.word_count, 1)
        assert want[4] == 0 and want[3] == mp - 1 and len(set(want)) >= LANES - 1
        e.set_words_lanes(R_A, w)
        assert e.get_ints(R_A) == want == [e.get_int(R_A, lane=l) for l in range(LANES)]
        e.set(R_B, 0)
        for l in range(LANES):
            e.set_words(R_B, w[l], lane=l)
        assert e.equal_lanes(R_A, R_B) == [True] * LANES
        # the digits are valid operands
        e.square_mul(R_A); e.square_mul(R_B)
        assert e.get_ints(R_A) == [v * v % mp for v in want] == e.get_ints(R_B)
        # a target with pending run carries (R_A after its squaring), and one that holds an image
        w2, want2 = lane_words(p, e.word_count, 2)
        e.set_multiplicand(R_C, R_B)
        e.square_mul(R_A)
        e.set_words_lanes(R_A, w2); e.set_words_lanes(R_C, w2)
        assert e.get_ints(R_A) == want2 == e.get_ints(R_C)
        e.square_mul(R_A, 3); e.set_multiplicand(R_D, R_C); e.mul(R_C, R_D)
        assert e.get_ints(R_A) == [3 * v * v % mp for v in want2] and e.get_ints(R_C) == [v * v % mp for v in want2]
        # set_ints reduces its values
        big = [v + mp * (l % 3) for l, v in enumerate(want)]
        big[2] = -1
        e.set_ints(R_D, big)
        assert e.get_ints(R_D) == [mp - 1 if l == 2 else v for l, v in enumerate(want)]
        with pytest.raises(ValueError):
            e.set_ints(R_D, big[:-1])
        with pytest.raises(ValueError):
            e.set_words_lanes(R_D, w[:, :-1])


@pytest.mark.parametrize("p", [1277, 132049])
def test_an_engine_made_under_host_carry_agrees(p, monkeypatch):
    from prmers_amd import Engine
    mp = (1 << p) - 1
    answers = []
    for host in (False, True):
        if host:
            monkeypatch.setenv("MI355_HOST_CARRY", "1")
        with Engine(p, 3, lanes=LANES) as e:
            w, want = lane_words(p, e.word_count, 3)
            e.set(1, 7); e.set_multiplicand(1, 1)
            e.set_words_lanes(0, w); e.set_words_lanes(1, w)           # 1 held an image
            first = e.get_ints(0)
            e.square_mul(0)
            answers.append((first, e.get_ints(1), e.get_ints(0)))
    assert answers[0] == answers[1] == (want, want, [v * v % mp for v in want])


def test_engines_without_lanes_answer_through_set_words():
    from prmers_amd import CrtEngine, Engine
    p = 9941
    mp = (1 << p) - 1
    v = values(p, 2, 5)
    for make in (lambda: Engine(p, 3), lambda: Engine(p, 3, onelaunch=True), lambda: CrtEngine(p, 9, reg_count=3)):
        with make() as e:
            assert e.lanes == 1
            e.set_ints(0, [v[0] + mp])
            e.set_words_lanes(1, to_words(v[1], e.word_count).reshape(1, -1))
            e.set_int(2, v[1])
            assert e.get_int(0) == v[0] and e.get_int(1) == v[1] and e.is_equal(1, 2)
            e.square_mul(0)
            assert e.get_ints(0) == [v[0] * v[0] % mp]
            with pytest.raises(ValueError):
                e.set_ints(0, v)


def test_inside_a_batch_the_queue_runs_first():
    from prmers_amd import Engine
    p = 9941
    mp = (1 << p) - 1
    x, y = values(p, LANES, 21), values(p, LANES, 22)
    with Engine(p, 3, lanes=LANES, onelaunch=True) as e:
        e.set_ints(0, x); e.set_ints(1, x)
        with e.batch():
            e.square_mul(0); e.square_mul(1)
            assert e.batch_stats()[3] == 2
            e.set_ints(0, y)                               # after the queued squaring of 0, not before it
            assert e.batch_stats()[3] == 0
            e.square_mul(0)
            assert e.batch_stats()[3] == 1
        assert e.get_ints(0) == [v * v % mp for v in y] and e.get_ints(1) == [v * v % mp for v in x]


def test_refusals():
    from prmers_amd import Engine, EngineError
    from prmers_amd.engine import load_library
    L = load_library()
    p = 1277
    with Engine(p, 3, lanes=LANES) as e:
        count = LANES * e.word_count
        words = (C.c_uint32 * ((LANES + 1) * e.word_count))()
        e.set(0, 5)

        def refused(rc, text):
            assert rc == 0 and text in L.mi355_engine_last_error().decode(), L.mi355_engine_last_error()
        refused(L.mi355_lanewise_set_words(None, 0, words, count), "null")
        refused(L.mi355_lanewise_set_words(e.h, 0, None, count), "null")
        for bad in (count - 1, e.word_count, count + e.word_count, 0):
            refused(L.mi355_lanewise_set_words(e.h, 0, words, bad), "count")
        refused(L.mi355_lanewise_set_words(e.h, 3, words, count), "out of range")
        with pytest.raises(EngineError, match="out of range"):
            e.set_ints(3, [1] * LANES)
        assert e.get_ints(0) == [5] * LANES                                # nothing was written, and the engine works on
        e.set_ints(0, range(LANES))
        assert e.get_ints(0) == list(range(LANES))
    with Engine(p, 2) as e:
        assert L.mi355_lanewise_set_words(e.h, 0, words, 2 * e.word_count) == 0 and "count" in L.mi355_engine_last_error().decode()
        refused(L.mi355_lanewise_set_words(e.h, 2, words, e.word_count), "out of range")


def test_more_lanes_than_a_chunk():
    """p = 132049 with 600 lanes: a chunk is 511 lanes, so lanes 510 and 511 lie on either side of the boundary"""
    from prmers_amd import Engine
    from prmers_amd.engine import load_library
    p, lanes = 132049, 600
    mp = (1 << p) - 1
    with Engine(p, 2, lanes=lanes) as e:
        chunk = load_library().mi355_lanewise_chunk_lanes(e.n, lanes)
        assert e.n == 8192 and chunk == 511
        v = values(p, 4, 41)
        want = [v[0]] * lanes
        want[chunk - 1], want[chunk], want[lanes - 1] = v[1], v[2], v[3]
        e.set_int(0, 1); e.square_mul(0)                    # pending run carries on every lane
        e.set_ints(0, want)
        assert e.get_ints(0) == want
        for l in (0, chunk - 2, chunk - 1, chunk, chunk + 1, lanes - 2, lanes - 1):
            assert e.get_int(0, lane=l) == want[l]
        e.square_mul(0)
        got = e.get_ints(0)
        sq = {x: x * x % mp for x in v}
        assert got == [sq[x] for x in want]
