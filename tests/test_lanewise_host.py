"""Host side of the lane-wise reads (no GPU): the mi355_lanewise_* symbols through header, binding and library, the null-handle refusals,
and the chunk rule -- how many lanes one launch sequence of the canonical-form pipeline takes -- restated here and checked against the
library and against the cases of tests/test_gpu_lanewise.py."""
import ctypes
import os
import re

from prmers_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRATCH_BYTES = 64 << 20          # canon.hpp kCanonLanesScratchBytes
BLOCK_DIGITS = 4096               # canon.hip kBlockDigits: digits of a scan block


def lane_bytes(n):
    """scratch of one lane: two work arrays and two outputs of n u32 digits, an aggregate and a carry word per scan block, 16 flag words"""
    blocks = -(-n // BLOCK_DIGITS)
    return 4 * n * 4 + (2 * blocks + 16) * 4


def chunk_lanes(n, lanes):
    return min(lanes, max(1, SCRATCH_BYTES // lane_bytes(n)))


def test_lanewise_symbols_are_declared_bound_and_exported_and_stay_out_of_the_other_lists():
    header = open(os.path.join(ROOT, "include", "mi355_lanewise.h")).read()
    declared = sorted(set(re.findall(r"\b(mi355_lanewise_[a-z0-9_]+)\s*\(", header)))
    assert declared == sorted(E.LANEWISE_EXPORTS) and {"mi355_lanewise_equal", "mi355_lanewise_get_words"} <= set(declared)
    lib = ctypes.CDLL(E.LIB_PATH)
    for name in declared:
        getattr(lib, name)
    assert not set(declared) & set(E.EXPORTS + E.LANE_EXPORTS + E.BATCH_EXPORTS)
    for other in ("mi355_engine.h", "mi355_lanes.h", "mi355_batch.h"):
        assert "mi355_lanewise_" not in open(os.path.join(ROOT, "include", other)).read()
    capi = open(os.path.join(ROOT, "prmers_amd", "csrc", "capi.cpp")).read()
    for name in declared:
        assert re.search(r"\b%s\(" % name, capi)
    assert callable(E.Engine.equal_lanes) and callable(E.Engine.get_ints)


def test_null_handles_and_buffers_are_refused_with_a_message():
    L = E.load_library()
    out = (ctypes.c_uint8 * 4)()
    words = (ctypes.c_uint32 * 4)()
    assert L.mi355_lanewise_equal(None, 0, 1, out, 4) == 0 and b"null" in L.mi355_engine_last_error()
    assert L.mi355_lanewise_get_words(None, 0, words, 4) == 0 and b"null" in L.mi355_engine_last_error()
    assert L.mi355_lanewise_equal(None, 0, 1, None, 4) == 0 and b"null" in L.mi355_engine_last_error()
    assert L.mi355_lanewise_get_words(None, 0, None, 4) == 0 and b"null" in L.mi355_engine_last_error()


def test_the_chunk_rule():
    L = E.load_library()
    assert lane_bytes(8192) == 131152 and chunk_lanes(8192, 600) == 511          # "about 128 KiB a lane": 600 lanes are two sequences
    for n in (8, 64, 512, 4096, 4097, 8192, 10240, 16384, 5 << 17, 1 << 22, 1 << 23, 5 << 26):
        for lanes in (1, 2, 9, 511, 512, 600, 65535):
            got = L.mi355_lanewise_chunk_lanes(n, lanes)
            assert got == chunk_lanes(n, lanes), (n, lanes)
            assert 1 <= got <= lanes and (got == 1 or got * lane_bytes(n) <= SCRATCH_BYTES)
            assert got == lanes or got == 1 or (got + 1) * lane_bytes(n) > SCRATCH_BYTES
    assert chunk_lanes(5 << 26, 4) == 1                                          # one lane is larger than the bound: lane by lane
    # the GPU cases: nine lanes are one chunk at every size; 600 lanes at n = 8192 have their boundary between lanes 510 and 511
    for p, n in ((1277, 64), (9941, 512), (132049, 8192), (216091, 10240), (301447, 16384)):
        assert ("n=%d:" % n) in E.resolve_plan(p) and chunk_lanes(n, 9) == 9
    assert -(-600 // chunk_lanes(8192, 600)) == 2
