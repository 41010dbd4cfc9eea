"""Host side of the lane-wise write (no GPU): mi355_lanewise_set_words through header, binding and library, the null refusals, and the
ECM driver's write of every lane through set_ints where the object has it."""
import ctypes
import os
import re

from prmers_amd import ecm
from prmers_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mi355_lanewise_set_words"


def test_the_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "mi355_lanewise.h")).read()
    assert re.search(r"MI355_ENGINE_API int %s\(mi355_engine_handle handle, size_t dst, const uint32_t\* words, size_t count\);" % NAME, header)
    assert NAME in E.LANEWISE_EXPORTS and NAME not in E.EXPORTS + E.LANE_EXPORTS + E.BATCH_EXPORTS
    getattr(ctypes.CDLL(E.LIB_PATH), NAME)
    f = getattr(E.load_library(), NAME)
    assert f.restype is ctypes.c_int and len(f.argtypes) == 4
    assert re.search(r"\b%s\(" % NAME, open(os.path.join(ROOT, "prmers_amd", "csrc", "capi.cpp")).read())
    assert callable(E.Engine.set_words_lanes) and callable(E.Engine.set_ints)
    # the engine's own header keeps its 51 symbols
    engine_header = open(os.path.join(ROOT, "include", "mi355_engine.h")).read()
    assert "mi355_lanewise_" not in engine_header and len(E.EXPORTS) == 51


def test_null_handle_and_null_buffer_are_refused_with_a_message():
    L = E.load_library()
    words = (ctypes.c_uint32 * 4)()
    assert L.mi355_lanewise_set_words(None, 0, words, 4) == 0 and b"null" in L.mi355_engine_last_error()
    assert L.mi355_lanewise_set_words(None, 0, None, 4) == 0 and b"null" in L.mi355_engine_last_error()
    assert b"lanewise_set_words" in L.mi355_engine_last_error()          # the null buffer is named by the call


class _Lanes:
    """what _IO.put needs of an engine with lanes: with set_ints, or with the per-lane set_int alone"""

    def __init__(self, lanes, lanewise):
        self.lanes, self.log = lanes, []
        if lanewise:
            self.set_ints = lambda reg, values: self.log.append(("set_ints", reg, list(values)))

    def set(self, reg, v):
        self.log.append(("set", reg, v))

    def set_int(self, reg, v, lane=None):
        self.log.append(("set_int", reg, v, lane))


def test_the_driver_writes_all_lanes_at_once_where_it_can():
    e = _Lanes(3, True)
    ecm._IO(e, 3, True, False).put(5, [7, 8, 9])
    assert e.log == [("set_ints", 5, [7, 8, 9])]
    e = _Lanes(3, False)
    ecm._IO(e, 3, True, False).put(5, [7, 8, 9])
    assert e.log == [("set", 5, 0), ("set_int", 5, 7, 0), ("set_int", 5, 8, 1), ("set_int", 5, 9, 2)]
    e = _Lanes(1, True)                                    # one curve on an engine used as it is: set_int, as before
    ecm._IO(e, 1, False, False).put(5, [7])
    assert e.log == [("set_int", 5, 7, None)]
