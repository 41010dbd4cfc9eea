"""Python binding of libmi355_engine.so (ctypes over the C ABI in include/mi355_engine.h).

`Engine` mirrors the reference's `engine` register machine for the Marin path
(include/marin/engine.h:16-303: set / copy / square_mul / set_multiplicand / mul / sub / add /
sub_reg / get_mpz / set_mpz / digit / checkpoint), same names, same argument meaning, errors raised
as EngineError where the reference throws std::runtime_error.  There is no CPU fallback: without the
built HIP library or without a GPU, construction fails.
"""
import contextlib
import ctypes as C
import operator
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# MI355_ENGINE_LIB overrides the library path (A/B builds), as AEVUM_ENGINE_LIB does for the reference's plugin
# (src/aevum/EngineAevum.cpp:193-223)
LIB_PATH = os.environ.get("MI355_ENGINE_LIB") or os.path.join(_HERE, "libmi355_engine.so")


class EngineError(RuntimeError):
    pass


_lib = None


def load_library():
    """dlopen the in-tree HIP library; raises if it has not been built (see __graft_entry__.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EngineError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, sz, u32, u64p = C.c_void_p, C.c_size_t, C.c_uint32, C.POINTER(C.c_uint64)
    dp = C.POINTER(C.c_double)
    sig = {
        "mi355_engine_version": (C.c_char_p, []),
        "mi355_engine_last_error": (C.c_char_p, []),
        "mi355_engine_resolve_fft": (C.c_int, [u32, C.c_char_p, C.c_char_p, sz]),
        "mi355_engine_create": (vp, [u32, sz, u32, C.c_int, C.c_char_p, C.c_char_p]),
        "mi355_engine_destroy": (None, [vp]),
        "mi355_engine_transform_size": (sz, [vp]),
        "mi355_engine_word_count": (sz, [vp]),
        "mi355_engine_sync": (C.c_int, [vp]),
        "mi355_engine_set_u32": (C.c_int, [vp, sz, u32]),
        "mi355_engine_set_words": (C.c_int, [vp, sz, vp, sz]),
        "mi355_engine_get_words": (C.c_int, [vp, sz, vp, sz]),
        "mi355_engine_copy": (C.c_int, [vp, sz, sz]),
        "mi355_engine_prepare": (C.c_int, [vp, sz, sz]),
        "mi355_engine_square_mul": (C.c_int, [vp, sz, u32]),
        "mi355_engine_mul": (C.c_int, [vp, sz, sz, u32]),
        "mi355_engine_add": (C.c_int, [vp, sz, sz]),
        "mi355_engine_sub_reg": (C.c_int, [vp, sz, sz]),
        "mi355_engine_sub_u32": (C.c_int, [vp, sz, u32]),
        "mi355_engine_equal": (C.c_int, [vp, sz, sz, C.POINTER(C.c_int)]),
        "mi355_engine_get_digits": (C.c_int, [vp, sz, vp, sz]),
        "mi355_engine_set_digits": (C.c_int, [vp, sz, vp, sz]),
        "mi355_engine_res64": (C.c_int, [vp, sz, u64p]),
        "mi355_engine_register_data_size": (sz, [vp]),
        "mi355_engine_get_data": (C.c_int, [vp, sz, vp, sz]),
        "mi355_engine_set_data": (C.c_int, [vp, sz, vp, sz]),
        "mi355_engine_checkpoint_size": (sz, [vp]),
        "mi355_engine_get_checkpoint": (C.c_int, [vp, vp, sz]),
        "mi355_engine_set_checkpoint": (C.c_int, [vp, vp, sz]),
        "mi355_engine_time_square_mul": (C.c_int, [vp, sz, u32, u32, sz, dp, dp, sz]),
        "mi355_engine_kernel_count": (sz, [vp]),
        "mi355_engine_kernel_name": (C.c_char_p, [vp, sz]),
        "mi355_engine_algorithmic_bytes": (sz, [vp]),
        "mi355_engine_selftest": (C.c_int, [sz]),
        "mi355_engine_addsub": (C.c_int, [vp, sz, sz, sz, sz]),
        "mi355_engine_addsub_copy": (C.c_int, [vp, sz, sz, sz, sz, sz, sz]),
        "mi355_engine_mul_add": (C.c_int, [vp, sz, sz, sz, u32]),
        "mi355_engine_square_mul_copy": (C.c_int, [vp, sz, sz, u32]),
        "mi355_engine_square_mul_n": (C.c_int, [vp, sz, u32, sz, u32]),
        "mi355_engine_mul_copy": (C.c_int, [vp, sz, sz, sz, u32]),
        "mi355_engine_exp_mul": (C.c_int, [vp, sz, C.c_uint64, sz, sz]),
        "mi355_engine_exp_mul2": (C.c_int, [vp, sz, C.c_uint64, sz, sz]),
        "mi355_engine_mul_sum": (C.c_int, [vp, sz, sz, sz, sz]),
        "mi355_engine_mul_sum_is_fused": (C.c_int, [vp]),
        "mi355_engine_square_mul_bits": (C.c_int, [vp, sz, u32, C.c_char_p, sz]),
        "mi355_engine_square_mul_prepare": (C.c_int, [vp, sz, sz, u32]),
        "mi355_engine_square_mul_prepare_is_fused": (C.c_int, [vp]),
        "mi355_crt_carry": (C.c_int, [u32, sz, u32, u32, vp, vp, vp, vp, sz, dp]),
        "mi355_crt_transform_size": (sz, [u32, u32]),
        "mi355_engine_describe": (C.c_int, [vp, C.c_char_p, sz]),
        "mi355_crt_get_raw_digits": (C.c_int, [vp, sz, vp, sz, C.c_int]),
        "mi355_crt_set_raw_digits": (C.c_int, [vp, sz, vp, sz]),
        # include/mi355_lanes.h
        "mi355_lanes_count": (sz, [vp]),
        "mi355_lanes_set_words": (C.c_int, [vp, sz, sz, vp, sz]),
        "mi355_lanes_get_words": (C.c_int, [vp, sz, sz, vp, sz]),
        "mi355_lanes_res64": (C.c_int, [vp, sz, sz, u64p]),
        # include/mi355_batch.h
        "mi355_batch_begin": (C.c_int, [vp]),
        "mi355_batch_end": (C.c_int, [vp]),
        "mi355_batch_stats": (C.c_int, [vp, u64p]),
        # include/mi355_lanewise.h
        "mi355_lanewise_equal": (C.c_int, [vp, sz, sz, vp, sz]),
        "mi355_lanewise_get_words": (C.c_int, [vp, sz, vp, sz]),
        "mi355_lanewise_set_words": (C.c_int, [vp, sz, vp, sz]),
        "mi355_lanewise_chunk_lanes": (sz, [sz, sz]),
        # include/mi355_lanecross.h
        "mi355_lanecross_mul_sibling": (C.c_int, [vp, sz, sz, sz, u32]),
    }
    for name, (res, args) in sig.items():
        if name in LANE_EXPORTS + BATCH_EXPORTS + LANEWISE_EXPORTS + LANECROSS_EXPORTS and os.environ.get("MI355_ENGINE_LIB") and not hasattr(L, name):
            continue           # an A/B library from before the lanes, the batches, the lane-wise reads or the product across lanes
                               # (tools/time_lanes.py): Engine.lanes reads 1, batch(), equal_lanes() and mul_sibling() raise
        f = getattr(L, name)   # AttributeError here = the library does not export what the header declares
        f.restype, f.argtypes = res, args
    _lib = L
    return L


EXPORTS = [
    "mi355_engine_version", "mi355_engine_last_error", "mi355_engine_resolve_fft", "mi355_engine_create",
    "mi355_engine_destroy", "mi355_engine_transform_size", "mi355_engine_word_count", "mi355_engine_sync",
    "mi355_engine_set_u32", "mi355_engine_set_words", "mi355_engine_get_words", "mi355_engine_copy",
    "mi355_engine_prepare", "mi355_engine_square_mul", "mi355_engine_mul", "mi355_engine_add",
    "mi355_engine_sub_reg", "mi355_engine_sub_u32", "mi355_engine_equal", "mi355_engine_get_digits",
    "mi355_engine_set_digits", "mi355_engine_res64", "mi355_engine_register_data_size", "mi355_engine_get_data",
    "mi355_engine_set_data", "mi355_engine_checkpoint_size", "mi355_engine_get_checkpoint",
    "mi355_engine_set_checkpoint", "mi355_engine_time_square_mul", "mi355_engine_kernel_count",
    "mi355_engine_kernel_name", "mi355_engine_algorithmic_bytes", "mi355_engine_selftest",
    "mi355_crt_carry", "mi355_crt_transform_size", "mi355_engine_describe", "mi355_crt_get_raw_digits", "mi355_crt_set_raw_digits",
    "mi355_engine_addsub", "mi355_engine_addsub_copy", "mi355_engine_mul_add", "mi355_engine_square_mul_copy", "mi355_engine_mul_copy", "mi355_engine_square_mul_n",
    "mi355_engine_exp_mul", "mi355_engine_exp_mul2",
    "mi355_engine_mul_sum", "mi355_engine_mul_sum_is_fused", "mi355_engine_square_mul_bits",
    "mi355_engine_square_mul_prepare", "mi355_engine_square_mul_prepare_is_fused",
]


# include/mi355_lanes.h: per-lane I/O of engines created with the plan token lanes=B
LANE_EXPORTS = ["mi355_lanes_count", "mi355_lanes_set_words", "mi355_lanes_get_words", "mi355_lanes_res64"]


# include/mi355_batch.h: a run of register operations of a one-launch engine as one launch
BATCH_EXPORTS = ["mi355_batch_begin", "mi355_batch_end", "mi355_batch_stats"]


# include/mi355_lanewise.h: compare, read or write every lane of a register in one launch sequence
LANEWISE_EXPORTS = ["mi355_lanewise_equal", "mi355_lanewise_get_words", "mi355_lanewise_set_words", "mi355_lanewise_chunk_lanes"]


# include/mi355_lanecross.h: a product whose multiplicand image comes from another lane
LANECROSS_EXPORTS = ["mi355_lanecross_mul_sibling"]


def resolve_plan(p, spec=None):
    """Transform plan text for exponent p (no GPU needed)."""
    L = load_library()
    buf = C.create_string_buffer(256)
    if not L.mi355_engine_resolve_fft(p, spec.encode() if spec else None, buf, 256):
        raise EngineError(L.mi355_engine_last_error().decode())
    return buf.value.decode()


def u64_arg(name, v):
    """v as a uint64_t argument of the C ABI (see u32_arg)"""
    try:
        iv = operator.index(v)
    except TypeError:
        raise TypeError("%s must be an integer, not %s" % (name, type(v).__name__)) from None
    if not 0 <= iv <= 0xFFFFFFFFFFFFFFFF:
        raise ValueError("%s = %d is outside the 64-bit range [0, 2**64) of the engine's C ABI" % (name, iv))
    return iv


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def u32_arg(name, v):
    """v as a uint32_t argument of the C ABI: ctypes would silently keep the low 32 bits of anything else
    (2**32 + 3 -> 3, -1 -> 2**32 - 1), so values outside [0, 2**32) are refused here, before any C call."""
    try:
        iv = operator.index(v)
    except TypeError:
        raise TypeError("%s must be an integer, not %s" % (name, type(v).__name__)) from None
    if not 0 <= iv <= 0xFFFFFFFF:
        raise ValueError("%s = %d is outside the 32-bit range [0, 2**32) of the engine's C ABI" % (name, iv))
    return iv


class Engine:
    """engine::create_gpu(p, reg_count, device, verbose) on an MI355X (include/marin/engine.h:301)."""

    def __init__(self, p, reg_count=8, device=0, verbose=False, plan=None, lanes=1, onelaunch=False):
        """lanes = B > 1: B independent residues per register, every operation on all of them in one launch (include/mi355_lanes.h);
        reads then take lane=l, writes lane=l or None for every lane.
        onelaunch: the plan token of that name -- a product is one launch, the whole lane in one work-group (p <= 204799)."""
        self.L = load_library()
        if lanes != 1:
            plan = (plan + "," if plan else "") + "lanes=%d" % operator.index(lanes)
        if onelaunch:
            plan = (plan + "," if plan else "") + "onelaunch"
        self.h = self.L.mi355_engine_create(p, reg_count, device, int(verbose), plan.encode() if plan else None, None)
        if not self.h:
            raise EngineError(self.L.mi355_engine_last_error().decode())
        self.p, self.reg_count = p, reg_count
        self.lanes = self.L.mi355_lanes_count(self.h) if hasattr(self.L, "mi355_lanes_count") else 1
        self.n = self.L.mi355_engine_transform_size(self.h)
        self.word_count = self.L.mi355_engine_word_count(self.h)

    def close(self):
        if getattr(self, "h", None):
            self.L.mi355_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _ok(self, rc):
        if not rc:
            raise EngineError(self.L.mi355_engine_last_error().decode())

    # --- engine.h surface ---
    def get_size(self): return self.n
    def sync(self): self._ok(self.L.mi355_engine_sync(self.h))
    def set(self, dst, a): self._ok(self.L.mi355_engine_set_u32(self.h, dst, u32_arg("value", a)))
    def copy(self, dst, src): self._ok(self.L.mi355_engine_copy(self.h, dst, src))
    def square_mul(self, src, a=1): self._ok(self.L.mi355_engine_square_mul(self.h, src, u32_arg("factor", a)))
    def set_multiplicand(self, dst, src): self._ok(self.L.mi355_engine_prepare(self.h, dst, src))
    def mul(self, dst, src, a=1): self._ok(self.L.mi355_engine_mul(self.h, dst, src, u32_arg("factor", a)))
    def sub(self, src, a): self._ok(self.L.mi355_engine_sub_u32(self.h, src, u32_arg("value", a)))
    def add(self, dst, src): self._ok(self.L.mi355_engine_add(self.h, dst, src))
    def sub_reg(self, dst, src): self._ok(self.L.mi355_engine_sub_reg(self.h, dst, src))

    # fused variants (engine.h:65-131): one sweep each
    def addsub(self, sum_out, diff_out, a, b): self._ok(self.L.mi355_engine_addsub(self.h, sum_out, diff_out, a, b))
    def addsub_copy(self, s, d, s_copy, d_copy, a, b): self._ok(self.L.mi355_engine_addsub_copy(self.h, s, d, s_copy, d_copy, a, b))
    def mul_add(self, dst, mul_src, add_src, a=1): self._ok(self.L.mi355_engine_mul_add(self.h, dst, mul_src, add_src, u32_arg("factor", a)))
    def square_mul_copy(self, src, dst_copy, a=1): self._ok(self.L.mi355_engine_square_mul_copy(self.h, src, dst_copy, u32_arg("factor", a)))
    def square_mul_n(self, src, count, a=1, sub=0):
        """count x { src = src^2 * a; src -= sub } in one engine call."""
        self._ok(self.L.mi355_engine_square_mul_n(self.h, src, u32_arg("factor", a), count, u32_arg("sub", sub)))
    def mul_copy(self, dst, src, dst_copy, a=1): self._ok(self.L.mi355_engine_mul_copy(self.h, dst, src, dst_copy, u32_arg("factor", a)))

    def exp_mul(self, a, h, b, tmp):
        """a = a^h * b with a 64-bit h, in one engine call (the fold of a PRP proof); b and tmp are consumed."""
        self._ok(self.L.mi355_engine_exp_mul(self.h, a, u64_arg("h", h), b, tmp))

    def exp_mul2(self, a, h, b, tmp):
        """a = a^h * b^2; b and tmp are consumed."""
        self._ok(self.L.mi355_engine_exp_mul2(self.h, a, u64_arg("h", h), b, tmp))

    def mul_sum(self, dst, src_a, src_b, tmp):
        """dst = dst * (a + b) for two multiplicand images (left intact; tmp is scratch): one product where the plan allows it."""
        self._ok(self.L.mi355_engine_mul_sum(self.h, dst, src_a, src_b, tmp))

    def mul_sum_is_fused(self):
        """True if mul_sum runs as one product on this plan (False: the two-product composition, same result)"""
        return bool(self.L.mi355_engine_mul_sum_is_fused(self.h))

    def square_mul_bits(self, reg, factor, bits, nbits):
        """reg = reg^(2^nbits) * factor^B, B = the nbits bits of `bits` (bytes, most significant bit first), in one engine call."""
        bits = bytes(bits)
        if nbits < 0 or nbits > 8 * len(bits):
            raise ValueError("nbits = %d does not fit the %d bytes given" % (nbits, len(bits)))
        self._ok(self.L.mi355_engine_square_mul_bits(self.h, reg, u32_arg("factor", factor), bits, nbits))

    def square_mul_prepare(self, src, img_out, a=1):
        """img_out = the multiplicand image of src, then src = src^2 * a: one squaring whose row sweep keeps the transform of its operand."""
        self._ok(self.L.mi355_engine_square_mul_prepare(self.h, src, img_out, u32_arg("factor", a)))

    def square_mul_prepare_is_fused(self):
        """True if square_mul_prepare runs as one squaring (False: set_multiplicand + square_mul, same result)"""
        return bool(self.L.mi355_engine_square_mul_prepare_is_fused(self.h))

    # --- batches (include/mi355_batch.h): engines made with onelaunch=True ---
    def _batch_fn(self, name):
        f = getattr(self.L, name, None)
        if f is None:
            raise EngineError("batch: %s does not export %s (a library from before the batches)" % (LIB_PATH, name))
        return f

    @contextlib.contextmanager
    def batch(self):
        """with e.batch(): the copies, sums and differences and one-launch products issued inside are queued and run as ONE launch, in
        order, with the results of the same calls issued one by one.  Anything else (sub, set, a read, sync, a factor above the fused
        bound) runs the queue first and then itself; a full queue runs by itself.  The batch ends on an exception too."""
        begin, end = self._batch_fn("mi355_batch_begin"), self._batch_fn("mi355_batch_end")
        self._ok(begin(self.h))
        try:
            yield self
        except BaseException:
            if getattr(self, "h", None):
                end(self.h)              # the first error is the one to report
            raise
        else:
            self._ok(end(self.h))

    def batch_stats(self):
        """(operations queued so far, batch launches so far, capacity of the queue, operations pending now)"""
        out = (C.c_uint64 * 4)()
        self._ok(self._batch_fn("mi355_batch_stats")(self.h, out))
        return tuple(int(v) for v in out)

    def is_equal(self, lhs, rhs):
        out = C.c_int(0)
        self._ok(self.L.mi355_engine_equal(self.h, lhs, rhs, C.byref(out)))
        return bool(out.value)

    equal = is_equal        # the names prmers_amd/proof.py uses

    # --- every lane at once (include/mi355_lanewise.h) ---
    def _lanewise_fn(self, name):
        f = getattr(self.L, name, None)
        if f is None:
            raise EngineError("%s does not export %s (a library from before the lane-wise reads)" % (LIB_PATH, name))
        return f

    def equal_lanes(self, lhs, rhs):
        """[lane l of lhs == lane l of rhs mod 2^p - 1 for every lane], one launch sequence for all of them (an engine without lanes: the
        one answer of is_equal)"""
        out = np.zeros(self.lanes, dtype=np.uint8)
        self._ok(self._lanewise_fn("mi355_lanewise_equal")(self.h, lhs, rhs, _ptr(out), out.size))
        return [bool(v) for v in out]

    def words_lanes(self, src):
        """the canonical words of every lane: an array of lanes x word_count (what get_ints is made of)"""
        w = np.zeros((self.lanes, self.word_count), dtype=np.uint32)
        self._ok(self._lanewise_fn("mi355_lanewise_get_words")(self.h, src, _ptr(w), w.size))
        return w

    def get_ints(self, src):
        """[get_int(src, lane=l) for every lane], read in one launch sequence"""
        return [int.from_bytes(row.astype("<u4").tobytes(), "little") for row in self.words_lanes(src)]

    def set_words_lanes(self, dst, w):
        """lane l of dst = the residue of the words w[l]: an array of lanes x word_count, written in one upload and one launch per chunk of
        lanes.  dst becomes a register of residues whatever it held."""
        w = np.ascontiguousarray(w, dtype=np.uint32)
        if w.shape != (self.lanes, self.word_count):
            raise ValueError("set_words_lanes wants an array of %d x %d words, not %s" % (self.lanes, self.word_count, w.shape))
        self._ok(self._lanewise_fn("mi355_lanewise_set_words")(self.h, dst, _ptr(w), w.size))

    def set_ints(self, dst, values):
        """set_int(dst, values[l], lane=l) for every lane, in one launch sequence; each value is reduced mod 2^p - 1 first"""
        values = list(values)
        if len(values) != self.lanes:
            raise ValueError("set_ints wants one value per lane: %d given, the engine has %d lanes" % (len(values), self.lanes))
        mp, size = (1 << self.p) - 1, self.word_count * 4
        raw = b"".join((int(v) % mp).to_bytes(size, "little") for v in values)
        self.set_words_lanes(dst, np.frombuffer(raw, dtype="<u4").reshape(self.lanes, self.word_count))

    # --- across lanes (include/mi355_lanecross.h) ---
    def mul_sibling(self, dst, src, alt, level):
        """dst[l] = dst[l] * src[g] on every lane l, g = ((l >> level) ^ 1) << level the first lane of l's sibling block of 2^level lanes,
        the image read from lane g of src; where g is no lane, dst[l] * alt[l].  src and alt are multiplicand images (keep the image of 1
        in alt), left as they are.  An engine with one lane: mul(dst, alt).  prmers_amd/lanecross.py builds the inverse on every lane
        from it."""
        f = getattr(self.L, "mi355_lanecross_mul_sibling", None)
        if f is None:
            raise EngineError("%s does not export mi355_lanecross_mul_sibling (a library from before the product across lanes)" % LIB_PATH)
        self._ok(f(self.h, dst, src, alt, u32_arg("level", level)))

    def pow(self, dst, src, e):
        """dst = src^e, src is erased (engine.h:160-170)."""
        self.set_multiplicand(src, src)
        self.set(dst, 1)
        if e == 0:
            return
        for i in range(int(e).bit_length() - 1, -1, -1):
            self.square_mul(dst)
            if (e >> i) & 1:
                self.mul(dst, src)

    # --- digit / word I/O ---
    def digits(self, src):
        """engine::digit (engine.h:234-296): n values `digit | width << 32`."""
        d = np.zeros(self.n, dtype=np.uint64)
        self._ok(self.L.mi355_engine_get_digits(self.h, src, _ptr(d), self.n))
        return d

    def set_digits(self, dst, d):
        d = np.ascontiguousarray(d, dtype=np.uint64)
        self._ok(self.L.mi355_engine_set_digits(self.h, dst, _ptr(d), d.size))

    # lane=None: the register as a whole -- today's call on an engine without lanes; with lanes a write goes to every lane and a read
    # is refused (name the lane).  lane=l: that lane (l = 0 is the register itself on an engine without lanes).
    def res64(self, src, lane=None):
        out = C.c_uint64(0)
        if lane is None:
            self._ok(self.L.mi355_engine_res64(self.h, src, C.byref(out)))
        else:
            self._ok(self.L.mi355_lanes_res64(self.h, lane, src, C.byref(out)))
        return out.value

    def words(self, src, lane=None):
        w = np.zeros(self.word_count, dtype=np.uint32)
        if lane is None:
            self._ok(self.L.mi355_engine_get_words(self.h, src, _ptr(w), w.size))
        else:
            self._ok(self.L.mi355_lanes_get_words(self.h, lane, src, _ptr(w), w.size))
        return w

    get_words = words

    def set_words(self, dst, w, lane=None):
        w = np.ascontiguousarray(w, dtype=np.uint32)
        if lane is None:
            self._ok(self.L.mi355_engine_set_words(self.h, dst, _ptr(w), w.size))
        else:
            self._ok(self.L.mi355_lanes_set_words(self.h, lane, dst, _ptr(w), w.size))

    def get_int(self, src, lane=None):
        """get_mpz (engine.h:173-203) as a Python int in [0, 2^p-1)."""
        return int.from_bytes(self.words(src, lane).astype("<u4").tobytes(), "little")

    def set_int(self, dst, v, lane=None):
        """set_mpz (engine.h:206-232); v is reduced mod 2^p-1 first."""
        v = int(v) % ((1 << self.p) - 1)
        self.set_words(dst, np.frombuffer(v.to_bytes(self.word_count * 4, "little"), dtype="<u4"), lane)

    # --- raw images / checkpoints ---
    def get_register_data_size(self): return self.L.mi355_engine_register_data_size(self.h)

    def get_data(self, src):
        buf = np.zeros(self.get_register_data_size(), dtype=np.uint8)
        self._ok(self.L.mi355_engine_get_data(self.h, src, _ptr(buf), buf.size))
        return buf

    def set_data(self, dst, buf):
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        rc = self.L.mi355_engine_set_data(self.h, dst, _ptr(buf), buf.size)
        return bool(rc)

    def get_checkpoint_size(self): return self.L.mi355_engine_checkpoint_size(self.h)

    def get_checkpoint(self):
        buf = np.zeros(self.get_checkpoint_size(), dtype=np.uint8)
        self._ok(self.L.mi355_engine_get_checkpoint(self.h, _ptr(buf), buf.size))
        return buf

    def set_checkpoint(self, buf):
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        return bool(self.L.mi355_engine_set_checkpoint(self.h, _ptr(buf), buf.size))

    # --- measurement ---
    def kernel_names(self):
        return [self.L.mi355_engine_kernel_name(self.h, k).decode() for k in range(self.L.mi355_engine_kernel_count(self.h))]

    def time_square_mul(self, reg, iters, a=1, sub=0, per_kernel=False):
        """(total_ms, {kernel: avg_ms}) for `iters` back-to-back squarings, HIP events on the engine stream."""
        a, sub = u32_arg("factor", a), u32_arg("sub", sub)
        total = C.c_double(0)
        k = self.L.mi355_engine_kernel_count(self.h)
        ks = (C.c_double * k)()
        self._ok(self.L.mi355_engine_time_square_mul(self.h, reg, a, sub, iters, C.byref(total),
                                                     ks if per_kernel else None, k if per_kernel else 0))
        return total.value, (dict(zip(self.kernel_names(), list(ks))) if per_kernel else {})

    def algorithmic_bytes(self): return self.L.mi355_engine_algorithmic_bytes(self.h)

    def describe(self):
        """plan text of this engine (kernel set included)"""
        buf = C.create_string_buffer(256)
        self._ok(self.L.mi355_engine_describe(self.h, buf, 256))
        return buf.value.decode()



class CrtEngine(Engine):
    """The GF(M61^2) x GF(M31^2) engine with a prime-factor axis of radix 1, 3 or 9 (the reference's Aevum plugin,
    third_party/aevum/src/EngineApi.h:28-59) -- the same register machine as `Engine`, selected through the fft_spec "crt:odd[:words=N]".
    Digits are plain u64 values here (widths reach 39 bits).  No CPU fallback."""

    def __init__(self, p, odd=1, n=0, device=0, plan=None, reg_count=4):
        """odd = None / "auto": radix 9, 3 or none by the reference's stock / PFA size-ratio gates (README.md:888-926)"""
        spec = ("crt:auto" if odd in (None, "auto") else "crt:%d" % odd) + (":words=%d" % n if n else "") + (":" + plan if plan else "")
        Engine.__init__(self, p, reg_count, device, False, spec)
        self.odd = int(self.describe().split("odd=")[1].split(":")[0]) if odd in (None, "auto") else odd

    def raw_digits(self, src=0):
        """the engine's own digits: plain values in base 2^width_j, canonical (widths reach 39 bits)"""
        d = np.zeros(self.n, dtype=np.uint64)
        self._ok(self.L.mi355_crt_get_raw_digits(self.h, src, _ptr(d), self.n, 1))
        return d

    def set_digits(self, dst, d):
        """plain digit values (the engine's own base 2^width_j digits)"""
        d = np.ascontiguousarray(d, dtype=np.uint64)
        self._ok(self.L.mi355_crt_set_raw_digits(self.h, dst, _ptr(d), d.size))

    def digits(self, src=0):
        """value | width << 32 like engine::get (engine.h:24), for callers that cut a residue into words themselves (prp.py): the canonical
        residue in 32-bit pieces -- this family's own digits do not always fit that encoding"""
        w = self.words(src).astype(np.uint64)
        width = np.full(w.size, 32, dtype=np.uint64)
        if self.p % 32:
            width[-1] = self.p % 32
        return w | (width << np.uint64(32))

    def time_square_mul(self, reg, iters, a=1, sub=0, per_kernel=True):
        """(total_ms of `iters` squarings, {stage: average ms}); every iteration is bracketed by events here"""
        return Engine.time_square_mul(self, reg, iters, a, sub, per_kernel)
