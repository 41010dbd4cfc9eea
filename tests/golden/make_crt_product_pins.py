#!/usr/bin/env python3
"""Generate tests/golden/crt_product_pins.json: products of seeded operands at the exponents of tests/crt_cases.py above its pin threshold,
independent of the oracle and of the engine.

With x, y the seeded operands of a run (crt_cases.operand_bytes) and A = 2^32 - 1, all mod 2^p - 1:
    v1 = x^2 A      v2 = v1 y A      xy = x y      v3 = (v2 - 2)^2 y
each recorded as its res64 and the SHA-256 of its canonical little-endian 32-bit words.  Arithmetic: libgmp through ctypes (mpz_mul +
shift/add reduction mod 2^p-1) -- nothing from the reference is imported or executed.  Run: python tests/golden/make_crt_product_pins.py
"""
import ctypes
import ctypes.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import crt_cases  # noqa: E402

gmp = ctypes.CDLL(ctypes.util.find_library("gmp") or "libgmp.so.10")


class Mpz(ctypes.Structure):
    _fields_ = [("alloc", ctypes.c_int), ("size", ctypes.c_int), ("d", ctypes.c_void_p)]


def fn(name, *argtypes, restype=None):
    f = getattr(gmp, "__gmpz_" + name)
    f.argtypes, f.restype = list(argtypes), restype
    return f


P_ = ctypes.POINTER(Mpz)
init, clear = fn("init", P_), fn("clear", P_)
set_ui = fn("set_ui", P_, ctypes.c_ulong)
set_ = fn("set", P_, P_)
mul = fn("mul", P_, P_, P_)
mul_ui = fn("mul_ui", P_, P_, ctypes.c_ulong)
add = fn("add", P_, P_, P_)
sub = fn("sub", P_, P_, P_)
cmp_ = fn("cmp", P_, P_, restype=ctypes.c_int)
cmp_ui = fn("cmp_ui", P_, ctypes.c_ulong, restype=ctypes.c_int)
tdiv_r_2exp = fn("tdiv_r_2exp", P_, P_, ctypes.c_ulong)
tdiv_q_2exp = fn("tdiv_q_2exp", P_, P_, ctypes.c_ulong)
mul_2exp = fn("mul_2exp", P_, P_, ctypes.c_ulong)
sub_ui = fn("sub_ui", P_, P_, ctypes.c_ulong)
import_ = fn("import", P_, ctypes.c_size_t, ctypes.c_int, ctypes.c_size_t, ctypes.c_int, ctypes.c_size_t, ctypes.c_char_p)
export = fn("export", ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t), ctypes.c_int, ctypes.c_size_t, ctypes.c_int,
            ctypes.c_size_t, P_, restype=ctypes.c_void_p)


def words_of(x, p):
    """canonical little-endian 32-bit words of x (0 <= x < 2^p-1), ceil(p/32) words"""
    nw = (p + 31) // 32
    buf = (ctypes.c_uint32 * (nw + 2))()
    cnt = ctypes.c_size_t(0)
    export(buf, ctypes.byref(cnt), -1, 4, -1, 0, ctypes.byref(x))
    return bytes(buf)[: 4 * nw]


class Mersenne:
    """values mod 2^p - 1 in mpz variables"""

    def __init__(self, p):
        self.p = p
        self.hi, self.mp = Mpz(), Mpz()
        for z in (self.hi, self.mp):
            init(ctypes.byref(z))
        set_ui(ctypes.byref(self.mp), 1)
        mul_2exp(ctypes.byref(self.mp), ctypes.byref(self.mp), p)
        sub_ui(ctypes.byref(self.mp), ctypes.byref(self.mp), 1)

    def new(self, data=None):
        z = Mpz()
        init(ctypes.byref(z))
        if data is not None:
            import_(ctypes.byref(z), len(data), -1, 1, -1, 0, data)
        return z

    def fold(self, t):
        """t <- t mod 2^p - 1 for 0 <= t < 2^(2p + 64): t = hi 2^p + lo => hi + lo, until it fits"""
        r = ctypes.byref
        while cmp_(r(t), r(self.mp)) > 0:
            tdiv_q_2exp(r(self.hi), r(t), self.p)
            tdiv_r_2exp(r(t), r(t), self.p)
            add(r(t), r(t), r(self.hi))
        if cmp_(r(t), r(self.mp)) == 0:
            set_ui(r(t), 0)

    def mul(self, out, a, b, factor=1):
        """out <- a b factor"""
        r = ctypes.byref
        mul(r(out), r(a), r(b))
        self.fold(out)
        if factor != 1:
            mul_ui(r(out), r(out), factor)
            self.fold(out)

    def sub_small(self, out, a, k):
        """out <- a - k for a small k"""
        r = ctypes.byref
        set_(r(out), r(a))
        if cmp_ui(r(out), k) < 0:
            add(r(out), r(out), r(self.mp))
        sub_ui(r(out), r(out), k)


def pin(odd, ln, which):
    p = crt_cases.exponent(odd, ln, which)
    seed = crt_cases.seed_of(odd, ln)
    M = Mersenne(p)
    xb, yb = crt_cases.operand_bytes(seed, p)
    x, y, v, t, xy = M.new(xb), M.new(yb), M.new(), M.new(), M.new()
    out = {"odd": odd, "ln": ln, "p": p, "seed": seed}
    M.mul(v, x, x, crt_cases.A)
    out["v1"] = crt_cases.stamp(words_of(v, p))
    M.mul(v, v, y, crt_cases.A)
    out["v2"] = crt_cases.stamp(words_of(v, p))
    M.mul(xy, x, y)
    out["xy"] = crt_cases.stamp(words_of(xy, p))
    M.sub_small(t, v, 2)
    M.mul(v, t, t)
    M.mul(v, v, y)
    out["v3"] = crt_cases.stamp(words_of(v, p))
    for z in (x, y, v, t, xy, M.hi, M.mp):
        clear(ctypes.byref(z))
    sys.stderr.write("%s p=%d v3 res64=%s\n" % (crt_cases.pin_key(odd, ln, which), p, out["v3"]["res64"]))
    return out


if __name__ == "__main__":
    doc = {"_source": "libgmp via ctypes (tests/golden/make_crt_product_pins.py); x, y = crt_cases.operand_bytes(seed, p), A = 2^32 - 1, "
                      "v1 = x^2 A, v2 = v1 y A, xy = x y, v3 = (v2 - 2)^2 y mod 2^p-1; res64 and the SHA-256 of the canonical "
                      "little-endian 32-bit words",
           "pins": {crt_cases.pin_key(*r): pin(*r) for r in crt_cases.pinned_runs()}}
    path = os.path.join(HERE, "crt_product_pins.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", path)
