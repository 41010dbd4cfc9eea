"""Timings behind DESIGN.md 7a (needs an MI355X except `cpu-step`); one JSON line each.

  python tools/time_proof.py words P [REPS]          wall time of set_words / get_words (host clock around calls that end synchronised)
  python tools/time_proof.py proof P POWER [verify]  build_proof from 2^POWER seeded random point files in a temporary directory (build
                                                     time does not depend on their content), split into file loads and the rest; with
                                                     `verify` also verify_proof on the result (expected verdict on random points: False)
  python tools/time_proof.py cpu-step P              one fold "A <- A^h mod 2^p - 1" (64-bit h) on the CPU with GMP, the host method of
                                                     the reference: 63 squarings and 33 products, each reduced by folding at bit p

MI355_ENGINE_LIB selects the library for `words` (A/B against another build of it)."""
import ctypes
import ctypes.util
import json
import os
import shutil
import sys
import tempfile
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def random_words(rng, p):
    wc = (p + 31) // 32
    w = np.frombuffer(rng.bytes(wc * 4), dtype="<u4").copy()
    if p % 32:
        w[-1] &= (1 << (p % 32)) - 1
    return w


def time_words(p, reps):
    import prmers_amd
    from prmers_amd import Engine
    rng = np.random.default_rng(7)
    with Engine(p, 2) as e:
        w = random_words(rng, p)
        for _ in range(3):                                   # code objects, canonical-form buffers
            e.set_words(0, w); e.square_mul(0); got = e.words(0)
        ts, tg = [], []
        for _ in range(reps):
            e.sync()
            t = time.perf_counter(); e.set_words(0, w); e.sync(); ts.append(time.perf_counter() - t)
            e.square_mul(0); e.sync()                        # a weakly carried register, as after an iteration
            t = time.perf_counter(); got = e.words(0); tg.append(time.perf_counter() - t)
        return {"p": p, "n": e.n, "set_words_ms": [round(1e3 * v, 2) for v in ts], "get_words_ms": [round(1e3 * v, 2) for v in tg],
                "crc_of_square": zlib.crc32(got.tobytes()), "lib": prmers_amd.LIB_PATH}


def time_proof(p, power, do_verify):
    from prmers_amd import Engine, proof as P
    d = tempfile.mkdtemp(prefix="proofpts_")
    try:
        rng = np.random.default_rng(11)
        pts = P.ProofPoints(p, power, d)
        t = time.perf_counter()
        for it in pts.points:
            pts.save(it, random_words(rng, p))
        out = {"p": p, "power": power, "points_written_s": round(time.perf_counter() - t, 2), "folds": (1 << power) - 1 - power}
        load_s = [0.0]
        real_load = P.ProofPoints.load

        def timed_load(self, it):
            t0 = time.perf_counter()
            r = real_load(self, it)
            load_s[0] += time.perf_counter() - t0
            return r
        P.ProofPoints.load = timed_load
        with Engine(p, P.build_registers(power)) as e:
            e.set_words(0, pts.load(p)); e.exp_mul(0, 3, 1, power); e.set_words(1, pts.load(p)); e.words(1)   # warm-up
            e.sync()
            load_s[0] = 0.0
            t = time.perf_counter()
            pr = P.build_proof(e, p, power, d)
            e.sync()
            out["build_s"] = round(time.perf_counter() - t, 2)
        out["build_file_load_s"] = round(load_s[0], 2)
        out["build_engine_and_hash_s"] = round(out["build_s"] - load_s[0], 2)
        if do_verify:
            print(json.dumps(out), flush=True)
            with Engine(p, P.VERIFY_REGISTERS) as e:
                t = time.perf_counter()
                out["verify_verdict_on_random_points"] = P.verify_proof(e, pr)
                out["verify_s"] = round(time.perf_counter() - t, 2)
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def cpu_step(p):
    name = ctypes.util.find_library("gmp") or "libgmp.so.10"
    G = ctypes.CDLL(name)

    class Mpz(ctypes.Structure):
        _fields_ = [("alloc", ctypes.c_int), ("size", ctypes.c_int), ("d", ctypes.c_void_p)]
    for f, args in (("init", 1), ("mul", 3), ("add", 3), ("sub", 3), ("set", 2)):
        getattr(G, "__gmpz_" + f).argtypes = [ctypes.POINTER(Mpz)] * args
    for f in ("tdiv_q_2exp", "tdiv_r_2exp"):
        getattr(G, "__gmpz_" + f).argtypes = [ctypes.POINTER(Mpz), ctypes.POINTER(Mpz), ctypes.c_ulong]
    G.__gmpz_import.argtypes = [ctypes.POINTER(Mpz), ctypes.c_size_t, ctypes.c_int, ctypes.c_size_t, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    G.__gmpz_cmp.argtypes = [ctypes.POINTER(Mpz)] * 2
    G.__gmpz_fdiv_ui.argtypes = [ctypes.POINTER(Mpz), ctypes.c_ulong]
    G.__gmpz_fdiv_ui.restype = ctypes.c_ulong
    a, x, t, m = (Mpz() for _ in range(4))
    for z in (a, x, t, m):
        G.__gmpz_init(ctypes.byref(z))
    w = random_words(np.random.default_rng(1), p)
    G.__gmpz_import(ctypes.byref(a), w.size, -1, 4, -1, 0, w.ctypes.data)
    ones = np.frombuffer(((1 << p) - 1).to_bytes(w.size * 4, "little"), dtype="<u4")
    G.__gmpz_import(ctypes.byref(m), ones.size, -1, 4, -1, 0, ones.ctypes.data)

    def reduce():
        G.__gmpz_tdiv_q_2exp(ctypes.byref(t), ctypes.byref(x), p)
        G.__gmpz_tdiv_r_2exp(ctypes.byref(x), ctypes.byref(x), p)
        G.__gmpz_add(ctypes.byref(x), ctypes.byref(x), ctypes.byref(t))
        if G.__gmpz_cmp(ctypes.byref(x), ctypes.byref(m)) >= 0:
            G.__gmpz_sub(ctypes.byref(x), ctypes.byref(x), ctypes.byref(m))
    h = 0xB5C3A1F097E6D24B
    sq = mu = 0
    t0 = time.perf_counter()
    G.__gmpz_set(ctypes.byref(x), ctypes.byref(a))
    for i in range(62, -1, -1):
        G.__gmpz_mul(ctypes.byref(x), ctypes.byref(x), ctypes.byref(x)); reduce(); sq += 1
        if (h >> i) & 1:
            G.__gmpz_mul(ctypes.byref(x), ctypes.byref(x), ctypes.byref(a)); reduce(); mu += 1
    dt = time.perf_counter() - t0
    if p <= 20000:                                           # the loop is what it says
        v = int.from_bytes(w.tobytes(), "little")
        assert G.__gmpz_fdiv_ui(ctypes.byref(x), 1000003) == pow(v, h, (1 << p) - 1) % 1000003
    return {"p": p, "squarings": sq, "multiplications": mu, "seconds": round(dt, 3)}


def main(argv):
    if len(argv) >= 2 and argv[0] == "words":
        out = time_words(int(argv[1]), int(argv[2]) if len(argv) > 2 else 8)
    elif len(argv) >= 3 and argv[0] == "proof":
        out = time_proof(int(argv[1]), int(argv[2]), len(argv) > 3 and argv[3] == "verify")
    elif len(argv) == 2 and argv[0] == "cpu-step":
        out = cpu_step(int(argv[1]))
    else:
        print(__doc__)
        return 2
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
