"""P-1 factoring of a Mersenne number 2^p - 1 on the engine, stages 1 and 2 (the reference: src/modes/RunPM1.cpp).

    python -m prmers_amd.pm1 P B1 [B2] [--D 30|210|2310] [--plan SPEC] [--device N]

Stage 1:  E = 2 p prod_{q <= B1 prime} q^floor(log_q B1),  H = 3^E,  g1 = gcd(H - 1, Mp).  One chain of square_mul with the base
          folded into the carry (Engine.square_mul_bits: one library call for all ~1.44 B1 steps).
Stage 2:  for every prime q in (B1, B2], q = k D +- j with j in J = {1 <= j < D/2, gcd(j, D) = 1}:  A <- A (H^((kD)^2) - H^(j^2)),
          which q divides-in because (kD)^2 - j^2 = (kD - j)(kD + j);  g2 = gcd(A, Mp) with g1 divided out.
          The table holds multiplicand images of N_j = Mp - H^(j^2), so that the difference is a SUM of two images and the step is one
          Engine.mul_sum (one product; see include/mi355_engine.h).  X_k = H^((kD)^2) advances by finite differences:
          G_k = H^((2k+1) D^2), X_{k+1} = X_k G_k, G_{k+1} = G_k H^(2 D^2): two products and two set_multiplicand per k.
          k = 0 is part of the range (X_0 = 1), which is how primes below D/2 are reached.

The driver works on anything with the interface of prmers_amd.Engine.  mul_sum, square_mul_bits and exp_mul are used when the object
has them and replaced by the compositions they stand for when it has not.  Not here: a checkpoint inside P-1, an
error check of stage 1, Pminus1= / Pfactor= worktodo lines, the PrimeNet JSON, a C++ twin.
"""
import argparse
import ctypes
import ctypes.util
import json
import math
import sys

D_CHOICES = (30, 210, 2310)
FIXED_REGISTERS = 10          # H, its image, A, X_k, G_k, the images of X_k, G_k and H^(2 D^2), a work residue, a temporary
R_H, R_HI, R_A, R_X, R_G, R_XI, R_GI, R_CI, R_T, R_TMP = range(FIXED_REGISTERS)
DEFAULT_BUDGET = 32 << 30     # bytes of device memory the register file of stage 2 may take when D is chosen automatically
SLOW_GCD_BITS = 1 << 22       # above this math.gcd takes hours: libgmp or an error


# ---- integers ---------------------------------------------------------------------------------------------------------------------

def primes_upto(n):
    """all primes <= n (sieve of Eratosthenes on a bytearray)"""
    if n < 2:
        return []
    s = bytearray([1]) * (n + 1)
    s[0:2] = b"\0\0"
    for i in range(2, math.isqrt(n) + 1):
        if s[i]:
            s[i * i::i] = bytearray(len(range(i * i, n + 1, i)))
    return [i for i in range(2, n + 1) if s[i]]


def primes_between(lo, hi, segment=1 << 22):
    """primes q with lo < q <= hi, in increasing order (segmented sieve)"""
    if hi <= lo or hi < 2:
        return
    base = primes_upto(math.isqrt(hi))
    start = max(lo + 1, 2)
    while start <= hi:
        end = min(start + segment - 1, hi)
        s = bytearray([1]) * (end - start + 1)
        for q in base:
            if q * q > end:
                break
            first = max(q * q, (start + q - 1) // q * q)
            if first <= end:
                s[first - start::q] = bytearray(len(range(first, end + 1, q)))
        for i, f in enumerate(s):
            if f:
                yield start + i
        start = end + 1


def stage1_exponent(p, b1):
    """E = 2 p prod_{q <= B1 prime} q^floor(log_q B1)"""
    e = 2 * p
    for q in primes_upto(b1):
        qq = q
        while qq * q <= b1:
            qq *= q
        e *= qq
    return e


def residues(D):
    """J = {1 <= j < D/2 : gcd(j, D) = 1}"""
    return [j for j in range(1, D // 2 + 1) if 2 * j < D and math.gcd(j, D) == 1]


def registers_needed(D):
    """registers of an engine that runs stage 2 with this D: the table of |J| images plus FIXED_REGISTERS"""
    if D not in D_CHOICES:
        raise ValueError("D must be one of %s" % (D_CHOICES,))
    return len(residues(D)) + FIXED_REGISTERS


def choose_D(n, b1, b2, budget=DEFAULT_BUDGET):
    """The largest D in {30, 210, 2310} whose register file (registers_needed(D) + the engine's work buffer, 8 n bytes each) fits `budget`
    bytes and that is not wider than the interval (B1, B2] itself (a table larger than the interval is built for nothing).
    n = 2^23: 34 registers = 2.1 GiB for D = 210, 250 registers = 15.6 GiB for D = 2310."""
    best = D_CHOICES[0]
    for D in D_CHOICES[1:]:
        if (registers_needed(D) + 1) * 8 * n <= budget and D <= max(b2 - b1, D_CHOICES[0]):
            best = D
    return best


def stage2_pairs(b1, b2, D):
    """{k: sorted j} so that every prime q in (B1, B2] that does not divide D is k D - j or k D + j for one listed pair.
    k = round(q / D) and j = |q - k D| < D/2; j is coprime to D because q is."""
    pairs = {}
    for q in primes_between(b1, b2):
        if D % q == 0:
            continue   # 2, 3, 5, 7, 11: no residue class; run() puts them into the stage-1 exponent
        k = (q + D // 2) // D
        pairs.setdefault(k, set()).add(abs(q - k * D))
    return {k: sorted(v) for k, v in sorted(pairs.items())}


_gmp = None


def load_gmp():
    """libgmp through ctypes, or None when it does not load"""
    global _gmp
    if _gmp is None:
        try:
            G = ctypes.CDLL(ctypes.util.find_library("gmp") or "libgmp.so.10")

            class Mpz(ctypes.Structure):
                _fields_ = [("alloc", ctypes.c_int), ("size", ctypes.c_int), ("d", ctypes.c_void_p)]
            P = ctypes.POINTER(Mpz)
            G.__gmpz_init.argtypes = [P]
            G.__gmpz_clear.argtypes = [P]
            G.__gmpz_gcd.argtypes = [P, P, P]
            G.__gmpz_import.argtypes = [P, ctypes.c_size_t, ctypes.c_int, ctypes.c_size_t, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
            G.__gmpz_export.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t), ctypes.c_int, ctypes.c_size_t, ctypes.c_int, ctypes.c_size_t, P]
            G.__gmpz_export.restype = ctypes.c_void_p
            G.__gmpz_sizeinbase.argtypes = [P, ctypes.c_int]
            G.__gmpz_sizeinbase.restype = ctypes.c_size_t
            G.Mpz = Mpz
            _gmp = G
        except (OSError, AttributeError):
            _gmp = False
    return _gmp or None


def gcd_gmp(a, b):
    """gcd of two non-negative Python integers through mpz_gcd"""
    G = load_gmp()
    if G is None:
        raise RuntimeError("libgmp does not load")
    za, zb, zg = G.Mpz(), G.Mpz(), G.Mpz()
    for z in (za, zb, zg):
        G.__gmpz_init(ctypes.byref(z))
    try:
        for z, v in ((za, a), (zb, b)):
            raw = int(v).to_bytes((int(v).bit_length() + 7) // 8 or 1, "little")
            G.__gmpz_import(ctypes.byref(z), len(raw), -1, 1, -1, 0, raw)
        G.__gmpz_gcd(ctypes.byref(zg), ctypes.byref(za), ctypes.byref(zb))
        size = (G.__gmpz_sizeinbase(ctypes.byref(zg), 2) + 7) // 8
        buf = ctypes.create_string_buffer(size or 1)
        count = ctypes.c_size_t(0)
        G.__gmpz_export(buf, ctypes.byref(count), -1, 1, -1, 0, ctypes.byref(zg))
        return int.from_bytes(buf.raw[:count.value], "little")
    finally:
        for z in (za, zb, zg):
            G.__gmpz_clear(ctypes.byref(z))


def big_gcd(a, b, use_gmp=None):
    """gcd(a, b): libgmp when it loads (use_gmp=None) or is asked for (True), math.gcd otherwise -- which is refused above about
    2^22 bits, where it would run for hours without a word."""
    if use_gmp is None:
        use_gmp = load_gmp() is not None
    if use_gmp:
        return gcd_gmp(a, b)
    if max(int(a).bit_length(), int(b).bit_length()) > SLOW_GCD_BITS:
        raise RuntimeError("gcd of %d-bit numbers needs libgmp (it did not load); math.gcd would take hours at this size"
                           % max(int(a).bit_length(), int(b).bit_length()))
    return math.gcd(a, b)


# ---- engine operations, with the compositions for objects that lack the fused ones ---------------------------------------------------

class _Ops:
    def __init__(self, eng, use_mul_sum=True):
        self.e = eng
        self.squarings = self.products = 0
        self.has_mul_sum = use_mul_sum and hasattr(eng, "mul_sum")
        self.fused = bool(self.has_mul_sum and getattr(eng, "mul_sum_is_fused", lambda: False)())

    def square_bits(self, reg, factor, value):
        """reg = reg^(2^nbits) factor^value over the nbits = value.bit_length() bits of value"""
        nbits = value.bit_length()
        if nbits == 0:
            return
        if hasattr(self.e, "square_mul_bits"):
            self.e.square_mul_bits(reg, factor, (value << (-nbits % 8)).to_bytes((nbits + 7) // 8, "big"), nbits)
        else:
            for i in range(nbits - 1, -1, -1):
                self.e.square_mul(reg, factor if (value >> i) & 1 else 1)
        self.squarings += nbits

    def mul(self, dst, img):
        self.e.mul(dst, img)
        self.products += 1

    def power(self, dst, base_img, exponent):
        """dst = base^exponent, base given as a multiplicand image; any non-negative exponent"""
        self.e.set(dst, 1)
        for i in range(exponent.bit_length() - 1, -1, -1):
            self.e.square_mul(dst)
            self.squarings += 1
            if (exponent >> i) & 1:
                self.mul(dst, base_img)

    def exp_mul(self, a, h, b, tmp):
        """a = a^h b (0 < h < 2^64); b and tmp end as multiplicand images"""
        if hasattr(self.e, "exp_mul"):
            self.e.exp_mul(a, h, b, tmp)
        else:
            self.e.set_multiplicand(tmp, a)
            for i in range(h.bit_length() - 2, -1, -1):
                self.e.square_mul(a)
                if (h >> i) & 1:
                    self.e.mul(a, tmp)
            self.e.set_multiplicand(b, b)
            self.e.mul(a, b)
        self.squarings += h.bit_length() - 1
        self.products += bin(h).count("1")

    def mul_sum(self, dst, a, b, tmp):
        """dst = dst (a + b) for two multiplicand images"""
        if self.has_mul_sum:
            self.e.mul_sum(dst, a, b, tmp)
        else:
            self.e.copy(tmp, dst)
            self.e.mul(dst, a)
            self.e.mul(tmp, b)
            self.e.add(dst, tmp)
        self.products += 1 if self.fused else 2


def run(eng, p, b1, b2=0, D=None, use_mul_sum=True, use_gmp=None):
    """P-1 on 2^p - 1 with bounds B1 and B2 (B2 <= B1: stage 1 only) on `eng`, an engine for exponent p with at least FIXED_REGISTERS
    registers (stage 1) or registers_needed(D) (stage 2).  use_mul_sum=False forces the two-product composition.
    -> {p, b1, b2, D, factors, g1, g2, squarings, products, fused}"""
    if b1 < 2:
        raise ValueError("B1 must be at least 2")
    mp = (1 << p) - 1
    have = getattr(eng, "reg_count", None)
    stage2 = b2 > b1
    if stage2:
        if D is None:
            D = max([d for d in D_CHOICES if have is None or registers_needed(d) <= have] or [0])
            D = min(D, choose_D(eng.n, b1, b2)) if D else 0
        if D not in D_CHOICES:
            raise ValueError("stage 2 needs D in %s and an engine with registers_needed(D) registers" % (D_CHOICES,))
    need = registers_needed(D) if stage2 else FIXED_REGISTERS
    if have is not None and have < need:
        raise ValueError("the engine has %d registers, P-1 with D = %s needs %d" % (have, D if stage2 else None, need))
    ops = _Ops(eng, use_mul_sum)

    # ---- stage 1 ----
    e = stage1_exponent(p, b1)
    if stage2:   # the primes in (B1, B2] that divide D have no residue class in stage 2
        for q in (2, 3, 5, 7, 11):
            if D % q == 0 and b1 < q <= b2:
                e *= q
    eng.set(R_H, 1)
    ops.square_bits(R_H, 3, e)
    eng.copy(R_T, R_H)
    eng.sub(R_T, 1)
    g1 = big_gcd(eng.get_int(R_T), mp, use_gmp)
    g2 = 1

    # ---- stage 2 ----
    if stage2 and g1 != mp:
        J = residues(D)
        slot = {j: FIXED_REGISTERS + i for i, j in enumerate(J)}
        pairs = stage2_pairs(b1, b2, D)
        eng.set_multiplicand(R_HI, R_H)
        for j in J:   # table: the image of N_j = Mp - H^(j^2)
            s = slot[j]
            eng.copy(R_T, R_H)
            if j > 1:
                eng.set(R_GI, 1)
                ops.exp_mul(R_T, j * j, R_GI, R_TMP)      # T = H^(j^2) * 1
            eng.set(s, 0)
            eng.sub_reg(s, R_T)
            eng.set_multiplicand(s, s)
        if pairs:
            k0, k1 = min(pairs), max(pairs)
            d2 = D * D
            ops.power(R_X, R_HI, k0 * k0 * d2)              # X_k0 = H^((k0 D)^2)
            ops.power(R_G, R_HI, (2 * k0 + 1) * d2)         # G_k0 = H^((2 k0 + 1) D^2)
            ops.power(R_T, R_HI, 2 * d2)
            eng.set_multiplicand(R_CI, R_T)                 # H^(2 D^2)
            eng.set(R_A, 1)
            for k in range(k0, k1 + 1):
                if k in pairs:
                    eng.set_multiplicand(R_XI, R_X)
                    for j in pairs[k]:
                        ops.mul_sum(R_A, R_XI, slot[j], R_TMP)
                if k < k1:
                    eng.set_multiplicand(R_GI, R_G)
                    ops.mul(R_X, R_GI)                      # X_{k+1} = X_k G_k
                    ops.mul(R_G, R_CI)                      # G_{k+1} = G_k H^(2 D^2)
            a = eng.get_int(R_A)
            g = mp if a == 0 else big_gcd(a, mp, use_gmp)
            g2 = g // big_gcd(g, g1, use_gmp)
    factors = [f for f in (g1, g2) if f > 1]
    return {"p": p, "b1": b1, "b2": b2 if stage2 else 0, "D": D if stage2 else None, "factors": factors, "g1": g1, "g2": g2,
            "squarings": ops.squarings, "products": ops.products, "fused": ops.fused}


def pm1(p, b1, b2=0, D=None, plan=None, device=0, budget=DEFAULT_BUDGET):
    """run() on a fresh prmers_amd.Engine sized for the chosen D (default: choose_D for the plan's transform size)"""
    from .engine import Engine, resolve_plan
    if b2 > b1 and D is None:
        n = int(resolve_plan(p, plan).split("n=")[1].split(":")[0])
        D = choose_D(n, b1, b2, budget)
    regs = registers_needed(D) if b2 > b1 else FIXED_REGISTERS
    with Engine(p, regs, device=device, plan=plan) as eng:
        return run(eng, p, b1, b2, D)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m prmers_amd.pm1", description="P-1 factoring of 2^P - 1 (stages 1 and 2) on an MI355X")
    ap.add_argument("p", type=int)
    ap.add_argument("b1", type=int)
    ap.add_argument("b2", type=int, nargs="?", default=0)
    ap.add_argument("--D", type=int, choices=D_CHOICES, default=None, help="stage-2 wheel (default: the largest whose register file fits --budget-gib)")
    ap.add_argument("--budget-gib", type=float, default=DEFAULT_BUDGET / 2**30)
    ap.add_argument("--plan", default=None)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    res = pm1(a.p, a.b1, a.b2, a.D, a.plan, a.device, int(a.budget_gib * 2**30))
    print(json.dumps(res))
    return 0 if res["factors"] else 1


if __name__ == "__main__":
    sys.exit(main())
