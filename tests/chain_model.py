"""An exact model of one product's back sweep on Python integers (numpy for the O(n^2) sums): the unweighted coefficients z_k of the
weighted cyclic convolution, the carry chain of adc_mul (kernels.hip) run by run, the carry-in of the following sweep (take_carry_in),
k_scale, k_linear's sum and the value a register stands for.  Nothing here wraps at 2^64: every 64-bit term is computed exactly and its
maximum reported, so that a caller can say whether the device's arithmetic was inside its words.  Imports no engine code, needs no GPU.

Digit j of an exponent p on n digits starts at bit ceil(p j / n).  A run is 2C consecutive natural digits (Plan::pos puts them next to
each other in memory); a run's carry word belongs to the first digits of the next run in digit order, the last run's to digit 0."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

FIELD = 2**64 - 2**32 + 1
LIM = 1 << 64
DIGIT_LIM = 1 << 31          # weigh_pair shifts a uint32_t digit left by one


@lru_cache(maxsize=8)
def offsets(p, n):
    """first bit of digit j, j = 0 .. n"""
    return tuple(-(-p * j // n) for j in range(n + 1))


@lru_cache(maxsize=8)
def widths(p, n):
    o = offsets(p, n)
    return tuple(o[j + 1] - o[j] for j in range(n))


@lru_cache(maxsize=8)
def weight_exponents(p, n):
    """f_j = n ceil(p j / n) - p j: digit j's weight is 2^(f_j / n)"""
    return tuple((-p * j) % n for j in range(n))


def to_digits(p, n, v):
    """the digits of 0 <= v < 2^p, each inside its width (v = 2^p - 1, the all-ones words, has every digit at its maximum)"""
    o = offsets(p, n)
    out = [0] * n
    todo = [(v, 0, n)]                     # halves of halves: shifting the whole value once per digit is quadratic
    while todo:
        part, lo, hi = todo.pop()
        if hi - lo == 1:
            out[lo] = part
            continue
        mid = (lo + hi) // 2
        cut = o[mid] - o[lo]
        todo.append((part & ((1 << cut) - 1), lo, mid))
        todo.append((part >> cut, mid, hi))
    return out


def coefficients(p, n, x, y):
    """z_k = sum over i + j = k (mod n) of x_i y_j 2^c(i,j), c(i,j) = 1 iff f_i + f_j >= n: O(n^2), limbs in int64 recombined as integers"""
    f = np.array(weight_exponents(p, n), dtype=np.int64)
    bits = max(1, max(int(v).bit_length() for v in list(x) + list(y)))
    limb = max(1, min(13, (62 - n.bit_length()) // 2))     # n products of two limbs, doubled, inside 63 bits
    count = -(-bits // limb)
    mask = (1 << limb) - 1
    xl = [np.array([(int(v) >> (limb * a)) & mask for v in x], dtype=np.int64) for a in range(count)]
    yl = [np.array([(int(v) >> (limb * a)) & mask for v in y], dtype=np.int64) for a in range(count)]
    i = np.arange(n)
    z = []
    for k in range(n):
        j = (k - i) % n
        dbl = ((f + f[j]) >= n).astype(np.int64)
        total = 0
        for a in range(count):
            xa = xl[a] << dbl
            for b in range(count):
                total += int(np.dot(xa, yl[b][j])) << (limb * (a + b))
        z.append(total)
    return z


bigmul = lambda a, b: a * b      # a caller may put a faster exact product of two integers here (the tests: libgmp where it loads)


def _cyclic(n, x, y):
    """plain cyclic convolution of two vectors of values below 2^64 by one big-integer product, 16 bytes per coefficient (sums < 2^128)
    -> an array of Python integers"""
    def pack(d):
        a = np.zeros((n, 2), dtype="<u8")
        a[:, 0] = d
        return int.from_bytes(a.tobytes(), "little")
    w = np.frombuffer(bigmul(pack(x), pack(y)).to_bytes(32 * n, "little"), dtype="<u8").reshape(2 * n, 2)
    L = w[:, 0].astype(object) + (w[:, 1].astype(object) << 64)
    return L[:n] + L[n:]


def coefficients_fast(p, n, x, y):
    """the same z_k from three plain cyclic convolutions (big-integer products), for the sizes at which O(n^2) takes minutes.  With
    i + j = k (mod n) the sum f_i + f_j is f_k or f_k + n, the latter exactly where c(i,j) = 1.  So with S0 = sum x_i y_j and
    S1 = the same sum over the pairs with c = 1:  sum x_i y_j (f_i + f_j) = f_k S0 + n S1, and z_k = S0 + S1."""
    f = np.array(weight_exponents(p, n), dtype=np.uint64)
    same = x is y or list(x) == list(y)
    x, y = np.array(x, dtype=np.uint64), np.array(y, dtype=np.uint64)
    assert max(int(x.max()), int(y.max())) * n < LIM and 2 * n.bit_length() + 64 < 128
    if not x.any() or not y.any():
        return [0] * n
    s0 = _cyclic(n, x, y)
    a = _cyclic(n, x * f, y)
    b = a if same else _cyclic(n, x, y * f)
    s1 = a + b - f.astype(object) * s0
    assert not (s1 % n).any() and (s1 >= 0).all()
    return list(s0 + s1 // n)


Sweep = namedtuple("Sweep", "digits carries max_r max_carry max_z")


def back_sweep(p, n, C, z, a, addend=None):
    """adc_mul over every run of 2C digits from carry 0 (its a == 1 branch included): digits, one carry word per run, the largest r and
    the largest carry seen, max z_k"""
    w = widths(p, n)
    digits, carries, max_r, max_c = [0] * n, [], 0, 0
    for start in range(0, n, 2 * C):
        carry = 0
        for j in range(start, start + 2 * C):
            u, mask, ad = z[j], (1 << w[j]) - 1, (addend[j] if addend is not None else 0)
            if a == 1:
                r = u + carry + ad
                carry = r >> w[j]
            else:
                dlo, chi = u & mask, u >> w[j]
                r = dlo * a + carry + ad
                carry = (r >> w[j]) + chi * a
            digits[j] = r & mask
            max_r, max_c = max(max_r, r), max(max_c, carry)
        carries.append(carry)
    return Sweep(digits, carries, max_r, max_c, max(z))


Taken = namedtuple("Taken", "digits max_sum max_digit")


def carry_in(p, n, C, digits, carries):
    """take_carry_in on every run: the carry word of the run before goes into three masked digits and the rest stays on the fourth
    (C >= 2), or into one masked digit with the rest on the second (C = 1): the digits a front sweep weighs, the largest v + c and the
    largest digit"""
    if carries is None:
        return Taken(list(digits), 0, max(digits))
    w = widths(p, n)
    out, ndig, max_sum = list(digits), 2 * C, 0
    for run in range(n // ndig):
        c = carries[run - 1]
        for k in range(min(ndig, 4)):
            j = run * ndig + k
            v = out[j] + c
            max_sum = max(max_sum, v)
            if k < 3 and k + 1 < ndig:
                out[j], c = v & ((1 << w[j]) - 1), v >> w[j]
            else:
                out[j], c = v, 0
    return Taken(out, max_sum, max(out))


def relax(p, n, digits):
    """one local carry pass (canon.hip k_relax): every digit keeps its width's bits and takes what its left neighbour had above its own"""
    w = widths(p, n)
    return [(digits[j] & ((1 << w[j]) - 1)) + (digits[j - 1] >> w[j - 1]) for j in range(n)]


def relax_passes(n, q, excess=None):
    """the number of passes Engine::carry_fix_now adds on a plan with runs of two digits"""
    if excess is None:
        excess = (n.bit_length() - 1) + 1 + 4 - 2
    count = 0
    while excess > q - 2:
        count, excess = count + 1, excess - q
    return count


def scale(p, n, C, digits, carries, a):
    """k_scale: the digits with their carry-in taken, times a with a carry through the run -> a Sweep (max_z: the largest digit read)"""
    t = carry_in(p, n, C, digits, carries)
    w = widths(p, n)
    out, cs, max_r, max_c = [0] * n, [], t.max_sum, 0
    for start in range(0, n, 2 * C):
        c = 0
        for j in range(start, start + 2 * C):
            v = t.digits[j] * a + c
            out[j], c = v & ((1 << w[j]) - 1), v >> w[j]
            max_r, max_c = max(max_r, v), max(max_c, c)
        cs.append(c)
    return Sweep(out, cs, max_r, max_c, t.max_digit)


def add(p, n, C, da, ca, db, cb):
    """k_linear's sum of two registers with their carry-ins taken -> a Sweep"""
    ta, tb = carry_in(p, n, C, da, ca), carry_in(p, n, C, db, cb)
    w = widths(p, n)
    out, cs, max_r = [0] * n, [], max(ta.max_sum, tb.max_sum)
    for start in range(0, n, 2 * C):
        c = 0
        for j in range(start, start + 2 * C):
            v = ta.digits[j] + tb.digits[j] + c
            out[j], c = v & ((1 << w[j]) - 1), v >> w[j]
            max_r = max(max_r, v)
        cs.append(c)
    return Sweep(out, cs, max_r, max(cs), max(ta.max_digit, tb.max_digit))


def sub_small(p, n, digits, v):
    """k_sub_small: digits - v with a cyclic borrow through the digit vector; pending carry words stay as they are"""
    w = widths(p, n)
    out, borrow = list(digits), v
    for _ in range(3):
        for j in range(n):
            if not borrow:
                return out
            if out[j] >= borrow:
                out[j], borrow = out[j] - borrow, 0
            else:
                k = (borrow - out[j] + (1 << w[j]) - 1) >> w[j]
                out[j], borrow = out[j] + (k << w[j]) - borrow, k
    assert not borrow
    return out


def value(p, n, C, digits, carries=None):
    """what digits plus pending carry words stand for, mod 2^p - 1"""
    o = offsets(p, n)
    terms = [int(d) for d in digits]
    if carries is not None:
        for run, c in enumerate(carries):
            terms[((run + 1) * 2 * C) % n] += int(c)
    parts = list(zip(terms, o))            # sum of terms[j] << o[j], neighbours first: no long sum is shifted more than log2 n times
    while len(parts) > 1:
        merged = [(parts[i][0] + (parts[i + 1][0] << (parts[i + 1][1] - parts[i][1])), parts[i][1]) for i in range(0, len(parts) - 1, 2)]
        parts = merged + ([parts[-1]] if len(parts) % 2 else [])
    v = parts[0][0]
    mp = (1 << p) - 1
    while v >> p:
        v = (v & mp) + (v >> p)
    return 0 if v == mp else v


class Trace:
    """the 64-bit terms of a sequence of operations: the maxima over all of them, and which operation set each"""

    def __init__(self):
        self.max_z = self.max_r = self.max_carry = self.max_sum = self.max_digit = 0

    def sweep(self, s):
        self.max_z, self.max_r, self.max_carry = max(self.max_z, s.max_z), max(self.max_r, s.max_r), max(self.max_carry, s.max_carry)

    def taken(self, t):
        self.max_sum, self.max_digit = max(self.max_sum, t.max_sum), max(self.max_digit, t.max_digit)

    def inside(self):
        """every term inside the words the device holds it in"""
        return self.max_z < FIELD and self.max_r < LIM and self.max_carry < LIM and self.max_sum < LIM and self.max_digit < DIGIT_LIM


class Machine:
    """Registers of one lane as (digits, carry words or None), with the engine's operations restated on the model above; every term goes
    through a Trace.  a_fast: the plan's fused bound (a larger factor runs as factor 1 plus scale, as the engine does it)."""

    def __init__(self, p, n, C, a_fast, fast=True, fused_back=True, memo=None):
        """fused_back: False on the split column sweeps, where mul_add is mul + add; memo: a dict shared by machines of the same
        (p, n, C), so that equal products of equal operands are computed once"""
        self.p, self.n, self.C, self.a_fast, self.fused_back = p, n, C, a_fast, fused_back
        self.q = p // n
        self.coeff = coefficients_fast if fast else coefficients
        self.memo = {} if memo is None else memo
        self.trace = Trace()
        self.reg = {}
        self._taken = None       # the last carry-in: a squaring asks for its operand twice

    def set(self, r, v):
        self.reg[r] = (to_digits(self.p, self.n, v), None)

    def copy(self, dst, src):
        self.reg[dst] = self.reg[src]

    def sub(self, r, v):
        d, c = self.reg[r]
        self.reg[r] = (sub_small(self.p, self.n, d, v), c)

    def get(self, r):
        d, c = self.reg[r]
        return value(self.p, self.n, self.C, d, c)

    def operand(self, r):
        """the digits a front sweep weighs"""
        d, c = self.reg[r]
        if self._taken is None or self._taken[0] is not d or self._taken[1] is not c:
            self._taken = (d, c, carry_in(self.p, self.n, self.C, d, c))
        self.trace.taken(self._taken[2])
        return self._taken[2].digits

    def _settle(self, s, excess=None):
        """after a back sweep or a scale: runs of two digits take their carries at once (carry_fix_now), others leave them pending"""
        self.trace.sweep(s)
        if self.C >= 2:
            return (s.digits, s.carries)
        t = carry_in(self.p, self.n, 1, s.digits, s.carries)
        self.trace.taken(t)
        d = t.digits
        for _ in range(relax_passes(self.n, self.q, excess)):
            d = relax(self.p, self.n, d)
        return (d, None)

    def product(self, dst, ydigits, a=1, addend=None, copy=None):
        """dst = dst * y * a (+ addend register), y given as the digits its image was made of; copy: a second destination"""
        fused = a <= self.a_fast
        x = self.operand(dst)
        ad = self.operand(addend) if (addend is not None and fused and self.fused_back) else None
        key = (tuple(x), tuple(ydigits), a if fused else 1, None if ad is None else tuple(ad))
        if key not in self.memo:
            z = self.coeff(self.p, self.n, x, ydigits)
            self.memo[key] = back_sweep(self.p, self.n, self.C, z, key[2], ad)
        b = self.reg[addend] if addend is not None else None      # (the addend may be dst)
        out = self._settle(self.memo[key])
        if not fused:
            self.trace.taken(carry_in(self.p, self.n, self.C, out[0], out[1]))
            out = self._settle(scale(self.p, self.n, self.C, out[0], out[1], a), 34 - self.q)
        if addend is not None and ad is None:
            self.trace.taken(carry_in(self.p, self.n, self.C, out[0], out[1]))
            self.trace.taken(carry_in(self.p, self.n, self.C, b[0], b[1]))
            out = self._settle(add(self.p, self.n, self.C, out[0], out[1], b[0], b[1]))
        self.reg[dst] = out
        if copy is not None:
            self.reg[copy] = out

    def square(self, r, a=1, copy=None):
        self.product(r, self.operand(r), a, copy=copy)
