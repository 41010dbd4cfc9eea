"""The cases of test_gpu_factor_bound.py: every back sweep at the top of its size's exponent range, where the fused factor bound
(plan.hpp fused_factor_limit -> Plan::a_fast) has the least room, with the factors a_fast - 1, a_fast and a_fast + 1.  One list, the
operands per lane and the sequences of register operations, written once and run three ways: on an engine, on Python integers (what the
engine must give) and on the exact model of chain_model.py (whether the device's 64-bit terms were inside their words).
test_factor_bound_cases.py pins every field of the list against tests/host/plan_query.cpp.  No GPU is needed to import this."""
import random
from collections import namedtuple

import chain_model as cm
import orc
from lane_program import _bigmul, mulmod

cm.bigmul = _bigmul      # libgmp where it loads; Python's own product otherwise

# kernels: the value of MI355_KERNELS (None: unset); cols, rows: what plan_query's k: line names; n, c, a_fast: what its plan line gives
Case = namedtuple("Case", "p spec lanes onelaunch kernels n c cols rows a_fast")

# the largest exponents of the 5 2^odd sizes at which every coefficient of the all-maximum squaring is below the field prime, found by
# bisection (test_factor_bound_cases.py repeats it): at the top of these ranges, 983039 and 66559, the largest is 1.25 times the prime
P_40960, P_2560 = 975360, 66048

PLAIN = [
    Case(102399, "m2=16,c=1", 1, False, None, 4096, 1, "generic", "generic", 15),
    Case(127999, "m2=64,c=2", 1, False, None, 5120, 2, "generic", "generic", 53681846),
    Case(393215, "m2=8,c=4", 1, False, None, 16384, 4, "radix8-1024", "generic", 33553406),
    Case(393215, "m2=8,c=4", 1, False, "generic", 16384, 4, "generic", "generic", 33553406),
    Case(393215, "m2=1024", 1, False, None, 16384, 4, "generic", "radix4-planes", 33553406),
    Case(393215, "m2=2048", 1, False, None, 16384, 8, "generic", "rows2048-one", 33553407),
    Case(393215, "m2=4096", 1, False, None, 16384, 16, "generic", "rows4096", 33553407),
    Case(393215, "m2=8192", 1, False, None, 16384, 16, "generic", "rows8192", 33553407),
    Case(102399, "m2=8,c=4", 1, False, None, 4096, 4, "radix4-planes", "generic", 67100671),
    Case(491519, "m2=8,c=4", 1, False, None, 20480, 4, "radix5-1280", "generic", 26842889),
    Case(P_40960, "m2=8,c=2", 1, False, None, 40960, 2, "radix5-2560", "generic", 13421607),
    Case(P_2560, "m2=16,split5", 1, False, None, 2560, 1, "split", "generic", 15),
]
ONELAUNCH = [
    Case(239, None, 3, True, None, 8, 4, "generic", "generic", 1010580539),
    Case(1791, None, 9, True, None, 64, 4, "generic", "generic", 532709120),
    Case(2239, None, 7, True, None, 80, 4, "generic", "generic", 426829046),
    Case(13823, None, 9, True, None, 512, 4, "generic", "generic", 134086783),
    Case(13823, "m2=16,c=2", 9, True, None, 512, 2, "generic", "generic", 134086782),
    Case(127999, None, 3, True, None, 5120, 4, "generic", "generic", 53681847),
    Case(204799, None, 3, True, None, 8192, 4, "generic", "generic", 33552383),
    Case(204799, "m2=2,c=2", 3, True, None, 8192, 2, "generic", "generic", 33552382),
    Case(204799, "m2=4096,c=2", 3, True, None, 8192, 2, "generic", "generic", 33552382),
    Case(132049, None, 3, True, None, 8192, 4, "generic", "generic", 2**32 - 1),
    Case(9941, "m2=16,c=2", 6, True, None, 512, 2, "generic", "generic", 2**32 - 1),
]
LANES = [
    Case(393215, None, 9, False, None, 16384, 4, "generic", "generic", 33553406),
    Case(102399, "c=1", 3, False, None, 4096, 1, "generic", "generic", 15),
]
CASES = PLAIN + ONELAUNCH + LANES

# (c): the cases at the top of a range with n >= 512 and runs of four digits or more, whose carry word at a_fast is at the edge of 64 bits
EDGE_MIN_N, EDGE_FRACTION = 512, 0.99
# (e): exponents at which "2^(q+1) - 1 on every digit" overflows the carry word at a_fast
ALL_WIDE_OVERFLOWS = [44497, 2203, 110503]
# 5 2^odd sizes up to 40960 (the top of the range, its first exponent): the all-maximum squaring passes the field prime at the top
FIVE_ODD = {40: (1159, 928), 160: (4479, 3584), 640: (17279, 13824), 2560: (66559, 53248), 10240: (255999, 204800), 40960: (983039, 786432)}


def case_id(c):
    return "%d-%s-%s%d%s" % (c.p, (c.spec or "auto").replace(",", "_").replace("=", ""), "one" if c.onelaunch else "l", c.lanes,
                             "-" + c.kernels if c.kernels else "")


def token(c):
    """the plan spec with the lanes and the one-launch token, as plan_query and resolve_plan take it"""
    parts = ([c.spec] if c.spec else []) + (["lanes=%d" % c.lanes] if c.lanes > 1 else []) + (["onelaunch"] if c.onelaunch else [])
    return ",".join(parts)


def fused_back(c):
    return c.cols != "split"


def factors(c):
    return [a for a in (c.a_fast - 1, c.a_fast, c.a_fast + 1) if 1 <= a < 2**32]


# ---- operands: values in [0, 2^p - 1], 2^p - 1 being the all-ones words (value 0, every digit at its maximum) ----

KINDS = ("2^p-2", "all-ones", "2^p-2-2^k", "0", "1", "random")
Y_OF = (2, 0, 1, 5, 2, 0)     # the multiplicand's kind for each kind of x: the same set


def kind_value(c, kind, seed):
    p, mp = c.p, (1 << c.p) - 1
    if kind == 0:
        return mp - 1
    if kind == 1:
        return mp
    if kind == 2:   # the first bit of a run: the run before ends below its maximum, the carry chain of the next starts there
        runs = c.n // (2 * c.c)
        k = -(-p * (2 * c.c * (1 + seed % (runs - 1))) // c.n) if runs > 1 else p // 2
        return mp - 1 - (1 << k)
    if kind == 3:
        return 0
    if kind == 4:
        return 1
    return orc.mers_reduce(random.Random(1000003 * p + seed).getrandbits(p), p)


def rounds(c):
    """[[(kind, x, y, z) per lane] per round]: every kind of x on some lane, lanes that differ; z (mul_add's addend) all-maximum"""
    count = -(-len(KINDS) // c.lanes)
    mp = (1 << c.p) - 1
    out = []
    for r in range(count):
        lanes = []
        for l in range(c.lanes):
            seed = l + r * c.lanes            # the running number of the operand set: the same sets whatever the lane count
            kind = seed % len(KINDS)
            ykind = Y_OF[kind] if seed < len(KINDS) else 5             # a kind's second lane: a random multiplicand
            lanes.append((kind, kind_value(c, kind, seed), kind_value(c, ykind, seed + 1), mp - 1 if kind % 2 == 0 else mp))
        out.append(lanes)
    return out


# ---- the sequences.  Registers: 0 the residue, 1 y, 2 y's image, 3 a copy, 4 the addend, 5 the image square_mul_prepare writes ----

R_X, R_Y, R_YIMG, R_COPY, R_ADD, R_PREP, REGS = 0, 1, 2, 3, 4, 5, 6
ENTRIES = ("square_mul", "mul", "square_mul_copy", "mul_copy", "mul_add", "mul_add_self", "square_mul_prepare", "square_mul_n", "square_mul_bits")
BITS, NBITS = bytes([0b10100000]), 3                    # set, clear, set
FOLLOW = (("square_mul", R_X, 1), ("square_mul", R_X, 1), ("mul", R_X, R_YIMG, 1))


def entry_ops(entry, a):
    return {
        "square_mul": [("square_mul", R_X, a)],
        "mul": [("mul", R_X, R_YIMG, a)],
        "square_mul_copy": [("square_mul_copy", R_X, R_COPY, a)],
        "mul_copy": [("mul_copy", R_X, R_YIMG, R_COPY, a)],
        "mul_add": [("mul_add", R_X, R_YIMG, R_ADD, a)],
        "mul_add_self": [("mul_add", R_X, R_YIMG, R_X, a)],
        "square_mul_prepare": [("square_mul_prepare", R_X, R_PREP, a), ("mul", R_X, R_PREP, 1)],
        "square_mul_n": [("square_mul_n", R_X, 3, a, 2)],
        "square_mul_bits": [("square_mul_bits", R_X, a, BITS, NBITS)],
    }[entry]


def refused(c, entry, a):
    """mul_add onto its own destination needs the fused sweep: refused above the bound, and on the split sweeps at every factor"""
    return entry == "mul_add_self" and (a > c.a_fast or not fused_back(c))


def sequence(entry, a):
    return entry_ops(entry, a) + list(FOLLOW)


def outputs(entry):
    return (R_X, R_COPY) if entry in ("square_mul_copy", "mul_copy") else (R_X,)


CHAIN_LENGTH = 6


def chain_ops(c, onto_itself):
    if onto_itself:
        return [("mul_add", R_X, R_YIMG, R_X, c.a_fast)] * CHAIN_LENGTH
    return [("square_mul", R_X, c.a_fast)] * CHAIN_LENGTH


# ---- the three interpreters ----

def run_engine(e, ops):
    for op in ops:
        getattr(e, op[0])(*op[1:])


def run_ints(p, reg, ops):
    """reg: {register: value mod 2^p - 1}, images as the value they were made of"""
    mp = (1 << p) - 1
    for op in ops:
        name = op[0]
        if name == "square_mul":
            reg[op[1]] = mulmod(p, reg[op[1]], reg[op[1]], op[2])
        elif name == "mul":
            reg[op[1]] = mulmod(p, reg[op[1]], reg[op[2]], op[3])
        elif name == "square_mul_copy":
            reg[op[1]] = reg[op[2]] = mulmod(p, reg[op[1]], reg[op[1]], op[3])
        elif name == "mul_copy":
            reg[op[1]] = reg[op[3]] = mulmod(p, reg[op[1]], reg[op[2]], op[4])
        elif name == "mul_add":
            reg[op[1]] = (mulmod(p, reg[op[1]], reg[op[2]], op[4]) + reg[op[3]]) % mp
        elif name == "square_mul_prepare":
            reg[op[2]] = reg[op[1]]
            reg[op[1]] = mulmod(p, reg[op[1]], reg[op[1]], op[3])
        elif name == "square_mul_n":
            for _ in range(op[2]):
                reg[op[1]] = (mulmod(p, reg[op[1]], reg[op[1]], op[3]) - op[4]) % mp
        elif name == "square_mul_bits":
            for i in range(op[4]):
                bit = (op[3][i >> 3] >> (7 - (i & 7))) & 1
                reg[op[1]] = mulmod(p, reg[op[1]], reg[op[1]], op[2] if bit else 1)
        else:
            raise ValueError(name)
    return reg


def run_model(m, images, ops):
    """m: a chain_model.Machine; images: {register: the digits its image was made of}"""
    for op in ops:
        name = op[0]
        if name == "square_mul":
            m.square(op[1], op[2])
        elif name == "mul":
            m.product(op[1], images[op[2]], op[3])
        elif name == "square_mul_copy":
            m.square(op[1], op[3], copy=op[2])
        elif name == "mul_copy":
            m.product(op[1], images[op[2]], op[4], copy=op[3])
        elif name == "mul_add":
            m.product(op[1], images[op[2]], op[4], addend=op[3])
        elif name == "square_mul_prepare":
            images[op[2]] = m.operand(op[1])
            m.square(op[1], op[3])
        elif name == "square_mul_n":
            for _ in range(op[2]):
                m.square(op[1], op[3])
                m.sub(op[1], op[4])
        elif name == "square_mul_bits":
            for i in range(op[4]):
                m.square(op[1], op[2] if (op[3][i >> 3] >> (7 - (i & 7))) & 1 else 1)
        else:
            raise ValueError(name)


def machine(c, memo=None):
    return cm.Machine(c.p, c.n, c.c, c.a_fast, fused_back=fused_back(c), memo=memo)


def red(p, v):
    return orc.mers_reduce(v, p)
