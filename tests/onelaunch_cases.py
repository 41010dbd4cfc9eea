"""(exponent, plan, lanes) cases of the one-launch tests (test_gpu_onelaunch.py) and the shape rule of the one-launch kernel restated
(plan.hpp onelaunch_shape), shared by the GPU test and the host test that checks what the cases reach (test_onelaunch_cases.py).

An engine with the plan token `onelaunch` runs front sweep, row sweep and back sweep of a lane in one work-group: K whole lanes with TL
threads each.  TL is one thread per pair up to 1024 threads (640 where the transform has a radix-5 stage), K what fills a group of about
256 threads, but no more than the lane count rounded up to a power of two."""
import re

CASES = [
    (127, None, 512), (127, None, 3),          # M1 = 1, one tile of 4 pairs: 64 lanes a group; 3 lanes in a group made for 4
    (1277, None, 64), (1277, None, 300), (1277, None, 512), (1277, None, 9),   # 8 lanes a group: 300 = 37 x 8 + 4, 9 = 8 + 1
    (9941, None, 64), (9941, None, 300), (9941, None, 512),                    # a lane is a group of 256 threads
    (44497, None, 64), (44497, None, 300), (44497, None, 512),                 # 1024 threads
    (1009, None, 5), (2203, None, 7),          # n = 40, 80: columns of a bare radix-5
    (4253, None, 4), (110503, None, 3),        # n = 160, 5120: radix 5 with a power-of-two part; 640 threads at n = 5120
    (204799, None, 3),                         # the largest size: 128 KiB of LDS, mul_sum as two products
    (44497, "m2=256,c=16", 5), (9941, "m2=16,c=2", 6),   # runs of 32 and of 4 digits
    (132049, "m2=4096,c=2", 3), (132049, "m2=2,c=2", 3),   # 2048 tiles of 2 pairs, 2048 rows of 2 pairs: a team makes two trips
]
LARGEST_P, FIRST_REFUSED_P, MAX_N = 204799, 204800, 8192
SMALL_LANE_COUNTS = (64, 300, 512)
SMALL_EXPONENTS = (1277, 9941, 44497)
BARE_RADIX5 = {1009: 40, 2203: 80}             # p -> n: M1 = 5
RADIX5_WITH_POW2 = {4253: 160, 110503: 5120}
RUN_LENGTHS = {(44497, "m2=256,c=16"): 16, (9941, "m2=16,c=2"): 2}
REFUSED = [(FIRST_REFUSED_P, "onelaunch"), (9941, "c=1,onelaunch"), (9941, "crt:9,onelaunch"), (110503, "split5,onelaunch")]
FACTOR_CASE = (2203, None, 7, 2**32 - 5)        # (p, spec, lanes, factor): above the plan's fused bound (plan.hpp a_fast)
REGS = 10                                      # lane_program.REGS; an engine has one more slot, the work buffer
BUDGET_BYTES = 1 << 30
GROUP_THREADS = 256
LDS_BYTES = 160 * 1024


def pow2_ceil(v):
    b = 1
    while b < v:
        b <<= 1
    return b


def shape(n, lanes):
    """plan.hpp onelaunch_shape -> (TL, K, groups, LDS bytes of a group)"""
    m = n // 2
    tl = min(m, 640 if m % 5 == 0 else 1024)
    k = min(max(1, GROUP_THREADS // tl), pow2_ceil(lanes))
    return tl, k, (lanes + k - 1) // k, k * m * 32


def fields(plan_text):
    """the numbers of a plan string such as marin-hip:n=512:m1=8:m2=32:c=4"""
    return {k: int(v) for k, v in re.findall(r"(n|m1|m2|c|lanes)=(\d+)", plan_text)}


def token(spec, lanes=1):
    """the plan spec of an engine with these lanes and one-launch products"""
    return ",".join(t for t in (spec, "lanes=%d" % lanes if lanes != 1 else None, "onelaunch") if t)


def register_bytes(n, lanes, regs=REGS):
    return (regs + 1) * lanes * 8 * n


def case_id(case):
    p, spec, lanes = case
    return "%d%s-lanes%d" % (p, "-" + spec if spec else "", lanes)
