"""(exponent, plan, lanes) cases of the wide lane tests (test_gpu_lanes_wide.py), and the work-group rule of the generic kernels restated,
shared by the GPU test and the host test that checks which thread shapes the cases reach (test_lane_cases.py).

A lane engine launches `lanes` times the tiles of its plan, and kernels.hip block_for_small picks the work-group size from that count: a
small transform's tile can therefore run with a work-group no single-lane engine of the shape gets, and the generic bodies choose their
form (plane per thread, pair per thread, a quarter of the tile) from (pairs, threads)."""
import re

CASES = [
    (127, None, 512), (1277, None, 512),       # more lanes than anything else in the launch: 1 and 4 tiles per lane
    (9941, None, 64),
    (44497, None, 300),
    (86243, None, 16), (86243, None, 17),      # rows of 128: 128 threads, then 64
    (216091, None, 16), (216091, None, 17),    # radix-5 columns of 320 pairs: 512 threads, then 128
    (301447, None, 4), (301447, None, 5), (301447, None, 8), (301447, None, 9), (301447, None, 64),   # columns switch after 4 lanes, rows after 8
    (3021377, None, 4), (3021377, None, 5),    # radix-5 columns of 1280 pairs: 1024 threads, then 512
    (1600589, "m2=32,c=4", 32), (1600589, "m2=32,c=4", 33),   # an 80 KiB column tile of 5120 pairs: 1024 threads, then 512
]

# (p, spec, sweep, pairs per tile, groups per lane, threads while lanes x groups <= 256, threads beyond)
TABLE = [
    (301447, None, "columns", 128, 64, 128, 64),
    (301447, None, "rows", 256, 32, 256, 64),
    (86243, None, "rows", 128, 16, 128, 64),
    (216091, None, "columns", 320, 16, 512, 128),
    (3021377, None, "columns", 1280, 64, 1024, 512),
    (1600589, "m2=32,c=4", "columns", 5120, 8, 1024, 512),
]
SHAPES_BEYOND = {(5120, 512), (1280, 512), (320, 128), (256, 64), (128, 64)}   # (pairs, threads) only a lane engine reaches
SMALL_LANE_COUNTS = (64, 300, 512)      # each at an exponent of at most SMALL_P: the counts ECM is meant to run at
SMALL_P = 44497
# (p, spec, lanes, factor): factors above the plan's fused bound (plan.hpp a_fast; 15 on runs of two digits), which run as factor 1 and the
# run-wise factor pass after it, or as the base-class composition
FACTOR_CASES = [(86243, "c=1", 3, 16), (86243, "c=1", 3, 2**32 - 5), (301447, None, 9, 2**32 - 5), (756839, None, 5, 2**32 - 5)]
A_FAST = {(86243, "c=1"): 15, (301447, None): 1073183519, (756839, None): 16776959}
SMALL_FACTOR = 3                        # at or below every plan's bound: mul_add with add_src == dst takes it
REGS = 10                               # lane_program.REGS; an engine has one more slot, the work buffer
BUDGET_BYTES = 1 << 30
GROUP_SWITCH = 256                      # kernels.hip block_for_small: work-groups of the whole launch


def block_for(work):
    b = 64
    while b < 512 and b < work:
        b <<= 1
    return b


def threads(pairs, groups_per_lane, lanes):
    """kernels.hip block_for_small(pl, pairs, lanes)"""
    if lanes * groups_per_lane > GROUP_SWITCH:
        return block_for(pairs // 4 or 1)
    b = 64
    while b < 1024 and b < pairs:
        b <<= 1
    return b


def grid_of(plan_text):
    """(n, m1, m2, c) of a plan string such as marin-hip:n=512:m1=8:m2=32:c=4"""
    f = dict(re.findall(r"(n|m1|m2|c)=(\d+)", plan_text))
    return int(f["n"]), int(f["m1"]), int(f["m2"]), int(f["c"])


def sweeps(m1, m2, c):
    """sweep -> (pairs per tile, groups per lane): a column tile is m1 x c pairs, a row is m2"""
    return {"columns": (m1 * c, m2 // c), "rows": (m2, m1)}


def register_bytes(n, lanes, regs=REGS):
    return (regs + 1) * lanes * 8 * n


def case_id(case):
    p, spec, lanes = case
    return "%d%s-lanes%d" % (p, "-" + spec if spec else "", lanes)
