"""(exponent, plan, lanes) cases of the batch tests (test_gpu_batch.py) and what each of them pins, shared by the GPU test and the host
test that checks the claims against the shape rule (test_batch_cases.py).  No GPU is needed to import this.

A batch (include/mi355_batch.h; kernels.hip k_batch) runs a queue of register operations of a one-launch engine in one launch with the
work-group shape of the one-launch products (onelaunch_cases.shape): K whole lanes of TL threads a group."""

# (p, spec, lanes) -> the claim test_batch_cases.py checks, by name
CASES = [
    (127, None, 3),                 # dead_lane_inside_the_only_group: a group made for 4 lanes holds 3
    (1277, None, 9),                # tail_group_of_one_live_lane: 8 + 1
    (9941, None, 5),                # lane_is_a_group_of_256_threads
    (44497, None, 3),               # lane_is_a_group_of_1024_threads
    (1009, None, 5),                # bare_radix5
    (4253, None, 4),                # radix5_with_a_power_of_two_part
    (204799, None, 2),              # largest_size: 128 KiB of LDS; mul_sum as two products
    (132049, "m2=4096,c=2", 2),     # a_team_makes_two_trips
    (9941, "m2=16,c=2", 6),         # runs_of_four_digits
]
PINS = {
    (127, None, 3): "dead_lane_inside_the_only_group",
    (1277, None, 9): "tail_group_of_one_live_lane",
    (9941, None, 5): "lane_is_a_group_of_256_threads",
    (44497, None, 3): "lane_is_a_group_of_1024_threads",
    (1009, None, 5): "bare_radix5",
    (4253, None, 4): "radix5_with_a_power_of_two_part",
    (204799, None, 2): "largest_size",
    (132049, "m2=4096,c=2", 2): "a_team_makes_two_trips",
    (9941, "m2=16,c=2", 6): "runs_of_four_digits",
}
BIT_FOR_BIT_EXPONENTS = (1277, 4253, 204799)
CAPACITY_EXPONENT = 127
NEIGHBOURS = ((204799, 127), (127, 204799))     # (batched engine, plain engine), both orders of size


def case_id(case):
    p, spec, lanes = case
    return "%d%s-lanes%d" % (p, "-" + spec if spec else "", lanes)
