"""ECM's affine stage 2 (prmers_amd/ecm.py, stage2="affine") on lane engines: the normalisation on the engine with its lane-wise read
and write, one mul_sum per pair, against the integer model of tests/test_ecm_affine.py and against the projective stage 2 on the same
engine.  The accumulator is prod (x_k - x_j) over affine x-coordinates, so it is the same integer for both stage-1 drivers.
Needs a real MI355X:  python -m pytest tests -m gpu"""
import pytest

from prmers_amd import ecm, ecm_edwards
from test_ecm_affine import m_run_affine

pytestmark = pytest.mark.gpu


def accumulators(e):
    return e.get_ints(ecm.R_A)


def test_two_lanes_three_launches_agree_with_the_projective_run():
    from prmers_amd import Engine
    p, b1, b2, D, sigmas = 3001, 30, 300, 30, [6, 8]
    mp = (1 << p) - 1
    want = [m_run_affine(s, b1, b2, D, mp) for s in sigmas]
    with Engine(p, ecm.registers_needed(D, "affine"), lanes=2) as e:
        out = ecm.run_lanes(e, p, b1, b2, sigmas, D, stage2="affine")
        acc = accumulators(e)
        ref = ecm.run_lanes(e, p, b1, b2, sigmas, D)
        fused = e.mul_sum_is_fused()
    assert [(r["g1"], r["g2"]) for r in out] == [(1, 3217073), (1, 1)] == [(r["g1"], r["g2"]) for r in ref] == [w[:2] for w in want]
    assert all(w[3] for w in want) and acc == [w[2] for w in want]
    assert all((r["stage2"], r["fused_sum"], r["normalised"]) == ("affine", fused, want[0][4]) for r in out)
    assert all("stage2" not in r and "normalised" not in r for r in ref) and "launches" not in out[0]


def test_the_k0_case_in_a_lane_of_a_batched_one_launch_engine():
    from prmers_amd import Engine
    p, b1, b2, D, sigmas = 1009, 20, 104, 210, [7, 12, 8]
    mp = (1 << p) - 1
    want = [m_run_affine(s, b1, b2, D, mp) for s in sigmas]
    with Engine(p, ecm.registers_needed(D, "affine"), lanes=3, onelaunch=True) as e:
        out = ecm.run_lanes(e, p, b1, b2, sigmas, D, batch=True, stage2="affine")
        acc = accumulators(e)
    assert [(r["g1"], r["g2"]) for r in out] == [w[:2] for w in want]
    assert (out[1]["g1"], out[1]["g2"], out[1]["factors"]) == (1, 3454817, [3454817])      # through the Z product: no pair has k > 0
    assert out[0]["factors"] == [] == out[2]["factors"] and want[0][3] and want[2][3]
    assert acc == [w[2] for w in want] == [1, 1, 1]
    assert out[0]["launches"] > 0 and out[0]["normalised"] == 24


def test_giant_blocks_batched_and_the_same_through_the_edwards_driver():
    from prmers_amd import Engine
    p, b1, b2, D, sigmas = 10007, 20, 500, 210, [10, 11]
    mp = (1 << p) - 1
    want = [m_run_affine(s, b1, b2, D, mp) for s in sigmas]
    assert want[0][:2] == (1, 240169) and all(w[3] for w in want)
    with Engine(p, ecm.registers_needed(D, "affine"), lanes=2, onelaunch=True) as e:
        out = ecm.run_lanes(e, p, b1, b2, sigmas, D, batch=True, stage2="affine")
        acc = accumulators(e)
        plain = ecm.run_lanes(e, p, b1, b2, sigmas, D, stage2="affine")
        acc_plain = accumulators(e)
        ed = ecm_edwards.run_lanes(e, p, b1, b2, sigmas, D, batch=True, stage2="affine")
        acc_ed = accumulators(e)
        fused = e.mul_sum_is_fused()
    for res in (out, plain, ed):
        assert [(r["g1"], r["g2"]) for r in res] == [w[:2] for w in want]
        assert all((r["stage2"], r["fused_sum"], r["normalised"]) == ("affine", fused, want[0][4]) for r in res)
    assert acc == acc_plain == acc_ed == [w[2] for w in want]
    assert out[0]["launches"] > 0 and "launches" not in plain[0] and ed[0]["curve"] == "edwards" and ed[0]["rollbacks"] == 0
    assert want[0][4] == 24 + 2                    # the table and the giant points of k = 1 and 2


def test_a_plan_without_the_fused_sum():
    """p = 204799 (tests/mul_sum_cases.py): n = 8192 at its largest digit width has no room for the summed operand, so the engine's
    mul_sum is its two-product composition; the accumulator is the model's all the same.  (B1 = 3: the model's products of 204799-bit
    integers are what takes the time here.)"""
    from prmers_amd import Engine
    import mul_sum_cases
    p, b1, b2, D, sigmas = 204799, 3, 40, 30, [7, 9]
    assert (p, None) in mul_sum_cases.CASES
    mp = (1 << p) - 1
    want = [m_run_affine(s, b1, b2, D, mp, ecm.suyama(s, mp)) for s in sigmas]
    with Engine(p, ecm.registers_needed(D, "affine"), lanes=2) as e:
        assert not e.mul_sum_is_fused()
        out = ecm.run_lanes(e, p, b1, b2, sigmas, D, stage2="affine")
        acc = accumulators(e)
    # 204799 = 7 * 29257, so 127 divides: both curves meet the small factors in a block's Z product, get the inverse 1 there and ride on
    assert [(r["g1"], r["g2"]) for r in out] == [w[:2] for w in want] == [(1, 30353), (127, 239)] and not any(w[3] for w in want)
    assert acc == [w[2] for w in want]
    assert all(r["fused_sum"] is False and r["normalised"] == 4 + 1 for r in out)
