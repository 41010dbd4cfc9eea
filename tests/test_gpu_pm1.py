"""P-1 (prmers_amd/pm1.py) on the engine: stage 1 through square_mul_bits, stage 2 through mul_sum on every row kernel.
142885879 = 2 * 3 * 79 * 301447 + 1 divides M301447 and 43201009 = 2 * 300007 * 72 + 1 divides M300007 (checked with Python integers).
Needs a real MI355X:  python -m pytest tests -m gpu"""
import pytest

from prmers_amd import pm1

pytestmark = pytest.mark.gpu


def test_the_expected_factors_are_factors():
    assert pow(2, 301447, 142885879) == 1 and pow(2, 300007, 43201009) == 1


@pytest.mark.parametrize("plan", [None, "m2=1024", "m2=2048", "m2=4096", "m2=8192"])
def test_stage2_finds_the_factor_on_every_row_kernel(plan):
    p = 301447
    res = pm1.pm1(p, 7, 100, D=30, plan=plan)
    assert res["g1"] == 1 and res["g2"] % 142885879 == 0 and res["fused"] is True
    for f in res["factors"]:
        assert pow(2, p, f) == 1


def test_stage1_finds_the_factor():
    res = pm1.pm1(300007, 10)
    assert res["g1"] % 43201009 == 0 and res["g2"] == 1 and res["D"] is None
    for f in res["factors"]:
        assert pow(2, 300007, f) == 1


def test_forced_composition_returns_the_same_factors():
    from prmers_amd import Engine
    p = 301447
    out = []
    for use in (True, False):
        with Engine(p, pm1.registers_needed(30)) as e:
            out.append(pm1.run(e, p, 7, 100, 30, use_mul_sum=use))
    assert out[0]["factors"] == out[1]["factors"] and out[0]["g2"] % 142885879 == 0
    assert out[0]["fused"] is True and out[1]["fused"] is False and out[1]["products"] > out[0]["products"]
