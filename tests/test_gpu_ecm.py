"""ECM (prmers_amd/ecm.py) on the engine, on every row kernel: stage 1 through square_mul_prepare, stage 2 over the wheel.
142885879 divides M301447 and 43201009 divides M300007.  The sigmas are the first ones from 6 upwards with the wanted outcome for the
integer model of tests/test_ecm.py run modulo the factor alone (m_run(sigma, b1, b2, 30, factor)), with B1 <= 100 and B2 <= 1000.
Needs a real MI355X:  python -m pytest tests -m gpu"""
import pytest

from prmers_amd import ecm
from test_ecm import m_run

pytestmark = pytest.mark.gpu

PLANS = [None, "m2=1024", "m2=2048", "m2=4096", "m2=8192"]
# (p, factor, sigma, b1, b2, outcome)
CURVES = [
    (301447, 142885879, 77, 100, 0, "stage1"),
    (301447, 142885879, 37, 50, 1000, "stage2"),
    (301447, 142885879, 6, 50, 1000, "nothing"),
    (300007, 43201009, 63, 100, 0, "stage1"),
    (300007, 43201009, 10, 50, 1000, "stage2"),
    (300007, 43201009, 6, 50, 1000, "nothing"),
]


def test_the_sigmas_do_what_the_model_says():
    for p, f, sigma, b1, b2, outcome in CURVES:
        assert pow(2, p, f) == 1
        g1, g2, _ = m_run(sigma, b1, b2, 30, f)
        assert (g1, g2) == {"stage1": (f, 1), "stage2": (1, f), "nothing": (1, 1)}[outcome]


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("p, f, sigma, b1, b2, outcome", CURVES)
def test_curves_on_every_row_kernel(p, f, sigma, b1, b2, outcome, plan):
    from prmers_amd import Engine
    D = 30 if b2 else None
    with Engine(p, ecm.registers_needed(30) if b2 else ecm.FIXED_REGISTERS, plan=plan) as e:
        res = ecm.run(e, p, b1, b2, sigma, D)
        ref = ecm.run(e, p, b1, b2, sigma, D, use_fused=False)
    assert res["fused"] is True and ref["fused"] is False
    assert (res["g1"], res["g2"]) == (ref["g1"], ref["g2"])
    assert ref["prepares"] - res["prepares"] == 2 * (ecm.stage1_exponent(b1).bit_length() - 1)
    if outcome == "stage1":
        assert res["g1"] % f == 0 and res["g2"] == 1
    elif outcome == "stage2":
        assert res["g1"] == 1 and res["g2"] % f == 0
    else:
        assert res["g1"] == 1 and res["g2"] == 1 and res["factors"] == []
    for g in res["factors"]:
        assert pow(2, p, g) == 1


def test_the_entry_point_draws_and_records_sigmas():
    res = ecm.ecm(301447, 100, 0, sigma=6, curves=2, seed=1)
    assert len(res["sigmas"]) == 2 and res["sigmas"][0] == 6 and res["sigmas"][1] >= ecm.SIGMA_MIN and res["sigma"] == res["sigmas"][-1]
    res = ecm.ecm(301447, 100, 0, sigma=77, curves=3)
    assert res["sigmas"] == [77] and res["factors"] and res["factors"][0] % 142885879 == 0
    assert ecm.main(["300007", "100", "--sigma", "63", "--plan", "m2=4096"]) == 0
