"""P-1 driver (prmers_amd/pm1.py) on the CPU oracle: stage 1, stage 2 with every wheel that fits, the k = 0 block, both gcd paths.
The expected factors were computed with Python integers; every factor reported must divide 2^p - 1 and the gcd it came from."""
import math

import pytest

import orc
from prmers_amd import pm1


def _run(p, b1, b2, D=None, **kw):
    regs = pm1.registers_needed(D) if D else pm1.FIXED_REGISTERS
    with orc.OracleEngine(p, regs) as eng:
        return pm1.run(eng, p, b1, b2, D, **kw)


def _check_factors(res, p):
    g = res["g1"] * res["g2"]
    for f in res["factors"]:
        assert f > 1 and pow(2, p, f) == 1 and g % f == 0, (p, f)
    assert math.gcd(res["g1"], res["g2"]) == 1 or res["g2"] == 1
    assert ((1 << p) - 1) % g == 0


@pytest.mark.parametrize("p, b1, b2, D, g1, stage2", [
    (1009, 20, 120, 30, 1, 3454817),
    (3001, 250, 600, 30, 3217073, 5339517247),
    (10007, 40, 300, 30, 240169 * 136255313, 60282169),
    (12007, 10, 40, 30, None, 18658879),
    (12007, 10, 40, 210, None, 18658879),    # 37 < D/2: reached through k = 0 only
])
def test_stage2_finds_the_known_factors(p, b1, b2, D, g1, stage2):
    res = _run(p, b1, b2, D)
    _check_factors(res, p)
    if g1 is not None:
        assert res["g1"] == g1
    assert (res["g1"] * res["g2"]) % stage2 == 0 and res["g1"] % stage2 != 0, res   # found, and by stage 2
    assert res["g2"] % stage2 == 0
    assert res["D"] == D and res["b2"] == b2 and res["fused"] is False and res["squarings"] > 0 and res["products"] > 0


def test_stage1_alone():
    res = _run(5003, 10, 0)
    _check_factors(res, 5003)
    assert res["g1"] == 10007 * 1050631 and res["g2"] == 1 and res["factors"] == [10007 * 1050631] and res["D"] is None


@pytest.mark.parametrize("D", [30, 210])
def test_nothing_found(D):
    res = _run(7001, 100, 1000, D)
    assert res["factors"] == [] and res["g1"] == 1 and res["g2"] == 1


def test_stage1_exponent_against_a_direct_product():
    for p, b1 in ((1009, 20), (127, 2), (521, 100), (9941, 1000)):
        e = 2 * p
        for q in range(2, b1 + 1):
            if all(q % d for d in range(2, math.isqrt(q) + 1)):
                e *= q ** int(math.floor(math.log(b1) / math.log(q) + 1e-12))
        assert pm1.stage1_exponent(p, b1) == e, (p, b1)
    assert pm1.stage1_exponent(7, 8) == 2 * 7 * 8 * 3 * 5 * 7 and pm1.stage1_exponent(7, 9) == 2 * 7 * 8 * 9 * 5 * 7


@pytest.mark.parametrize("b1, b2, D", [(20, 120, 30), (10, 40, 30), (10, 40, 210), (7, 3000, 210), (3, 5000, 2310), (100, 1000, 30), (2309, 7000, 2310)])
def test_every_prime_of_the_interval_is_covered(b1, b2, D):
    J = set(pm1.residues(D))
    pairs = pm1.stage2_pairs(b1, b2, D)
    covered = set()
    for k, js in pairs.items():
        assert set(js) <= J and k >= 0
        for j in js:
            covered |= {k * D - j, k * D + j}
    primes = [q for q in pm1.primes_upto(b2) if q > b1]
    assert primes == list(pm1.primes_between(b1, b2))
    for q in primes:
        assert q in covered or D % q == 0, q   # the primes that divide D go into the stage-1 exponent (run())
    assert len(J) == {30: 4, 210: 24, 2310: 240}[D] and pm1.registers_needed(D) == len(J) + pm1.FIXED_REGISTERS


def test_primes_that_divide_the_wheel_are_not_lost():
    """13007 = 2 * 929 * 7 + 1 divides M929.  With B1 = 4 the prime 7 lies in (B1, B2] but has no residue class mod 210: it must be
    found all the same (run() puts such primes into the exponent of stage 1); with D = 30 it is an ordinary stage-2 prime."""
    for D in (30, 210):
        res = _run(929, 4, 50, D)
        _check_factors(res, 929)
        assert (res["g1"] * res["g2"]) % 13007 == 0, (D, res)
    res = _run(127, 3, 50, 210)   # M127 is prime: nothing to find, k = 0 included
    assert res["factors"] == []


def test_default_wheel_and_register_budget():
    n = 2**23
    assert pm1.choose_D(n, 10**6, 3 * 10**7) == 2310
    assert pm1.choose_D(n, 10**6, 3 * 10**7, budget=4 << 30) == 210
    assert pm1.choose_D(n, 10**6, 3 * 10**7, budget=1 << 30) == 30
    assert pm1.choose_D(64, 20, 120) == 30 and pm1.choose_D(64, 20, 1000) == 210
    assert 2.0 < pm1.registers_needed(210) * 8 * n / 2**30 < 2.2 and 15 < pm1.registers_needed(2310) * 8 * n / 2**30 < 16
    with orc.OracleEngine(1009, 5) as eng, pytest.raises(ValueError):
        pm1.run(eng, 1009, 20, 120, 30)


def test_forced_composition_gives_the_same_factors():
    assert _run(1009, 20, 120, 30, use_mul_sum=False)["factors"] == _run(1009, 20, 120, 30)["factors"]


@pytest.mark.skipif(pm1.load_gmp() is None, reason="libgmp does not load")
def test_gmp_and_math_gcd_agree():
    import random
    rng = random.Random(5)
    for bits in (1, 64, 65, 4000, 100000):
        a, b = rng.getrandbits(bits), rng.getrandbits(bits) * 3 * 5 * 7
        a *= 105
        assert pm1.gcd_gmp(a, b) == math.gcd(a, b)
    assert pm1.gcd_gmp(0, 12) == 12 and pm1.gcd_gmp(12, 0) == 12
    assert _run(3001, 250, 600, 30, use_gmp=True)["factors"] == _run(3001, 250, 600, 30, use_gmp=False)["factors"]


def test_slow_gcd_is_refused_without_gmp():
    with pytest.raises(RuntimeError, match="libgmp"):
        pm1.big_gcd(1 << (pm1.SLOW_GCD_BITS + 1), 3, use_gmp=False)
    assert pm1.big_gcd(12, 18, use_gmp=False) == 6
