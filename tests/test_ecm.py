"""ECM driver (prmers_amd/ecm.py) on the CPU oracle against an integer model of the same algorithm (Suyama setup, Montgomery ladder,
stage 2 over the wheel D) written here with pow and % on 2^p - 1: the stage-1 point, g1 and g2 must be the model's.

The sigmas below were found by running this model modulo the known factor alone (cheap) over sigma = 6, 7, 8, ... and keeping the first
ones with the wanted outcome; the model on the full 2^p - 1 then gave the g1 and g2 listed."""
import math

import pytest

import orc
from prmers_amd import ecm, pm1


# ---- the integer model: points are (X, Z) tuples modulo n ----

def m_suyama(sigma, n):
    u = (sigma * sigma - 5) % n
    v = 4 * sigma % n
    u3, v3 = pow(u, 3, n), pow(v, 3, n)
    den = 16 * u3 * v % n
    g = math.gcd(den * v3 % n, n)
    if g != 1:
        return None, None, g
    inv = pow(den * v3 % n, -1, n)
    return u3 * den % n * inv % n, pow(v - u, 3, n) * (3 * u + v) % n * v3 % n * inv % n, 1


def m_dbl(pt, a24, n):
    ss, dd = pow(pt[0] + pt[1], 2, n), pow(pt[0] - pt[1], 2, n)
    t = (ss - dd) % n
    return ss * dd % n, t * ((dd + a24 * t) % n) % n


def m_add(p1, p2, diff, n):
    a = (p1[0] - p1[1]) * (p2[0] + p2[1]) % n
    b = (p1[0] + p1[1]) * (p2[0] - p2[1]) % n
    return diff[1] * pow(a + b, 2, n) % n, diff[0] * pow(a - b, 2, n) % n


def m_ladder(m, pt, a24, n):
    """(m pt, (m + 1) pt), m >= 1"""
    r0, r1 = pt, m_dbl(pt, a24, n)
    for i in range(m.bit_length() - 2, -1, -1):
        if (m >> i) & 1:
            r0, r1 = m_add(r0, r1, pt, n), m_dbl(r1, a24, n)
        else:
            r0, r1 = m_dbl(r0, a24, n), m_add(r0, r1, pt, n)
    return r0, r1


def m_exponent(b1, b2, D):
    e = 1
    for q in range(2, b1 + 1):
        if all(q % d for d in range(2, math.isqrt(q) + 1)):
            qq = q
            while qq * q <= b1:
                qq *= q
            e *= qq
    if b2 > b1:
        for q in (2, 3, 5, 7, 11):
            if D % q == 0 and b1 < q <= b2:
                e *= q
    return e


def m_stage2(Q, a24, b1, b2, D, n):
    pairs = pm1.stage2_pairs(b1, b2, D)
    if not pairs:
        return 1
    J = pm1.residues(D)
    two = m_dbl(Q, a24, n)
    table, prev, cur = {}, Q, Q
    for j in range(1, J[-1] + 1, 2):
        if j in J:
            table[j] = cur
        prev, cur = cur, m_add(cur, two, prev, n)
    DQ = m_ladder(D, Q, a24, n)[0]
    k0, k1 = min(pairs), max(pairs)
    cur, nxt = ((1, 0), DQ) if k0 == 0 else m_ladder(k0, DQ, a24, n)
    A = 1
    for k in range(k0, k1 + 1):
        for j in pairs.get(k, ()):
            A = A * ((cur[0] * table[j][1] - cur[1] * table[j][0]) % n) % n
        cur, nxt = nxt, (m_dbl(DQ, a24, n) if k == 0 else m_add(nxt, DQ, cur, n))
    return A


def m_run(sigma, b1, b2, D, n):
    """(g1, g2, Q) of the model modulo n"""
    x0, a24, g = m_suyama(sigma, n)
    if g != 1:
        return g, 1, None
    Q = m_ladder(m_exponent(b1, b2, D), (x0, 1), a24, n)[0]
    g1 = math.gcd(Q[1], n)
    g2 = 1
    if b2 > b1 and g1 != n:
        g = math.gcd(m_stage2(Q, a24, b1, b2, D, n), n)
        g2 = g // math.gcd(g, g1)
    return g1, g2, Q


# ---- the driver on the oracle ----

def _run(p, b1, b2, sigma, D=None, **kw):
    regs = ecm.registers_needed(D) if D else ecm.FIXED_REGISTERS
    with orc.OracleEngine(p, regs) as eng:
        res = ecm.run(eng, p, b1, b2, sigma, D, **kw)
        return res, (eng.get_int(ecm.R_XQ), eng.get_int(ecm.R_ZQ))


# (p, sigma, b1, b2, D, g1, g2): first sigma >= 6 with the outcome modulo the factor named, searched with m_run(sigma, b1, b2, D, factor)
CASES = [
    (1009, 69, 50, 0, None, 3454817, 1),            # 3454817 in stage 1
    (1009, 12, 20, 104, 210, 1, 3454817),           # stage 2 only, and every prime of (20, 104] is below D/2: the k = 0 block alone
    (3001, 36, 100, 0, None, 3217073, 1),           # 3217073 in stage 1
    (3001, 6, 30, 300, 30, 1, 3217073),             # stage 2 only: B1 = 30 alone gives g1 = 1
    (10007, 61, 30, 0, None, 240169, 1),
    (10007, 10, 20, 500, 210, 1, 240169),           # k = 0, 1, 2 with D = 210
    (12007, 10, 50, 1000, 30, 1, 18658879),
    (1009, 7, 50, 300, 30, 1, 1),                   # curves that find nothing
    (3001, 8, 30, 300, 210, 1, 1),
]


def test_the_known_factors_are_factors():
    for p, fs in ((1009, [3454817]), (3001, [3217073, 5339517247]), (10007, [240169, 136255313, 60282169]), (12007, [18658879])):
        for f in fs:
            assert pow(2, p, f) == 1


@pytest.mark.parametrize("p, sigma, b1, b2, D, g1, g2", CASES)
def test_point_and_gcds_match_the_integer_model(p, sigma, b1, b2, D, g1, g2):
    mp = (1 << p) - 1
    res, (xe, ze) = _run(p, b1, b2, sigma, D)
    mg1, mg2, (xm, zm) = m_run(sigma, b1, b2, D or 30, mp)
    assert (xe * zm - xm * ze) % mp == 0                       # the same point, projectively
    assert (res["g1"], res["g2"]) == (mg1, mg2) == (g1, g2)
    assert res["factors"] == [f for f in (g1, g2) if f > 1]
    for f in res["factors"]:
        assert pow(2, p, f) == 1
    assert res["sigma"] == sigma and res["b2"] == b2 and res["D"] == D and res["fused"] is False
    steps = m_exponent(b1, b2, D or 30).bit_length() - 1
    assert res["squarings"] >= 4 * steps and res["products"] >= 6 * steps and res["prepares"] >= 4 * steps


def test_stage2_only_cases_need_stage2():
    for p, sigma, b1, b2, D, g1, g2 in CASES:
        if g2 > 1:
            assert m_run(sigma, b1, 0, 30, (1 << p) - 1)[0] == 1 and _run(p, b1, 0, sigma)[0]["factors"] == []
    # the k = 0 case: every pair of its interval has k = 0
    assert set(pm1.stage2_pairs(20, 104, 210)) == {0}


@pytest.mark.parametrize("b1, b2, D", [(20, 120, 30), (10, 40, 30), (10, 40, 210), (7, 3000, 210), (3, 5000, 2310), (100, 1000, 30), (2309, 7000, 2310)])
def test_every_prime_of_the_interval_is_covered(b1, b2, D):
    """the (b1, b2, D) triples of test_pm1.py: ECM's stage 2 walks the same pairs, and its table has both coordinates of every j"""
    J = set(pm1.residues(D))
    covered = set()
    for k, js in pm1.stage2_pairs(b1, b2, D).items():
        assert set(js) <= J and k >= 0
        for j in js:
            covered |= {k * D - j, k * D + j}
    e = m_exponent(b1, b2, D)
    assert ecm.stage1_exponent(b1) * math.prod(q for q in (2, 3, 5, 7, 11) if D % q == 0 and b1 < q <= b2) == e
    for q in pm1.primes_upto(b2):
        if q > b1:
            assert q in covered or (D % q == 0 and e % q == 0), q
    assert ecm.registers_needed(D) == 2 * len(J) + ecm.FIXED_REGISTERS


class CountingEngine(orc.OracleEngine):
    """the oracle with square_mul_prepare as the composition it stands for, counting calls"""

    def __init__(self, p, regs):
        orc.OracleEngine.__init__(self, p, regs)
        self.calls = {"set_multiplicand": 0, "square_mul": 0, "square_mul_prepare": 0, "mul": 0}

    def set_multiplicand(self, dst, src):
        self.calls["set_multiplicand"] += 1
        orc.OracleEngine.set_multiplicand(self, dst, src)

    def square_mul(self, src, a=1):
        self.calls["square_mul"] += 1
        orc.OracleEngine.square_mul(self, src, a)

    def mul(self, dst, src, a=1):
        self.calls["mul"] += 1
        orc.OracleEngine.mul(self, dst, src, a)

    def square_mul_prepare(self, src, img, a=1):
        assert src != img
        self.calls["square_mul_prepare"] += 1
        self.o.set_multiplicand(img, src)
        self.o.square_mul(src, a)

    def square_mul_prepare_is_fused(self):
        return True


def test_fused_and_composed_runs_agree_and_the_fused_one_saves_two_prepares_per_bit():
    p, sigma, b1, b2, D = 3001, 6, 30, 300, 30
    out = {}
    for use in (True, False):
        with CountingEngine(p, ecm.registers_needed(D)) as eng:
            out[use] = (ecm.run(eng, p, b1, b2, sigma, D, use_fused=use), dict(eng.calls))
    (rf, cf), (rc, cc) = out[True], out[False]
    assert rf["factors"] == rc["factors"] == [3217073] and (rf["g1"], rf["g2"]) == (rc["g1"], rc["g2"])
    assert rf["fused"] is True and rc["fused"] is False
    bits = m_exponent(b1, b2, D).bit_length() - 1               # ladder steps of stage 1
    assert cf["square_mul_prepare"] == 2 * bits and cc["square_mul_prepare"] == 0
    assert cc["set_multiplicand"] - cf["set_multiplicand"] == 2 * bits
    assert cf["square_mul"] + cf["square_mul_prepare"] == cc["square_mul"] and cf["mul"] == cc["mul"]
    assert rc["prepares"] - rf["prepares"] == 2 * bits and rf["squarings"] == rc["squarings"] and rf["products"] == rc["products"]
    assert rc["prepares"] == cc["set_multiplicand"]


def test_a_failing_inversion_is_reported_as_a_factor():
    # sigma = the factor itself: v = 4 sigma = 0 modulo it, so the denominator 16 u^3 v^4 is not invertible modulo 2^p - 1
    p, f = 1009, 3454817
    for use_gmp in (None, False):
        with orc.OracleEngine(p, ecm.FIXED_REGISTERS) as eng:
            res = ecm.run(eng, p, 50, 0, f, use_gmp=use_gmp)
        assert res["g1"] % f == 0 and f in [math.gcd(x, f) for x in res["factors"]] and res["squarings"] == 0
    assert m_suyama(f, (1 << p) - 1)[2] == res["g1"]
    x0, a24, g = ecm.suyama(69, (1 << p) - 1)
    assert g == 1 and (x0, a24) == m_suyama(69, (1 << p) - 1)[:2]


def test_slow_inversion_is_refused_without_gmp():
    n = (1 << (pm1.SLOW_GCD_BITS + 1)) - 1
    with pytest.raises(RuntimeError, match="libgmp"):
        ecm.mod_inverse(3, n, use_gmp=False)
    assert ecm.mod_inverse(3, 7, use_gmp=False) == 5 and ecm.mod_inverse(3, 9, use_gmp=False) == 0


@pytest.mark.skipif(pm1.load_gmp() is None, reason="libgmp does not load")
def test_gmp_and_python_inverses_agree():
    import random
    rng = random.Random(7)
    for bits in (8, 64, 65, 4000):
        n = rng.getrandbits(bits) | 1
        x = rng.getrandbits(bits + 3)
        assert ecm.mod_inverse(x, n, use_gmp=True) == ecm.mod_inverse(x, n, use_gmp=False)
    assert ecm.mod_inverse(6, 9, use_gmp=True) == 0


def test_arguments():
    with orc.OracleEngine(1009, 5) as eng, pytest.raises(ValueError):
        ecm.run(eng, 1009, 20, 0, 7)                       # too few registers
    with orc.OracleEngine(1009, ecm.FIXED_REGISTERS) as eng:
        with pytest.raises(ValueError):
            ecm.run(eng, 1009, 20, 0, 5)                   # sigma below the range
        with pytest.raises(ValueError):
            ecm.run(eng, 1009, 20, 120, 7, 30)             # stage 2 needs the table's registers
    assert ecm.choose_D(64, 20, 120) == 30 and ecm.choose_D(64, 20, 1000) == 210
