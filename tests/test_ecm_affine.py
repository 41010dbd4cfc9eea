"""ECM's affine stage 2 (prmers_amd/ecm.py, stage2="affine") on the CPU oracle against an integer model of the same algorithm written
here on top of the model of tests/test_ecm.py: points normalised in blocks by Montgomery's trick, the inverse 1 for a lane whose block
product is not invertible, the host's Z product zacc, and no pairs walked for k = 0.  (g1, g2) must be the model's and, on the stage-2
cases of tests/test_ecm.py, the projective values listed there; the accumulator register must be the model's prod (x_k - x_j)."""
import json
import math

import pytest

import orc
from prmers_amd import ecm, ecm_edwards, pm1
from test_ecm import CASES, m_add, m_dbl, m_exponent, m_ladder, m_suyama
from test_lanes_host import LaneOracles

STAGE2_CASES = [c for c in CASES if c[3] > c[2]]


# ---- the integer model ----

def _mod(x, n):
    """x % n; for n = 2^p - 1 of thousands of bits by shifts (a division of two 200000-bit numbers takes longer than their product)"""
    p = n.bit_length()
    if p < 4096 or n & (n + 1) or x < 0:
        return x % n
    while x >> p:
        x = (x & n) + (x >> p)
    return 0 if x == n else x


def f_dbl(pt, a24, n):
    """m_dbl, m_add and m_ladder of tests/test_ecm.py through _mod (test_the_fast_point_arithmetic_is_the_model_s)"""
    s, d = pt[0] + pt[1], pt[0] + n - pt[1]
    ss, dd = _mod(s * s, n), _mod(d * d, n)
    t = ss + n - dd
    return _mod(ss * dd, n), _mod(t * _mod(dd + a24 * t, n), n)


def f_add(p1, p2, diff, n):
    a = _mod((p1[0] + n - p1[1]) * (p2[0] + p2[1]), n)
    b = _mod((p1[0] + p1[1]) * (p2[0] + n - p2[1]), n)
    s, d = a + b, a + n - b
    return _mod(diff[1] * _mod(s * s, n), n), _mod(diff[0] * _mod(d * d, n), n)


def f_ladder(m, pt, a24, n):
    r0, r1 = pt, f_dbl(pt, a24, n)
    for i in range(m.bit_length() - 2, -1, -1):
        if (m >> i) & 1:
            r0, r1 = f_add(r0, r1, pt, n), f_dbl(r1, a24, n)
        else:
            r0, r1 = f_dbl(r0, a24, n), f_add(r0, r1, pt, n)
    return r0, r1


def m_inverse(x, n):
    """x^-1 mod n for a unit x: pow below 2^16 bits; above, where pow takes seconds, libgmp's when it loads"""
    if n.bit_length() > 1 << 16 and pm1.load_gmp() is not None:
        u = ecm.mod_inverse(x, n, use_gmp=True)
        assert u * x % n == 1
        return u
    return pow(x, -1, n)


def m_normalise(block, zacc, negate, n):
    """the x = X / Z of a block of points (X, Z) (their negatives when negate) by one inversion of the block's Z product, which is
    multiplied into zacc[0]; a product without an inverse is replaced by the inverse 1.  -> (xs, the inversion succeeded)"""
    c = [block[0][1]]
    for X, Z in block[1:]:
        c.append(_mod(c[-1] * Z, n))
    zacc[0] = _mod(zacc[0] * c[-1], n)
    ok = math.gcd(c[-1], n) == 1
    u = m_inverse(c[-1], n) if ok else 1
    if negate:
        u = n - u
    xs = [0] * len(block)
    for i in range(len(block) - 1, 0, -1):
        xs[i] = _mod(block[i][0] * _mod(u * c[i - 1], n), n)
        u = _mod(u * block[i][1], n)
    xs[0] = _mod(block[0][0] * u, n)
    return xs, ok


def m_stage2_affine(Q, a24, b1, b2, D, n, giants_per_block=None):
    """(A, zacc, every inversion succeeded, points normalised, blocks) of the affine stage 2 modulo n"""
    pairs = pm1.stage2_pairs(b1, b2, D)
    if not pairs:
        return 1, 1, True, 0, 0
    J = pm1.residues(D)
    two = f_dbl(Q, a24, n)
    table, prev, cur = {}, Q, Q
    for j in range(1, J[-1] + 1, 2):
        if j in J:
            table[j] = cur
        prev, cur = cur, f_add(cur, two, prev, n)
    zacc = [1]
    neg, good = m_normalise([table[j] for j in J], zacc, True, n)
    neg = dict(zip(J, neg))
    count, blocks = len(J), 1
    m = giants_per_block or max(1, 2 * len(J) // 3)
    k, k1 = max(min(pairs), 1), max(pairs)
    A = 1
    if k <= k1:
        DQ = f_ladder(D, Q, a24, n)[0]
        cur, nxt = f_ladder(k, DQ, a24, n)
    todo = []
    while k <= k1:
        if pairs.get(k):
            todo.append((k, cur))
        cur, nxt = nxt, (f_add(nxt, DQ, cur, n) if k < k1 else None)
        k += 1
    for i in range(0, len(todo), m):
        block = todo[i:i + m]
        xs, ok = m_normalise([pt for _, pt in block], zacc, False, n)
        good, count, blocks = good and ok, count + len(block), blocks + 1
        for (kk, _), x in zip(block, xs):
            for j in pairs[kk]:
                A = _mod(A * (x + neg[j]), n)
    return A, zacc[0], good, count, blocks


def m_run_affine(sigma, b1, b2, D, n, setup=None):
    """(g1, g2, A, every inversion succeeded, points normalised, blocks) of the model modulo n; setup: (x0, a24, 1) where m_suyama's pow
    would take seconds"""
    x0, a24, g = setup or m_suyama(sigma, n)
    assert g == 1
    Q = f_ladder(m_exponent(b1, b2, D), (x0, 1), a24, n)[0]
    g1 = math.gcd(Q[1], n)
    A, zacc, good, count, blocks = m_stage2_affine(Q, a24, b1, b2, D, n)
    g = math.gcd(_mod(A * zacc, n), n)
    return g1, g // math.gcd(g, g1), A, good, count, blocks


@pytest.fixture(scope="module")
def models():
    return {c[:5]: m_run_affine(c[1], c[2], c[3], c[4], (1 << c[0]) - 1) for c in STAGE2_CASES}


def test_the_fast_point_arithmetic_is_the_model_s():
    for n in ((1 << 1009) - 1, (1 << 4423) - 1, 3454817):
        x0, a24, _ = m_suyama(9, n)
        P = (x0, 1)
        assert f_dbl(P, a24, n) == m_dbl(P, a24, n)
        for m in (1, 2, 5, 30, 211):
            assert f_ladder(m, P, a24, n) == m_ladder(m, P, a24, n)
        a, b = m_ladder(6, P, a24, n)
        assert f_add(a, b, P, n) == m_add(a, b, P, n)
    n = (1 << 4423) - 1
    assert [_mod(x, n) for x in (n, 2 * n, n * n, n + 5, -3, 7 << 4423)] == [0, 0, 0, 5, n - 3, 7]


def test_inverses_of_many_values_with_and_without_one_that_has_none(monkeypatch):
    import random
    rng = random.Random(3)
    n = (1 << 1009) - 1
    xs = [rng.getrandbits(1009) for _ in range(7)] + [1, n - 1, n + 2]
    calls = []
    one = ecm.mod_inverse
    monkeypatch.setattr(ecm, "mod_inverse", lambda *a: calls.append(1) or one(*a))
    for use_gmp in (None, False):
        assert ecm.mod_inverses(xs, n, use_gmp) == [pow(x, -1, n) for x in xs]
    assert len(calls) == 2                                     # one inversion for all of them
    bad = xs[:3] + [3454817 * 5, 0, n] + xs[3:]                # 3454817 divides 2^1009 - 1
    assert ecm.mod_inverses(bad, n) == [0 if i in (3, 4, 5) else pow(x, -1, n) for i, x in enumerate(bad)]
    assert ecm.mod_inverses([], n) == [] and ecm.mod_inverses([5], n) == [pow(5, -1, n)] and ecm.mod_inverses([0, 0], n) == [0, 0]
    monkeypatch.setattr(ecm, "SHARED_INVERSE_BITS", 64)        # above the bound: one by one
    del calls[:]
    assert ecm.mod_inverses(xs, n) == [pow(x, -1, n) for x in xs] and len(calls) == len(xs)


def test_the_model_normalises():
    n = (1 << 127) - 1
    pts = [(3 * i + 5, 7 * i + 2) for i in range(1, 8)]
    for negate in (False, True):
        zacc = [1]
        xs, ok = m_normalise(pts, zacc, negate, n)
        assert ok and zacc[0] == math.prod(z for _, z in pts) % n
        assert xs == [(-1 if negate else 1) * x * pow(z, -1, n) % n for x, z in pts]
    n = 15                                         # a product that shares 3 with n: the inverse 1, and zacc carries the 3
    zacc = [1]
    assert m_normalise([(2, 7), (4, 3)], zacc, False, n) == ([2 * 3 % n, 4 * 7 % n], False) and math.gcd(zacc[0], n) == 3


# ---- the driver on the oracle ----

@pytest.mark.parametrize("p, sigma, b1, b2, D, g1, g2", STAGE2_CASES)
def test_gcds_and_accumulator_match_the_model_and_the_projective_values(p, sigma, b1, b2, D, g1, g2, models):
    mp = (1 << p) - 1
    mg1, mg2, A, good, count, blocks = models[(p, sigma, b1, b2, D)]
    with orc.OracleEngine(p, ecm.registers_needed(D, "affine")) as eng:
        res = ecm.run(eng, p, b1, b2, sigma, D, stage2="affine")
        acc = eng.get_int(ecm.R_A)
    assert (res["g1"], res["g2"]) == (mg1, mg2) == (g1, g2)
    assert res["factors"] == [f for f in (g1, g2) if f > 1]
    assert (res["stage2"], res["fused_sum"], res["normalised"]) == ("affine", False, count)
    # where every inversion succeeds the accumulator is prod (x_k - x_j), exactly; in the k = 0 case the baby block's product shares the
    # factor with Mp (that is how it is found), the inverse 1 stands in, and the accumulator is still the model's
    assert acc == A and good == ((p, sigma) != (1009, 12))
    with orc.OracleEngine(p, ecm.registers_needed(D)) as eng:
        ref = ecm.run(eng, p, b1, b2, sigma, D)
    assert (ref["g1"], ref["g2"]) == (g1, g2)
    assert set(res) - set(ref) == {"stage2", "fused_sum", "normalised"} and set(ref) <= set(res)   # a projective result has no new key


def test_the_k0_case_is_found_through_the_z_product_alone(models):
    p, sigma, b1, b2, D = 1009, 12, 20, 104, 210
    assert set(pm1.stage2_pairs(b1, b2, D)) == {0}
    g1, g2, A, good, count, blocks = models[(p, sigma, b1, b2, D)]
    assert (g1, g2, A, blocks) == (1, 3454817, 1, 1) and count == len(pm1.residues(D))


def test_the_accumulator_does_not_depend_on_the_block_size():
    p, sigma, b1, b2, D = 10007, 10, 20, 500, 30
    n = (1 << p) - 1
    x0, a24, _ = m_suyama(sigma, n)
    Q = f_ladder(m_exponent(b1, b2, D), (x0, 1), a24, n)[0]
    runs = [m_stage2_affine(Q, a24, b1, b2, D, n, m) for m in (1, 2, 3, 100)]
    assert len({r[0] for r in runs}) == 1 and all(r[2] for r in runs) and len({r[4] for r in runs}) == 4
    want = runs[1]                                 # D = 30 has |J| = 4: two giant points a block
    with orc.OracleEngine(p, ecm.registers_needed(D, "affine")) as eng:
        res = ecm.run(eng, p, b1, b2, sigma, D, stage2="affine")
        assert eng.get_int(ecm.R_A) == want[0] and res["normalised"] == want[3]
    # more registers than the mode needs change nothing: the blocks come from the table's registers
    with orc.OracleEngine(p, ecm.registers_needed(D, "affine") + 7) as eng:
        ecm.run(eng, p, b1, b2, sigma, D, stage2="affine")
        assert eng.get_int(ecm.R_A) == want[0]


def test_run_lanes_with_a_lane_that_finds_the_factor_next_to_lanes_that_find_nothing(models):
    p, b1, b2, D, sigmas = 3001, 30, 300, 30, [8, 6, 7]
    mp = (1 << p) - 1
    want = [m_run_affine(s, b1, b2, D, mp) for s in sigmas]
    with LaneOracles(p, ecm.registers_needed(D, "affine"), lanes=len(sigmas)) as eng:
        out = ecm.run_lanes(eng, p, b1, b2, sigmas, D, stage2="affine")
        acc = [eng.get_int(ecm.R_A, lane=l) for l in range(len(sigmas))]
    assert [(r["g1"], r["g2"]) for r in out] == [w[:2] for w in want]
    assert out[0]["factors"] == [] and out[1]["factors"] == [3217073]                    # sigma 6 finds it, sigma 8 does not (tests/test_ecm.py)
    assert all(w[3] for w in want) and acc == [w[2] for w in want]
    assert all(r["stage2"] == "affine" and r["normalised"] == want[0][4] for r in out)
    # the k = 0 case in a lane: found through the Z product while the other lane finds nothing
    p, b1, b2, D, sigmas = 1009, 20, 104, 210, [7, 12]
    with LaneOracles(p, ecm.registers_needed(D, "affine"), lanes=2) as eng:
        out = ecm.run_lanes(eng, p, b1, b2, sigmas, D, stage2="affine")
    assert [(r["g1"], r["g2"]) for r in out] == [m_run_affine(s, b1, b2, D, (1 << p) - 1)[:2] for s in sigmas]
    assert out[1]["g2"] == 3454817 and out[0]["factors"] == []


def test_the_edwards_driver_takes_the_mode(models):
    p, sigma, b1, b2, D = 3001, 6, 30, 300, 30
    with orc.OracleEngine(p, ecm_edwards.registers_needed(D, "affine")) as eng:
        res = ecm_edwards.run(eng, p, b1, b2, sigma, D, stage2="affine")
    with orc.OracleEngine(p, ecm_edwards.registers_needed(D)) as eng:
        ref = ecm_edwards.run(eng, p, b1, b2, sigma, D)
    assert (res["g1"], res["g2"]) == (ref["g1"], ref["g2"]) == (1, 3217073)
    assert res["stage2"] == "affine" and res["curve"] == "edwards" and "stage2" not in ref
    assert ecm_edwards.registers_needed(D, "affine") == ecm.registers_needed(D, "affine") and ecm_edwards.registers_needed() == ecm.FIXED_REGISTERS


# ---- counts ----

class Counting(orc.OracleEngine):
    """the oracle with a mul_sum (the composition it stands for), logging the calls that cost sweeps and the reads and writes"""

    def __init__(self, p, regs):
        orc.OracleEngine.__init__(self, p, regs)
        self.log = []

    def set_multiplicand(self, dst, src):
        self.log.append("prep"); orc.OracleEngine.set_multiplicand(self, dst, src)

    def square_mul(self, src, a=1):
        self.log.append("sq"); orc.OracleEngine.square_mul(self, src, a)

    def mul(self, dst, src, a=1):
        self.log.append("mul"); orc.OracleEngine.mul(self, dst, src, a)

    def mul_sum(self, dst, a, b, tmp):
        assert len({dst, a, b, tmp}) == 4
        self.log.append("mul_sum")
        self.o.copy(tmp, dst); self.o.mul(dst, a, 1); self.o.mul(tmp, b, 1); self.o.add(dst, tmp)

    def mul_sum_is_fused(self):
        return True

    def get_int(self, src):
        self.log.append("get"); return orc.OracleEngine.get_int(self, src)

    def set_int(self, dst, v):
        self.log.append("put"); orc.OracleEngine.set_int(self, dst, v)


class CountingLanes(LaneOracles):
    def __init__(self, p, regs, lanes):
        LaneOracles.__init__(self, p, regs, lanes=lanes)
        self.log = []

    def get_ints(self, src):
        self.log.append("get"); return [o.get_int(src) for o in self.o]

    def set_ints(self, dst, values):
        self.log.append("put")
        for o, v in zip(self.o, values):
            o.set_int(dst, v)


@pytest.mark.parametrize("p, sigma, b1, b2, D", [(10007, 10, 20, 500, 210), (10007, 10, 20, 500, 30), (3001, 6, 30, 300, 30)])
def test_one_mul_sum_per_pair_and_the_budget_of_a_normalised_point(p, sigma, b1, b2, D):
    pairs = pm1.stage2_pairs(b1, b2, D)
    npairs = sum(len(js) for k, js in pairs.items() if k > 0)
    with Counting(p, ecm.registers_needed(D, "affine")) as eng:
        res = ecm.run(eng, p, b1, b2, sigma, D, stage2="affine")
        log = eng.log
    assert res["fused_sum"] is True and log.count("mul_sum") == npairs > 0
    # a run of pairs is mul_sum calls and nothing else: between the first and the last mul_sum of a block no other product or prepare
    text = "".join({"mul_sum": "S", "mul": "m", "prep": "p", "sq": "q", "get": "G", "put": "P"}[c] for c in log)
    s2 = text[text.index("G", text.index("G") + 1):]          # from the second read on: stage 2's first block (the first read is stage 1's Z)
    blocks = s2.count("G") - 1                                # the last read is the accumulator
    giants = sum(1 for k, js in pairs.items() if k > 0 and js)
    m = max(1, 2 * len(pm1.residues(D)) // 3)
    assert blocks == 1 + -(-giants // m) and s2.count("P") == blocks
    assert res["normalised"] == len(pm1.residues(D)) + giants
    # every block: ... G P then the back pass, then (giant blocks) the pairs as one run of S
    segs = s2.split("G")[1:-1]                                 # after each block's read, up to the next block's read
    assert len(segs) == blocks and all(seg.startswith("P") for seg in segs)
    for i, seg in enumerate(segs[1:], 1):
        run = seg[seg.index("S"):seg.rindex("S") + 1]
        assert set(run) == {"S"}
    # the budget: products and prepares of the normalisations = all of stage 2's minus the point arithmetic's, counted here: an addition
    # is 4 products, 4 prepares and 2 squarings, a doubling 3, 2 and 2; a small ladder is a doubling, then an addition and a doubling a bit
    adds = (pm1.residues(D)[-1] - 1) // 2                      # baby additions
    k0, k1 = max(min(pairs), 1), max(pairs)
    n_add = adds + (D.bit_length() - 1) + (k0.bit_length() - 1) + max(0, k1 - k0 - 1)
    n_dbl = 1 + D.bit_length() + k0.bit_length()
    stage1 = text[:text.index("G")]
    rest = text[text.index("G"):]
    norm_mul = rest.count("m") - 4 * n_add - 3 * n_dbl
    norm_prep = rest.count("p") - 4 * n_add - 2 * n_dbl
    assert rest.count("q") == 2 * n_add + 2 * n_dbl and stage1.count("S") == 0
    assert 0 < norm_mul <= 4 * res["normalised"] and 0 < norm_prep <= 4 * res["normalised"]
    assert (norm_mul, norm_prep) == (4 * res["normalised"] - 3 * blocks, 4 * res["normalised"] - 2 * blocks)


def test_one_read_and_one_write_per_block_on_lanes_and_the_fallback_loop():
    p, b1, b2, D, sigmas = 3001, 30, 300, 30, [6, 8]
    with CountingLanes(p, ecm.registers_needed(D, "affine"), 2) as eng:
        out = ecm.run_lanes(eng, p, b1, b2, sigmas, D, stage2="affine")
        log = eng.log
    with LaneOracles(p, ecm.registers_needed(D, "affine"), lanes=2) as eng:      # no set_ints / get_ints: the per-lane loops
        ref = ecm.run_lanes(eng, p, b1, b2, sigmas, D, stage2="affine")
    assert [(r["g1"], r["g2"]) for r in out] == [(r["g1"], r["g2"]) for r in ref] == [(1, 3217073), (1, 1)]
    giants = sum(1 for k, js in pm1.stage2_pairs(b1, b2, D).items() if k > 0 and js)
    blocks = 1 + -(-giants // 2)
    assert log.count("get") == blocks + 2 and log.count("put") == blocks + 3         # + Z and A; + a24, x0 and the start point


# ---- arguments ----

def test_registers_needed_for_both_modes():
    for D in pm1.D_CHOICES:
        J = len(pm1.residues(D))
        assert ecm.registers_needed(D) == ecm.registers_needed(D, "projective") == 2 * J + ecm.FIXED_REGISTERS
        assert ecm.registers_needed(D, "affine") == ecm.registers_needed(D, stage2="affine") == 3 * J + ecm.FIXED_REGISTERS
    with pytest.raises(ValueError):
        ecm.registers_needed(30, "jacobian")
    with pytest.raises(ValueError):
        ecm.registers_needed(31, "affine")
    assert ecm.choose_D(64, 20, 1000) == ecm.choose_D(64, 20, 1000, stage2="affine") == 210
    # a budget between the two register files: the affine mode steps down
    n = 1 << 20
    budget = (ecm.registers_needed(210) + 1) * 8 * n
    assert ecm.choose_D(n, 20, 1000, budget) == 210 and ecm.choose_D(n, 20, 1000, budget, "affine") == 30


def test_too_few_registers_and_unknown_modes_are_refused():
    p = 1009
    with orc.OracleEngine(p, ecm.registers_needed(30)) as eng:
        with pytest.raises(ValueError, match="registers"):
            ecm.run(eng, p, 20, 120, 7, 30, stage2="affine")          # the projective file is too small
        with pytest.raises(ValueError, match="stage2"):
            ecm.run(eng, p, 20, 120, 7, 30, stage2="jacobian")
        assert ecm.run(eng, p, 20, 120, 7, None, stage2="projective")["D"] == 30
    with orc.OracleEngine(p, ecm.registers_needed(210)) as eng:          # D is chosen for the mode: 210 does not fit, 30 does
        assert ecm.run(eng, p, 20, 1000, 7, None, stage2="affine")["D"] == 30
    with orc.OracleEngine(p, ecm.FIXED_REGISTERS) as eng:                # no stage 2: the mode asks for nothing and adds nothing
        assert "stage2" not in ecm.run(eng, p, 20, 0, 7, stage2="affine")
    with pytest.raises(ValueError, match="stage2"):
        ecm.ecm(p, 20, 120, stage2="jacobian")


def test_the_cli_and_the_entry_point_pass_the_mode(monkeypatch, capsys):
    from prmers_amd import engine as E
    seen = {}

    def fake(*a, **kw):
        seen["kw"] = kw
        return {"factors": []}
    monkeypatch.setattr(ecm, "ecm", fake)
    assert ecm.main(["1009", "20", "104", "--stage2", "affine"]) == 1 and seen["kw"] == {"stage2": "affine"}
    assert ecm.main(["1009", "20", "104"]) == 1 and seen["kw"] == {}
    assert ecm.main(["1009", "20", "104", "--stage2", "projective"]) == 1 and seen["kw"] == {}
    with pytest.raises(SystemExit):
        ecm.main(["1009", "20", "104", "--stage2", "jacobian"])
    capsys.readouterr()
    monkeypatch.undo()
    # the entry point sizes the engine for the mode and hands it to run / run_lanes
    monkeypatch.setattr(E, "Engine", LaneOracles)
    LaneOracles.made = []
    res = ecm.ecm(1009, 20, 104, sigma=12, D=210, stage2="affine")
    assert LaneOracles.made[-1].reg_count == ecm.registers_needed(210, "affine")
    assert res["factors"] == [3454817] and res["stage2"] == "affine" and json.dumps(res)
    res = ecm.ecm(1009, 20, 104, sigma=12, D=210, lanes=2, seed=5, stage2="affine", curve="edwards")
    assert LaneOracles.made[-1].reg_count == ecm.registers_needed(210, "affine") and LaneOracles.made[-1].lanes == 2
    assert 3454817 in res["factors"] and res["batch"][0]["stage2"] == "affine" and res["batch"][0]["curve"] == "edwards"
    res = ecm.ecm(1009, 20, 104, sigma=12, D=210)
    assert LaneOracles.made[-1].reg_count == ecm.registers_needed(210) and "stage2" not in res and res["factors"] == [3454817]
