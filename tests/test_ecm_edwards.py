"""ECM on twisted Edwards curves (prmers_amd/ecm_edwards.py) on the CPU oracle against an integer model of the same formulas written here
with pow and % on 2^p - 1: the curve identities, the stage-1 point coordinate by coordinate, the Montgomery curve of the same sigma, the
factors test_ecm.py finds, the on-curve check with injected faults and roll-back, and the engine calls per doubling, addition and check
that DESIGN.md 7e counts."""
import math

import pytest

import orc
from prmers_amd import ecm
from prmers_amd import ecm_edwards as ed
from prmers_amd import engine as E
from test_batch_host import Recording
from test_ecm import CASES as MONTGOMERY_CASES
from test_lanes_host import LaneOracles


# ---- the integer model: points are (X, Y, Z, T) tuples modulo n ----

def m_curve(sigma, n):
    """(a, d, X0, Y0) by the formulas of the issue, each quotient by its own inversion"""
    u, v = (sigma * sigma - 5) % n, 4 * sigma % n
    def inv(x): return pow(x % n, -1, n)
    ap2 = pow(v - u, 3, n) * (3 * u + v) * inv(4 * u**3 * v) % n
    B = u * inv(v) % n
    a, d = ap2 * inv(B) % n, (ap2 - 4) * inv(B) % n
    x0 = u * u * v * inv((u - v) * (u + v) * (sigma * sigma + 5)) % n
    y0 = (u**3 - v**3) * inv(u**3 + v**3) % n
    return a, d, x0, y0


def m_dbl(pt, a, n):
    X, Y, Z, T = pt
    A, B, C, Ee = X * X % n, Y * Y % n, 2 * Z * Z % n, 2 * T * Z % n
    D = a * A % n
    G, H = (D + B) % n, (D - B) % n
    F = (G - C) % n
    return Ee * F % n, G * H % n, F * G % n, Ee * H % n


def m_add(pt, x2, y2, a, d, n):
    X, Y, Z, T = pt
    Ee, H = (X * y2 + Y * x2) % n, (Y * y2 - a * X * x2) % n
    C = d * T * (x2 * y2 % n) % n
    F, G = (Z - C) % n, (Z + C) % n
    return Ee * F % n, H * G % n, F * G % n, Ee * H % n


def m_naf(e):
    out = []
    while e:
        d = (2 - e % 4) if e & 1 else 0
        e = (e - d) >> 1
        out.append(d)
    return out[::-1]


def m_stage1(sigma, b1, n, extra=1):
    a, d, x0, y0 = m_curve(sigma, n)
    digits = m_naf(ecm.stage1_exponent(b1) * extra)
    assert digits[0] == 1 and all(not (x and y) for x, y in zip(digits, digits[1:]))
    pt = (x0, y0, 1, x0 * y0 % n)
    for dg in digits[1:]:
        pt = m_dbl(pt, a, n)
        if dg:
            pt = m_add(pt, dg * x0 % n, y0, a, d, n)
    return pt, digits


def on_curve(pt, a, d, n):
    X, Y, Z, T = pt
    return (a * X * X + Y * Y - Z * Z - d * T * T) % n == 0 and (X * Y - T * Z) % n == 0


def _run(p, b1, b2, sigma, D=None, **kw):
    with orc.OracleEngine(p, ed.registers_needed(D)) as eng:
        res = ed.run(eng, p, b1, b2, sigma, D, **kw)
        return res, tuple(eng.get_int(r) for r in ed.POINT)


# ---- the curve ----

@pytest.mark.parametrize("p", [1009, 1277, 3001, 10007])
def test_curve_identities(p):
    mp = (1 << p) - 1
    for sigma in (6, 7, 11, 69, 2**31 + 11):
        a, d, x0, y0, a24, g = ed.curve(sigma, mp)
        assert g == 1 and (a, d, x0, y0) == m_curve(sigma, mp)
        assert (a * x0 * x0 + y0 * y0) % mp == (1 + d * x0 * x0 * y0 * y0) % mp
        sx0, sa24, sg = ecm.suyama(sigma, mp)
        assert sg == 1 and a24 == sa24 and (1 + y0) * pow(1 - y0, -1, mp) % mp == sx0       # the same group as the Montgomery curve
        # the model's formulas keep a point on the curve
        pt = (x0, y0, 1, x0 * y0 % mp)
        for step in (lambda q: m_dbl(q, a, mp), lambda q: m_add(q, x0, y0, a, d, mp), lambda q: m_add(q, -x0 % mp, y0, a, d, mp)):
            pt = step(pt)
            assert on_curve(pt, a, d, mp)


def test_naf():
    for e in list(range(1, 200)) + [ecm.stage1_exponent(100), 2**70 - 1, 2**70 + 1]:
        digits = ed.naf(e)
        assert digits == m_naf(e) and digits[0] == 1
        assert sum(d << i for i, d in enumerate(reversed(digits))) == e
        assert all(not (x and y) for x, y in zip(digits, digits[1:]))


def test_a_failing_inversion_is_reported_as_a_factor():
    p, f = 1009, 3454817
    mp = (1 << p) - 1
    assert ed.curve(f, mp)[5] % f == 0 and ed.curve(f, mp)[:5] == (0, 0, 0, 0, 0)
    with orc.OracleEngine(p, ed.FIXED_REGISTERS) as eng:
        res = ed.run(eng, p, 50, 0, f)
    assert res["g1"] % f == 0 and res["squarings"] == 0 and res["doublings"] == 0 and res["curve"] == "edwards"
    assert any(x % f == 0 for x in res["factors"])


# ---- stage 1 against the model ----

STAGE1 = [(1009, 69, 50, 3454817), (3001, 36, 100, 3217073), (10007, 61, 30, 240169), (1009, 7, 50, None)]


@pytest.mark.parametrize("p, sigma, b1, factor", STAGE1)
@pytest.mark.parametrize("check_every", [0, 8])
def test_stage1_point_is_the_models_and_the_montgomery_curves(p, sigma, b1, factor, check_every):
    mp = (1 << p) - 1
    res, point = _run(p, b1, 0, sigma, check_every=check_every)
    want, digits = m_stage1(sigma, b1, mp)
    assert point == tuple(c % mp for c in want)                     # X, Y, Z, T exactly
    assert res["g1"] == math.gcd(want[0], mp) == (factor or 1) and res["g2"] == 1
    assert res["factors"] == ([factor] if factor else [])
    assert (res["doublings"], res["additions"]) == (len(digits) - 1, sum(1 for d in digits[1:] if d)) and res["rollbacks"] == 0
    assert res["checks"] == (-(-(len(digits) - 1) // check_every) if check_every else 1)
    assert set(res) >= {"p", "b1", "b2", "D", "sigma", "factors", "g1", "g2", "squarings", "products", "prepares", "fused", "curve"}
    assert (res["curve"], res["sigma"], res["b2"], res["D"], res["fused"]) == ("edwards", sigma, 0, None, False)
    # the Montgomery ladder of the same sigma ends in the same point: (Z + Y : Z - Y) = (X_m : Z_m)
    with orc.OracleEngine(p, ecm.FIXED_REGISTERS) as eng:
        mres = ecm.run(eng, p, b1, 0, sigma)
        xm, zm = eng.get_int(ecm.R_XQ), eng.get_int(ecm.R_ZQ)
    X, Y, Z, T = point
    assert ((Z + Y) * zm - (Z - Y) * xm) % mp == 0
    assert mres["factors"] == res["factors"]


@pytest.mark.parametrize("p, sigma, b1, b2, D, g1, g2", [c for c in MONTGOMERY_CASES if c[3]])
def test_stage2_finds_what_the_montgomery_driver_finds(p, sigma, b1, b2, D, g1, g2):
    res, _ = _run(p, b1, b2, sigma, D, check_every=16)
    assert (res["g1"], res["g2"]) == (g1, g2) and res["factors"] == [f for f in (g1, g2) if f > 1]
    assert (res["b2"], res["D"], res["rollbacks"]) == (b2, D, 0)


# ---- the check ----

def _add_one_to_y(at, lane=None, times=1):
    left = [times]

    def fault(position, eng):
        if position == at and left[0]:
            left[0] -= 1
            if lane is None:
                eng.set_int(ed.R_Y, eng.get_int(ed.R_Y) + 1)
            else:
                eng.set_int(ed.R_Y, eng.get_int(ed.R_Y, lane=lane) + 1, lane=lane)
    return fault


@pytest.mark.parametrize("check_every, at", [(8, 20), (8, 8), (0, 33), (5, 70)])
def test_a_fault_once_is_rolled_back_and_the_run_ends_as_the_clean_one(check_every, at):
    p, sigma, b1 = 1009, 69, 50
    clean, point = _run(p, b1, 0, sigma, check_every=check_every)
    hit, hit_point = _run(p, b1, 0, sigma, check_every=check_every, fault=_add_one_to_y(at))
    assert hit["rollbacks"] == 1 and clean["rollbacks"] == 0 and hit_point == point
    assert hit["factors"] == clean["factors"] == [3454817] and hit["checks"] == clean["checks"] + 1
    assert hit["doublings"] > clean["doublings"]                     # the stretch was walked again


def test_a_fault_that_strikes_every_time_raises():
    p = 1009
    with orc.OracleEngine(p, ed.FIXED_REGISTERS) as eng:
        with pytest.raises(ed.EcmCheckError, match="lane 0") as err:
            ed.run(eng, p, 50, 0, 69, check_every=8, fault=_add_one_to_y(20, times=2))
    assert err.value.lanes == [0] and err.value.position == 24


def test_the_check_sees_a_fault_in_every_coordinate():
    p, mp = 1009, (1 << 1009) - 1
    for reg in ed.POINT:
        def fault(position, eng, reg=reg):
            if position == 5:
                eng.set_int(reg, eng.get_int(reg) ^ 2)
        with orc.OracleEngine(p, ed.FIXED_REGISTERS) as eng, pytest.raises(ed.EcmCheckError):
            ed.run(eng, p, 50, 0, 69, fault=fault)


# ---- lanes ----

def test_run_lanes_on_a_stand_in_with_lanes():
    p, b1, f = 1009, 50, 3454817
    sigmas = [69, 7, f, 11]
    mp = (1 << p) - 1
    with LaneOracles(p, ed.FIXED_REGISTERS, lanes=4) as eng:
        out = ed.run_lanes(eng, p, b1, 0, sigmas, check_every=8)
        points = [tuple(eng.get_int(r, lane=l) for r in ed.POINT) for l in range(4)]
    for l, s in enumerate(sigmas):
        if l == 2:
            assert out[l]["g1"] % f == 0
            continue
        want, _ = m_stage1(s, b1, mp)
        assert points[l] == tuple(c % mp for c in want) and out[l]["g1"] == math.gcd(want[0], mp)
    assert out[0]["factors"] == [f] and out[1]["factors"] == [] and all(r["rollbacks"] == 0 for r in out)
    # a fault in lane 3 alone takes all lanes back; the end is the clean one
    with LaneOracles(p, ed.FIXED_REGISTERS, lanes=4) as eng:
        hit = ed.run_lanes(eng, p, b1, 0, sigmas, check_every=8, fault=_add_one_to_y(13, lane=3))
        assert [tuple(eng.get_int(r, lane=l) for r in ed.POINT) for l in range(4)] == points
    assert all(r["rollbacks"] == 1 for r in hit) and [r["factors"] for r in hit] == [r["factors"] for r in out]
    with LaneOracles(p, ed.FIXED_REGISTERS, lanes=4) as eng, pytest.raises(ed.EcmCheckError, match="lanes 1, 3") as err:
        def fault(position, e):
            if position == 13:
                for l in (1, 3):
                    e.set_int(ed.R_T, e.get_int(ed.R_T, lane=l) + 1, lane=l)
        ed.run_lanes(eng, p, b1, 0, sigmas, check_every=8, fault=fault)
    assert err.value.lanes == [1, 3]
    with LaneOracles(p, ed.FIXED_REGISTERS, lanes=3) as eng, pytest.raises(ValueError, match="lane"):
        ed.run_lanes(eng, p, b1, 0, [6, 7])


# ---- batches: the check runs between them ----

def test_with_batches_the_check_runs_between_them():
    p, b1, sigma = 1009, 50, 69
    with Recording(p, ed.FIXED_REGISTERS) as plain, Recording(p, ed.FIXED_REGISTERS) as batched:
        want = ed.run(plain, p, b1, 0, sigma, check_every=8)
        got = ed.run(batched, p, b1, 0, sigma, check_every=8, batch=True)
        assert [plain.get_int(r) for r in ed.POINT] == [batched.get_int(r) for r in ed.POINT]
        assert got.pop("launches") == batched.launches == want["checks"] and got == want
        assert batched.begun == batched.ended == want["checks"] and batched.reads_inside == [] and batched.writes_inside == 0
        assert plain.begun == 0


# ---- engine calls per doubling, per addition and per check ----

class Counting(orc.OracleEngine):
    """the oracle with the fused operations of prmers_amd.Engine as the compositions they stand for, counting calls"""

    def __init__(self, p, regs):
        orc.OracleEngine.__init__(self, p, regs)
        self.calls = {}

    def _count(self, name):
        self.calls[name] = self.calls.get(name, 0) + 1

    def square_mul(self, src, a=1): self._count("square_mul"); self.o.square_mul(src, a)
    def mul(self, dst, src, a=1): self._count("mul"); self.o.mul(dst, src, a)
    def set_multiplicand(self, dst, src): self._count("set_multiplicand"); self.o.set_multiplicand(dst, src)
    def copy(self, dst, src): self._count("copy"); self.o.copy(dst, src)
    def add(self, dst, src): self._count("linear"); self.o.add(dst, src)
    def sub_reg(self, dst, src): self._count("linear"); self.o.sub_reg(dst, src)

    def square_mul_prepare(self, src, img, a=1):
        assert src != img
        self._count("square_mul_prepare"); self.o.set_multiplicand(img, src); self.o.square_mul(src, a)

    def square_mul_prepare_is_fused(self): return True

    def mul_copy(self, dst, src, dst_copy, a=1):
        assert len({dst, src, dst_copy}) == 3
        self._count("mul_copy"); self.o.mul(dst, src, a); self.o.copy(dst_copy, dst)

    def addsub(self, s, d, a, b):
        assert len({s, d, a, b}) == 4
        self._count("linear")
        self.o.copy(s, a); self.o.add(s, b); self.o.copy(d, a); self.o.sub_reg(d, b)


def sweeps(calls):
    """a squaring or a product is three sweeps, a multiplicand image two"""
    return 3 * sum(calls.get(k, 0) for k in ("square_mul", "square_mul_prepare", "mul", "mul_copy")) + 2 * calls.get("set_multiplicand", 0)


def _loaded(eng, sigma, mp):
    a, d, x0, y0, _, _ = ed.curve(sigma, mp)
    for reg, v in ((ed.R_IA, a), (ed.R_ID, d), (ed.R_IY0, y0), (ed.R_IXP, x0), (ed.R_IXM, -x0), (ed.R_IAXP, a * x0), (ed.R_IAXM, -a * x0),
                   (ed.R_IDTP, d * x0 * y0), (ed.R_IDTM, -d * x0 * y0)):
        eng.set_int(reg, v % mp); eng.set_multiplicand(reg, reg)
    pt = m_dbl((x0, y0, 1, x0 * y0 % mp), a, mp)
    for reg, v in zip(ed.POINT, pt):
        eng.set_int(reg, v)
    eng.calls.clear()
    return (a, d, x0, y0), pt


def test_calls_per_doubling_addition_and_check_are_those_of_the_design():
    p, sigma = 1009, 69
    mp = (1 << p) - 1
    with Counting(p, ed.FIXED_REGISTERS) as eng:
        (a, d, x0, y0), pt = _loaded(eng, sigma, mp)
        cv = ed._Edwards(ecm._Ops(eng))
        cv.dbl()
        # 3 squarings (one keeps the image of Z), 6 products (E = 2 T Z and Z' = F G also write their copy), images of F and H
        assert eng.calls == {"square_mul_prepare": 1, "square_mul": 2, "mul": 4, "mul_copy": 2, "set_multiplicand": 2, "linear": 2, "copy": 2}
        assert sweeps(eng.calls) == 31
        pt = m_dbl(pt, a, mp)
        assert tuple(eng.get_int(r) for r in ed.POINT) == pt
        for sign in (1, -1):
            eng.calls.clear()
            cv.add(sign)
            assert eng.calls == {"mul": 8, "mul_copy": 1, "set_multiplicand": 2, "linear": 3, "copy": 5} and sweeps(eng.calls) == 31
            pt = m_add(pt, sign * x0 % mp, y0, a, d, mp)
            assert tuple(eng.get_int(r) for r in ed.POINT) == pt
        eng.calls.clear()
        cv.sides()
        assert eng.calls == {"square_mul": 4, "mul": 2, "linear": 2, "copy": 4} and sweeps(eng.calls) == 18
        assert eng.get_int(ed.R_L) == eng.get_int(ed.R_R) == (a * pt[0] ** 2 + pt[1] ** 2) % mp
        assert tuple(eng.get_int(r) for r in ed.POINT) == pt          # the check leaves the point alone
    # without the fused operations: one more image per doubling
    with orc.OracleEngine(p, ed.FIXED_REGISTERS) as eng:
        ops = ecm._Ops(eng)
        assert not ops.has_prepare and not ops.fused
        eng.calls = {}
        _loaded(eng, sigma, mp)
        ed._Edwards(ops).dbl()
        assert (ops.squarings, ops.products, ops.prepares) == (3, 6, 3)
        ed._Edwards(ops).add(1)
        assert (ops.squarings, ops.products, ops.prepares) == (3, 15, 5)
    # a whole run counts what its doublings, additions and checks add up to
    with Counting(p, ed.FIXED_REGISTERS) as eng:
        res = ed.run(eng, p, 50, 0, sigma, check_every=8)
    assert res["fused"] is True
    assert res["squarings"] == 3 * res["doublings"] + 4 * res["checks"]
    assert res["products"] == 6 * res["doublings"] + 9 * res["additions"] + 2 * res["checks"]
    assert res["prepares"] == 2 * (res["doublings"] + res["additions"]) + 9
    per_digit = 31 + 31 * res["additions"] / res["doublings"]
    assert 34 < per_digit < 31 + 31 / 2                              # more than the ladder's 34 sweeps a bit


# ---- the entry point and the command line ----

def test_ecm_entry_point_takes_the_curve(monkeypatch):
    monkeypatch.setattr(E, "Engine", LaneOracles)
    LaneOracles.made = []
    res = ecm.ecm(1009, 50, 0, sigma=69, curves=3, curve="edwards", check_every=8)
    assert res["factors"] == [3454817] and res["curve"] == "edwards" and res["sigmas"] == [69] and res["checks"] > 1
    res = ecm.ecm(1009, 50, 0, sigma=69, curves=4, lanes=2, seed=3, curve="edwards")
    assert 3454817 in res["factors"] and len(res["batch"]) == 2 and res["batch"][0]["curve"] == "edwards" and res["checks"] == 1
    assert "curve" not in ecm.ecm(1009, 50, 0, sigma=69)
    with pytest.raises(ValueError, match="curve"):
        ecm.ecm(1009, 50, 0, sigma=69, curve="weierstrass")
    with pytest.raises(ValueError, match="check_every"):
        ecm.ecm(1009, 50, 0, sigma=69, check_every=8)


def test_the_command_line_passes_the_options(monkeypatch):
    seen = {}

    def fake(*a, **k):
        seen["kw"] = k
        return {"factors": [1]}
    monkeypatch.setattr(ecm, "ecm", fake)
    assert ecm.main(["1009", "50", "--curve", "edwards", "--check-every", "64"]) == 0 and seen["kw"] == {"curve": "edwards", "check_every": 64}
    assert ecm.main(["1009", "50", "--curve", "montgomery"]) == 0 and seen["kw"] == {}
    assert ecm.main(["1009", "50"]) == 0 and seen["kw"] == {}


def test_arguments():
    assert ed.registers_needed() == ed.FIXED_REGISTERS == ecm.FIXED_REGISTERS and ed.registers_needed(30) == ecm.registers_needed(30)
    assert max(ed.R_IH, *ed.POINT, *ed.KEEP) < ed.FIXED_REGISTERS
    assert not {ecm.R_XQ, ecm.R_ZQ, ecm.R_A24} & set(ed.POINT)       # stage 2's inputs are written while the point is read
    with orc.OracleEngine(1009, 5) as eng, pytest.raises(ValueError):
        ed.run(eng, 1009, 20, 0, 7)
    with orc.OracleEngine(1009, ed.FIXED_REGISTERS) as eng:
        for bad in (dict(sigma=5), dict(b1=1), dict(check_every=-1)):
            kw = dict(b1=20, sigma=7, check_every=0)
            kw.update(bad)
            with pytest.raises(ValueError):
                ed.run(eng, 1009, kw["b1"], 0, kw["sigma"], check_every=kw["check_every"])
        with pytest.raises(ValueError):
            ed.run(eng, 1009, 20, 120, 7, 30)                        # stage 2 needs the table's registers
