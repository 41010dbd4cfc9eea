"""ECM stage 1 on twisted Edwards curves with an on-curve error check (the reference: src/modes/RunEcmTwistedEdwards.cpp, its default
ECM mode); stage 2 is ecm.py's, on the Montgomery form of the same curve.

    python -m prmers_amd.ecm P B1 [B2] --curve edwards [--check-every N] [...]

Why:      an x-only Montgomery ladder carries no invariant that could be tested, so a flipped bit silently turns a curve into garbage.  A
          point (X : Y : Z : T) in extended coordinates on a X^2 + Y^2 = Z^2 + d T^2 can be tested at any time: a wrong coordinate breaks
          the equation.  This mode buys that check, not speed: with a general `a` a NAF digit costs more sweeps than a ladder step
          (DESIGN.md 7e).
Curve:    from Suyama's sigma, u = sigma^2 - 5, v = 4 sigma:  A + 2 = (v - u)^3 (3u + v) / (4 u^3 v),  B = u / v,  a = (A + 2) / B,
          d = (A - 2) / B,  X0 = u^2 v / ((u - v)(u + v)(sigma^2 + 5)),  Y0 = (u^3 - v^3) / (u^3 + v^3).  (X0, Y0) lies on
          a x^2 + y^2 = 1 + d x^2 y^2, which is birationally the Montgomery curve of ecm.suyama(sigma): (A + 2) / 4 is its a24 and
          (1 + Y0) / (1 - Y0) its x0.  One inversion on the host for all four denominators; one that fails has found a factor.
Stage 1:  Q = E P by double-and-add over the NAF of E from the top, the addend +P or -P affine (Z2 = 1):
              doubling   A = X^2, B = Y^2, C = 2 Z^2, E = 2 T Z, D = a A, G = D + B, H = D - B, F = G - C
                         X' = E F, Y' = G H, Z' = F G, T' = E H                       3 squarings, 6 products, 2 images (F, H)
              addition   E = X1 Y2 + Y1 X2, H = Y1 Y2 - a X1 X2, C = d T1 T2, D = Z1, F = D - C, G = D + C
                         X' = E F, Y' = H G, Z' = F G, T' = E H                       9 products, 2 images (F, H)
          The constants stay multiplicand images throughout: a, d, Y0, and for either sign X2 = +-X0, a X2 and d T2 = +-d X0 Y0.  The
          image of Z that E = 2 T Z needs comes out of the squaring of Z (square_mul_prepare).  g1 = gcd(X, Mp): the neutral point is
          (0 : 1 : 1 : 0).
Check:    L = a X^2 + Y^2 and R = Z^2 + d T^2 in scratch registers, compared on every lane at once (Engine.equal_lanes; is_equal on an
          object without lanes) every check_every NAF digits and at the end of stage 1.  After a check that passes X, Y, Z, T are copied
          to four keep registers; after one that fails in any lane all lanes go back to them and the digits since are walked again (all
          lanes share one call sequence).  The same check failing twice in a row raises EcmCheckError, which names the lanes.  Those
          copies open the next stretch and the two sides close it, so with batch=True a stretch with all of them is one batch and only
          the comparison runs between two batches.  The engine operations and the lane and batch plumbing are ecm.py's (_Ops, _IO).
Stage 2:  Q maps to the Montgomery point (Z + Y : Z - Y); that goes into ecm.R_XQ, ecm.R_ZQ, a24 as an image into ecm.R_A24, and
          ecm._stage2 runs as it does for ecm.run.  (No invariant there: the check covers stage 1.)
Restart:  checkpoint=, checkpoint_every=, stop_after= as in ecm.py (its docstring), counted in NAF digits; the state is the extended
          point's four registers as canonical residues and the index of the next digit.  A checkpoint is written only from a point that has
          just passed the check, so no file ever holds a point off the curve: checkpoint_every is rounded up to a multiple of check_every,
          a check stands behind digit stop_after, and check_every = 0 with a checkpoint is refused.  save= writes the line of the
          Montgomery curve of the same sigma, x = (Z + Y) / (Z - Y).  Stage 2 has no checkpoint; it restarts from that line.
Not here: the reference's torsion-16 and iv163 families, windowed NAF, a twisted Edwards stage 2, stage-2 checkpoints.
"""
from . import ecm as M
from .pm1 import D_CHOICES, big_gcd

# the point, the last point that passed a check, temporaries (the check's L, R and a square share them), images
(R_X, R_Y, R_Z, R_T, R_KX, R_KY, R_KZ, R_KT, R_U, R_V, R_G, R_F,
 R_IA, R_ID, R_IY0, R_IXP, R_IXM, R_IAXP, R_IAXM, R_IDTP, R_IDTM, R_IZ, R_IF, R_IH) = range(24)
R_L, R_R, R_W = R_U, R_V, R_G
FIXED_REGISTERS = M.FIXED_REGISTERS          # stage 2 is ecm.py's and lives in its registers, so the file is that size from the start


class EcmCheckError(RuntimeError):
    """the on-curve check failed again right after a roll-back; .lanes: the lanes that failed, .position: the NAF digit it stood behind"""

    def __init__(self, lanes, position):
        RuntimeError.__init__(self, "ECM on-curve check failed twice behind NAF digit %d in lane%s %s"
                              % (position, "" if len(lanes) == 1 else "s", ", ".join(map(str, lanes))))
        self.lanes, self.position = list(lanes), position


def registers_needed(D=None, stage2="projective", lanes=1, inverse="host"):
    """registers of an engine for this driver: stage 1 alone (D=None) or with ecm.py's stage 2 over the wheel D, in its mode `stage2` and
    with its `inverse` on `lanes` lanes"""
    return FIXED_REGISTERS if D is None else M.registers_needed(D, stage2, lanes, inverse)


def naf(e):
    """the non-adjacent form of e >= 1, digits in {-1, 0, 1}, most significant first (the first is 1)"""
    out = []
    while e:
        d = 0
        if e & 1:
            d = 2 - (e & 3)
            e -= d
        out.append(d)
        e >>= 1
    return out[::-1]


def curve(sigma, n, use_gmp=None):
    """(a, d, X0, Y0, a24, 1) of the curve of `sigma` modulo n, or (0, 0, 0, 0, 0, g) when the inversion fails: g = gcd of the product of
    the four denominators and n, a factor of n (n itself for a degenerate sigma)"""
    u = (sigma * sigma - 5) % n
    v = 4 * sigma % n
    u3, v3 = u * u * u % n, v * v * v % n
    dens = [4 * u3 * v % n, u, (u - v) * (u + v) * (sigma * sigma + 5) % n, (u3 + v3) % n]
    prefix = [1]
    for x in dens:
        prefix.append(prefix[-1] * x % n)
    inv = M.mod_inverse(prefix[-1], n, use_gmp)
    if inv == 0:
        return 0, 0, 0, 0, 0, big_gcd(prefix[-1], n, use_gmp)
    invs = [0] * len(dens)
    for i in range(len(dens) - 1, -1, -1):       # one inversion for all: 1 / dens[i] = (prod before i) / (prod up to i)
        invs[i] = inv * prefix[i] % n
        inv = inv * dens[i] % n
    ap2 = pow(v - u, 3, n) * (3 * u + v) % n * invs[0] % n             # A + 2
    binv = v * invs[1] % n                                             # 1 / B
    a, d = ap2 * binv % n, (ap2 - 4) * binv % n
    x0 = u * u * v % n * invs[2] % n
    y0 = (u3 - v3) * invs[3] % n
    if (a * x0 * x0 + y0 * y0 - 1 - d * x0 * x0 % n * y0 * y0) % n:
        raise AssertionError("the start point of sigma = %d is not on its curve" % sigma)
    return a, d, x0, y0, ap2 * pow(4, -1, n) % n, 1


class _Edwards:
    """extended twisted Edwards arithmetic on the point in (R_X, R_Y, R_Z, R_T); the constants are the images named above"""

    def __init__(self, ops):
        self.o, self.e = ops, ops.e

    def _tail(self, h):
        """X' = E F, T' = E H, Y' = G H, Z' = F G from E (in R_X and in R_T), F in R_F, G in R_G and H in register h"""
        o, e = self.o, self.e
        o.prep(R_IF, R_F); o.prep(R_IH, h)
        o.mul(R_X, R_IF); o.mul(R_T, R_IH)
        e.copy(R_Y, R_G); o.mul(R_Y, R_IH)
        o.mul_copy(R_G, R_IF, R_Z)

    def dbl(self):
        o, e = self.o, self.e
        o.sq_prep(R_Z, R_IZ, 2)                  # C = 2 Z^2, and the image of Z
        o.sq(R_X); o.mul(R_X, R_IA)              # D = a X^2
        o.sq(R_Y)                                # B
        o.addsub(R_G, R_U, R_X, R_Y)             # G = D + B, H = D - B
        o.mul_copy(R_T, R_IZ, R_X, 2)            # E = 2 T Z, in R_T and R_X
        e.copy(R_F, R_G); e.sub_reg(R_F, R_Z)    # F = G - C
        self._tail(R_U)

    def add(self, sign):
        """the point += sign P, P = (X0, Y0) affine"""
        o, e = self.o, self.e
        ix, iax, idt = (R_IXP, R_IAXP, R_IDTP) if sign > 0 else (R_IXM, R_IAXM, R_IDTM)
        e.copy(R_U, R_X); o.mul(R_U, R_IY0)      # X1 Y2
        e.copy(R_V, R_Y); o.mul(R_V, ix)         # Y1 X2
        e.add(R_U, R_V)                          # E
        o.mul(R_Y, R_IY0); o.mul(R_X, iax)       # Y1 Y2, a X1 X2
        e.sub_reg(R_Y, R_X)                      # H
        o.mul(R_T, idt)                          # C = d T1 T2
        o.addsub(R_G, R_F, R_Z, R_T)             # G = D + C, F = D - C with D = Z1
        e.copy(R_X, R_U); e.copy(R_T, R_U)       # E
        self._tail(R_Y)

    def sides(self):
        """R_L = a X^2 + Y^2, R_R = Z^2 + d T^2"""
        o, e = self.o, self.e
        e.copy(R_L, R_X); o.sq(R_L); o.mul(R_L, R_IA)
        e.copy(R_F, R_Y); o.sq(R_F); e.add(R_L, R_F)
        e.copy(R_R, R_T); o.sq(R_R); o.mul(R_R, R_ID)
        e.copy(R_F, R_Z); o.sq(R_F); e.add(R_R, R_F)


POINT = (R_X, R_Y, R_Z, R_T)
KEEP = (R_KX, R_KY, R_KZ, R_KT)


def _run_curves(eng, p, b1, b2, sigmas, D, check_every, fault, use_gmp, by_lane, batch, mode="projective", inverse="host",
                checkpoint=None, checkpoint_every=0, stop_after=0, save=None, group=0):
    M._check_mode(mode)
    M._check_engine_inverse(eng, inverse, mode)
    size = {"lanes": len(sigmas), "inverse": inverse} if inverse != "host" else {}
    if b1 < 2:
        raise ValueError("B1 must be at least 2")
    if min(sigmas) < M.SIGMA_MIN:
        raise ValueError("sigma must be at least %d" % M.SIGMA_MIN)
    if check_every < 0:
        raise ValueError("check_every must be 0 (the end of stage 1 only) or a number of NAF digits")
    if checkpoint and not check_every:
        raise ValueError("a checkpoint is written only from a point that has just passed the on-curve check, so that no file ever holds a "
                         "point that is off the curve: with check_every = 0 the only check stands at the end of stage 1; give check_every")
    if checkpoint_every and check_every:         # ... and so only at a check: the next multiple of check_every
        checkpoint_every = -(-checkpoint_every // check_every) * check_every
    mp = (1 << p) - 1
    have = getattr(eng, "reg_count", None)
    stage2 = b2 > b1
    if stage2:
        if D is None:
            D = max([d for d in D_CHOICES if have is None or M.registers_needed(d, mode, **size) <= have] or [0])
            D = min(D, M.choose_D(eng.n, b1, b2, stage2=mode, **size)) if D else 0
        if D not in D_CHOICES:
            raise ValueError("stage 2 needs D in %s and an engine with registers_needed(D) registers" % (D_CHOICES,))
    need = registers_needed(D if stage2 else None, mode, **size)
    if have is not None and have < need:
        raise ValueError("the engine has %d registers, ECM on Edwards curves with D = %s needs %d" % (have, D if stage2 else None, need))
    ops = M._Ops(eng)
    ed = _Edwards(ops)
    lanes = range(len(sigmas))
    io = M._IO(eng, len(sigmas), by_lane, batch)
    batched, put, get = io.batched, io.put, io.get
    count = {"doublings": 0, "additions": 0, "checks": 0, "rollbacks": 0}

    def results(g1, g2, more2=None, xs=None):
        more = {**(more2 or {}), **io.launches()}
        return [{"p": p, "b1": b1, "b2": b2 if stage2 else 0, "D": D if stage2 else None, "sigma": sigmas[l],
                 "factors": [f for f in (g1[l], g2[l]) if 1 < f < mp], "g1": g1[l], "g2": g2[l],
                 "squarings": ops.squarings, "products": ops.products, "prepares": ops.prepares, "fused": ops.fused, "curve": "edwards", **count, **more,
                 **({"x": xs[l]} if xs and l in xs else {})} for l in lanes]

    setup = [curve(s, mp, use_gmp) for s in sigmas]
    failed = [c[5] != 1 for c in setup]          # the inversion failed: its argument shares g with Mp, which is the curve's result
    g1 = [c[5] if bad else 1 for c, bad in zip(setup, failed)]
    g2 = [1] * len(sigmas)
    if all(failed):
        return results(g1, g2)
    if any(failed):                              # such a lane rides along on a valid curve whose outcome is dropped
        s = M.SIGMA_MIN
        while curve(s, mp, use_gmp)[5] != 1:
            s += 1
        setup = [curve(s, mp, use_gmp) if bad else c for c, bad in zip(setup, failed)]

    # ---- the constants, as images, and the start point ----
    e = M.stage1_exponent(b1)
    if stage2:   # the primes in (B1, B2] that divide D have no residue class in stage 2
        for q in (2, 3, 5, 7, 11):
            if D % q == 0 and b1 < q <= b2:
                if save:
                    raise ValueError("save: with B1 = %d < 11 and a stage 2 over D = %d the stage-1 scalar also takes the prime %d, so the "
                                     "line would claim a B1 it does not describe; save a stage-1-only run" % (b1, D, q))
                e *= q
    digits = naf(e)
    restart = M._Restart(checkpoint, checkpoint_every, stop_after, "edwards", p, b1, b2 if stage2 else 0, D if stage2 else None,
                         sigmas, failed, e, group, get, POINT)
    state = restart.load(len(digits) - 1)        # a checkpoint of another run is refused here, before anything is written
    for reg, f in ((R_IA, lambda a, d, x, y: a), (R_ID, lambda a, d, x, y: d), (R_IY0, lambda a, d, x, y: y),
                   (R_IXP, lambda a, d, x, y: x), (R_IXM, lambda a, d, x, y: -x),
                   (R_IAXP, lambda a, d, x, y: a * x), (R_IAXM, lambda a, d, x, y: -a * x),
                   (R_IDTP, lambda a, d, x, y: d * x * y), (R_IDTM, lambda a, d, x, y: -d * x * y)):
        put(reg, [f(*c[:4]) % mp for c in setup]); ops.prep(reg, reg)
    if state is None:
        put(R_X, [c[2] for c in setup]); put(R_Y, [c[3] for c in setup]); eng.set(R_Z, 1)
        put(R_T, [c[2] * c[3] % mp for c in setup])
    else:                                        # the point of the checkpoint: it had passed the check when it was written
        for reg, values in zip(POINT, state):
            put(reg, values)

    def check():
        """the lanes in which a X^2 + Y^2 != Z^2 + d T^2, from the two sides in R_L and R_R"""
        count["checks"] += 1
        if by_lane and getattr(eng, "equal_lanes", None):
            ok = eng.equal_lanes(R_L, R_R)
        elif not by_lane and getattr(eng, "is_equal", None):
            ok = [eng.is_equal(R_L, R_R)]
        else:                                    # an object with neither: both sides as integers
            ok = [x == y for x, y in zip(get(R_L), get(R_R))]
        return [l for l, good in enumerate(ok) if not good]

    # ---- stage 1: the NAF from the top, in stretches that end in a check ----
    # A stretch is one batch: the four copies the last check asks for (the point to the keep registers after a pass, back from them after
    # a failure), the digits, the two sides of the check.  Between two batches only the comparison runs.
    # A check stands behind every check_every-th digit counted from the top, whatever digit the run began at, behind digit stop_after and
    # at the end.  A step of the checkpoints is a digit below the leading one: pos - 1 of them are done.
    pos, last = restart.start + 1, len(digits)   # digits[0] = 1 is the start point itself
    passed = True                                # the start point is on the curve (curve() asserts it)
    while pos < last or count["checks"] == 0:
        end = min(last, ((pos - 1) // check_every + 1) * check_every + 1) if check_every else last
        if stop_after > pos - 1:
            end = min(end, stop_after + 1)
        for attempt in (0, 1):
            with batched():
                for k, r in zip(KEEP, POINT):
                    eng.copy(k, r) if passed else eng.copy(r, k)
                for i in range(pos, end):
                    ed.dbl(); count["doublings"] += 1
                    if digits[i]:
                        ed.add(digits[i]); count["additions"] += 1
                    if fault is not None:
                        fault(i, eng)
                ed.sides()
            bad = check()
            passed = not bad
            if passed:
                break
            if attempt:
                raise EcmCheckError(bad, end - 1)
            count["rollbacks"] += 1
        pos = end
        restart.reached(pos - 1, last - 1)
    for l, x in enumerate(get(R_X)):
        if not failed[l]:
            g1[l] = mp if x == 0 else big_gcd(x, mp, use_gmp)

    # ---- stage 2: ecm.py's, on the Montgomery point (Z + Y : Z - Y) ----
    more2 = xs = None
    if stage2 or save:
        ops.addsub(M.R_XQ, M.R_ZQ, R_Z, R_Y)     # (R_XQ and R_ZQ are two of the keep registers, which are done; stage 2 leaves the point alone)
    if save:                                     # the line of the Montgomery curve of the same sigma: x = (Z + Y) / (Z - Y)
        xs = M._save_stage1(eng, ops, get, p, b1, sigmas, failed, g1, get(M.R_ZQ), save, inverse, use_gmp)
    if stage2:
        put(M.R_A24, [c[4] for c in setup]); ops.prep(M.R_A24, M.R_A24)
        more2 = M._stage2(eng, ops, M._Curve(ops), p, b1, b2, D, failed, g1, g2, batched, get, use_gmp, put, mode, inverse)
    restart.finish()
    return results(g1, g2, {**(more2 or {}), **restart.more()}, xs)


def run(eng, p, b1, b2=0, sigma=M.SIGMA_MIN, D=None, check_every=0, fault=None, use_gmp=None, batch=False, stage2="projective", inverse="host",
        checkpoint=None, checkpoint_every=0, stop_after=0, save=None, group=0):
    """One twisted Edwards curve of ECM on 2^p - 1 with bounds B1 and B2 (B2 <= B1: stage 1 only) on `eng`, an engine for exponent p with
    registers_needed(D) registers.  check_every: NAF digits between two on-curve checks (0: only the one at the end of stage 1).
    fault(position, eng), for tests, is called after every NAF digit.  batch=True: the stretches between checks run inside eng.batch().
    Afterwards R_X, R_Y, R_Z, R_T hold the stage-1 point.  stage2, inverse: the mode of ecm.py's stage 2 and who inverts in it, as for ecm.run.
    checkpoint, checkpoint_every, stop_after, group: as for ecm.run, in NAF digits, with the state (R_X, R_Y, R_Z, R_T) and the digit's
    index.  A checkpoint is written only from a point that has just passed the check: checkpoint_every is rounded up to a multiple of
    check_every, a check stands behind digit stop_after, and check_every = 0 with a checkpoint is a ValueError.  A resumed run checks
    behind the same digits as an uninterrupted one; its doublings, additions and checks count from the checkpoint on.
    save: as for ecm.run; the line is that of the Montgomery curve of the same sigma, x = (Z + Y) / (Z - Y).
    -> the keys of ecm.run, and curve: "edwards", doublings, additions (those carried out, repeated ones included), checks, rollbacks"""
    return _run_curves(eng, p, b1, b2, [sigma], D, check_every, fault, use_gmp, False, batch, stage2, inverse,
                       checkpoint, checkpoint_every, stop_after, save, group)[0]


def run_lanes(eng, p, b1, b2, sigmas, D=None, check_every=0, fault=None, use_gmp=None, batch=False, stage2="projective", inverse="host",
              checkpoint=None, checkpoint_every=0, stop_after=0, save=None, group=0):
    """len(sigmas) == eng.lanes curves at once, curve l in lane l, through the engine calls of ONE run(); the check compares every lane in
    one launch sequence (Engine.equal_lanes) and a failure in any lane takes all lanes back.  -> one result per curve"""
    sigmas = list(sigmas)
    if len(sigmas) != getattr(eng, "lanes", 1) or not sigmas:
        raise ValueError("run_lanes needs one sigma per lane: %d given, the engine has %d lanes" % (len(sigmas), getattr(eng, "lanes", 1)))
    return _run_curves(eng, p, b1, b2, sigmas, D, check_every, fault, use_gmp, True, batch, stage2, inverse,
                       checkpoint, checkpoint_every, stop_after, save, group)
