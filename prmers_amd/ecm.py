"""ECM factoring of a Mersenne number 2^p - 1 on the engine: Montgomery curves, stages 1 and 2 (the reference: src/modes/RunEcm.cpp).

    python -m prmers_amd.ecm P B1 [B2] [--sigma S] [--curves N] [--lanes B] [--D 30|210|2310] [--plan SPEC] [--onelaunch] [--batch] [--device N]
                             [--curve montgomery|edwards] [--check-every N] [--stage2 projective|affine] [--inverse host|engine]
                             [--save FILE] [--checkpoint FILE] [--checkpoint-every STEPS] [--stop-after STEPS]
    python -m prmers_amd.ecm --resume-file FILE B2 [--lanes B] [--D ..] [--stage2 ..] [--inverse ..] [--onelaunch] [--batch] [...]
    exit code 0: a factor was found, 1: none, 2: the arguments, 3: stopped at --stop-after with the checkpoint written

Curve:    Suyama's parametrisation from sigma: u = sigma^2 - 5, v = 4 sigma, the point (u^3 : v^3) on B y^2 = x^3 + A x^2 + x with
          a24 = (A + 2) / 4 = (v - u)^3 (3 u + v) / (16 u^3 v).  The start is taken affine, x0 = u^3 / v^3 and Z = 1: one modular inversion
          on the host (libgmp, or pow(x, -1, N) below 2^22 bits); an inversion that fails has found a factor.
Stage 1:  Q = E P, E = prod_{q <= B1 prime} q^floor(log_q B1), by one Montgomery ladder on x-coordinates; g1 = gcd(Z_Q, Mp).  A ladder
          step doubles (X2 : Z2) and adds (X3 : Z3), whose difference is the start point:
              s = X2 + Z2, d = X2 - Z2, ss = s^2, dd = d^2, t = ss - dd
              X2' = ss dd, Z2' = t (dd + a24 t)
              a = (X3 - Z3) s, b = (X3 + Z3) d, X3' = (a + b)^2, Z3' = x0 (a - b)^2
          4 squarings, 6 products, and multiplicand images of s, d, dd and dd + a24 t.  s and d are both squared and multiplied by:
          Engine.square_mul_prepare squares them and keeps the image the squaring's row sweep passes through, which saves the two
          sweeps of a set_multiplicand for each (38 -> 34 sweeps per step; include/mi355_engine.h).  a24 and x0 stay images throughout.
Stage 2:  the standard continuation on x-coordinates over the wheel D: every prime q in (B1, B2] is k D +- j with j in
          J = {1 <= j < D/2, gcd(j, D) = 1} (pm1.stage2_pairs: the same cover as P-1, k = 0 included), and q | ord(Q) exactly when
          x(k D Q) = x(j Q), so  A <- A (X_k Z_j - X_j Z_k)  with (X_j : Z_j) = j Q and (X_k : Z_k) = k D Q, all projective (no inversion);
          g2 = gcd(A, Mp) with g1 divided out.  Baby points: the odd multiples of Q by differential addition of 2 Q; the table keeps
          multiplicand images of X_j and of Z_j.  Giant steps: D Q and k0 D Q by short ladders on Q, then (k + 1) D Q = k D Q + D Q with
          difference (k - 1) D Q.  Per pair: 3 products and one set_multiplicand (X_k Z_j, Z_k X_j, the image of the difference, A times
          it).  0 Q = (1 : 0) is a valid giant point: the k = 0 terms are Z_j.
Affine:   stage2="affine" / --stage2 affine works on x = X / Z instead: the table holds images of -x_j, the giant points become images of
          x_k, and a pair is A <- A (x_k + (-x_j)), ONE engine call, Engine.mul_sum (one product of 3 sweeps where the plan has the
          fused sum, the engine's two-product composition where not; the composition copy, mul, mul, add for an object without it).
          Points are normalised in blocks by Montgomery's trick ON THE ENGINE (_stage2_affine.normalise): prefix products
          c_i = c_(i-1) Z_i, c_m read on every lane (get_ints), one host inversion per lane (mod_inverses: at small exponents one for
          all lanes, the trick once more, across the lanes), u written back (set_ints; Mp - u for the baby block, so the negation is
          free), then inv_i = u c_(i-1), u <- u Z_i, x_i = X_i inv_i: at most 4 products and 4
          set_multiplicand per point.  The baby table is one block; X_j, Z_j, c_j take 3 |J| registers, of which 2 |J| are free
          afterwards and hold the giant points in blocks of floor(2 |J| / 3).  A lane whose c_m has no inverse gets u = 1 and rides
          along.  The host keeps zacc = prod c_m per lane and g2 = gcd(A zacc, Mp) with g1 divided out: the Z product finds a factor
          modulo which some point is the point at infinity -- which is also how the k = 0 pairs are covered (q = j divides the order
          exactly when Z_j vanishes), so no pair is walked for k = 0.  Opt-in; the default stays projective.
Engine inverse:  inverse="engine" / --inverse engine (affine only, an engine with mul_sibling, include/mi355_lanecross.h): the read of
          c_m on every lane, the host's inversions and the write of every lane become lanecross.invert -- Montgomery's trick ACROSS the
          lanes on the engine, 2 ceil(log2 B) products by a sibling lane's image, one lane read, ONE host inversion and one broadcast
          write a block whatever B is.  The Z product stays on the engine too: ZACC <- ZACC c_m a block (one set_multiplicand, one
          product) and A ZACC is formed there at the end and read once.  A block in which some lane's c_m has no inverse (a point at
          infinity, a factor in a Z) makes the product over the lanes non-invertible: that block runs the host's way, with the same
          inverses as before (1 for the lanes without one), and is counted in "inverse_fallbacks".  Inverses are unique, so g1, g2,
          the accumulator and "normalised" are those of inverse="host".  L + 3 registers on top (registers_needed).  Opt-in too.

The driver works on anything with the interface of prmers_amd.Engine; addsub and square_mul_prepare are used when the object has them
and replaced by the compositions they stand for when it has not.
Lanes:    all curves of a batch make the same engine calls (the ladder bits come from B1, the stage-2 pairs from B1, B2 and D); only x0 and
          a24 differ.  run_lanes() puts curve l into lane l of an engine with lanes (Engine(..., lanes=B), include/mi355_lanes.h) and
          issues the calls of one run(): B curves per launch sequence.  --lanes B / ecm(lanes=B) batches the curves that way.
Batches:  on an engine with one-launch products (--onelaunch) every ladder step is some twenty launches and copies of almost no work.
          batch=True / --batch runs the stage-1 ladder and the stage-2 loops inside Engine.batch() (include/mi355_batch.h): the engine
          queues the calls and runs each queue as one launch.  Writes of constants inside those loops run the queue first; the x0, a24
          and start point go in before the first batch and Z, the accumulator and the stage-1 point are read after the last has ended.
Edwards:  --curve edwards / ecm(curve="edwards") runs stage 1 in twisted Edwards extended coordinates (prmers_amd/ecm_edwards.py), the
          same group as the Montgomery curve of that sigma, where a X^2 + Y^2 = Z^2 + d T^2 is tested every --check-every NAF digits and
          at the end, on all lanes at once (Engine.equal_lanes), with a roll-back to the last point that passed.  It costs more sweeps
          per bit than the ladder: it buys the check, not speed.  Stage 2 is the one below for both (_stage2).  The
          per-lane reads at the end of a stage go through Engine.get_ints where the object has it: one launch sequence for all lanes.
Restart:  all opt-in; with none of it given the calls below are the calls of before.  checkpoint= / --checkpoint FILE names the file of
          the stage-1 state (prmers_amd/ecm_files.py): every checkpoint_every ladder steps, and once more when stop_after steps are done,
          the running batch ends, the four ladder registers are read on all lanes (get_ints: canonical residues, so the file fits any
          plan, with or without onelaunch and batches), the file is replaced (os.replace) and a new batch begins; at stop_after the run
          raises EcmStopped (the command line: exit code 3).  Where the file exists the run goes on from it: the header must name this
          run's p, B1, scalar, curve form, sigmas and group, a24 and x0 are rebuilt from the sigmas, the registers go back with set_ints
          and the ladder goes on at the recorded bit; the exact arithmetic modulo 2^p - 1 reaches the residues of the run that was never
          stopped.  Stage 2 gets NO checkpoint: it restarts from the stage-1 line.  save= / --save FILE appends, after stage 1, the
          GMP-ECM / Prime95 resume line of every curve with gcd(Z_Q, N) = 1, x = X_Q / Z_Q; run_saved() / ecm_saved() /
          --resume-file FILE B2 run stage 2 alone on such lines (a24 from sigma, the point (x : 1)), ours or another program's.
Not here: PRAC chains, stage-2 checkpoints, raw images of lane engines, resume lines with PARAM != 0, ECM= worktodo
          lines, the PrimeNet JSON, a C++ twin.
"""
import argparse
import contextlib
import ctypes
import json
import os
import random
import sys

from . import ecm_files
from .pm1 import D_CHOICES, DEFAULT_BUDGET, SLOW_GCD_BITS, big_gcd, load_gmp, primes_upto, residues, stage2_pairs

# ladder points a and b, the stage-1 result Q, 2 Q, D Q, three giant points, temporaries, images, the accumulator
(R_XA, R_ZA, R_XB, R_ZB, R_XQ, R_ZQ, R_X2, R_Z2, R_XD, R_ZD, R_XG0, R_ZG0, R_XG1, R_ZG1, R_XG2, R_ZG2,
 R_S, R_D, R_U, R_V, R_W, R_T, R_IS, R_ID, R_IT, R_A24, R_X0, R_A) = range(28)
FIXED_REGISTERS = 28
SIGMA_MIN = 6                 # sigma in {0, 1, 3, 5} and a few more give degenerate curves; the customary range starts here


# ---- integers ---------------------------------------------------------------------------------------------------------------------

def stage1_exponent(b1):
    """E = prod_{q <= B1 prime} q^floor(log_q B1)"""
    e = 1
    for q in primes_upto(b1):
        qq = q
        while qq * q <= b1:
            qq *= q
        e *= qq
    return e


STAGE2_MODES = ("projective", "affine")


def _check_mode(stage2):
    if stage2 not in STAGE2_MODES:
        raise ValueError('stage2 must be "projective" or "affine"')


INVERSE_MODES = ("host", "engine")


def _check_inverse(inverse, stage2):
    if inverse not in INVERSE_MODES:
        raise ValueError('inverse must be "host" or "engine"')
    if inverse == "engine" and stage2 != "affine":
        raise ValueError('inverse="engine" belongs to stage2="affine": the projective stage 2 inverts nothing')


def _check_engine_inverse(eng, inverse, stage2):
    """_check_inverse, and for "engine" that the object has the product across lanes"""
    _check_inverse(inverse, stage2)
    if inverse == "engine" and getattr(eng, "mul_sibling", None) is None:
        raise ValueError('inverse="engine" needs an engine with mul_sibling (include/mi355_lanecross.h); this object has none')


def registers_needed(D, stage2="projective", lanes=1, inverse="host"):
    """registers of an engine that runs stage 2 with this D: images of X_j and Z_j for every j in J plus FIXED_REGISTERS; for
    stage2="affine" X_j, Z_j and the prefix product c_j for every j in J plus FIXED_REGISTERS -- nothing on top: the running inverse of a
    normalisation lives in R_U, a temporary of the point additions, which do not run meanwhile.  inverse="engine" on `lanes` lanes adds
    L + 3, L = ceil(log2 lanes): the Z product and the L + 2 of lanecross.invert (its copy, the image of 1, an image a level)"""
    if D not in D_CHOICES:
        raise ValueError("D must be one of %s" % (D_CHOICES,))
    _check_mode(stage2)
    _check_inverse(inverse, stage2)
    more = 0
    if inverse == "engine":
        from . import lanecross
        more = 1 + lanecross.registers_needed(lanes)
    return (3 if stage2 == "affine" else 2) * len(residues(D)) + FIXED_REGISTERS + more


def choose_D(n, b1, b2, budget=DEFAULT_BUDGET, stage2="projective", lanes=1, inverse="host"):
    """the largest D whose register file (registers_needed(D, stage2, lanes, inverse) + the engine's work buffer, 8 n bytes each) fits
    `budget` bytes and that is not wider than the interval (B1, B2] itself"""
    best = D_CHOICES[0]
    for D in D_CHOICES[1:]:
        if (registers_needed(D, stage2, lanes, inverse) + 1) * 8 * n <= budget and D <= max(b2 - b1, D_CHOICES[0]):
            best = D
    return best


def mod_inverse(x, n, use_gmp=None):
    """x^-1 mod n, or 0 when gcd(x, n) != 1: libgmp when it loads (use_gmp=None) or is asked for (True), pow(x, -1, n) otherwise -- which
    is refused above about 2^22 bits, where it would run for hours without a word."""
    G = load_gmp() if use_gmp in (None, True) else None
    if use_gmp and G is None:
        raise RuntimeError("libgmp does not load")
    if G is None:
        if int(n).bit_length() > SLOW_GCD_BITS:
            raise RuntimeError("inversion modulo a %d-bit number needs libgmp (it did not load); pow(x, -1, n) would take hours at this size"
                               % int(n).bit_length())
        try:
            return pow(int(x) % n, -1, n)
        except ValueError:
            return 0
    P = ctypes.POINTER(G.Mpz)
    G.__gmpz_invert.argtypes = [P, P, P]
    G.__gmpz_invert.restype = ctypes.c_int
    zx, zn, zr = G.Mpz(), G.Mpz(), G.Mpz()
    for z in (zx, zn, zr):
        G.__gmpz_init(ctypes.byref(z))
    try:
        for z, v in ((zx, int(x) % n), (zn, n)):
            raw = int(v).to_bytes((int(v).bit_length() + 7) // 8 or 1, "little")
            G.__gmpz_import(ctypes.byref(z), len(raw), -1, 1, -1, 0, raw)
        if not G.__gmpz_invert(ctypes.byref(zr), ctypes.byref(zx), ctypes.byref(zn)):
            return 0
        size = (G.__gmpz_sizeinbase(ctypes.byref(zr), 2) + 7) // 8
        buf = ctypes.create_string_buffer(size or 1)
        count = ctypes.c_size_t(0)
        G.__gmpz_export(buf, ctypes.byref(count), -1, 1, -1, 0, ctypes.byref(zr))
        return int.from_bytes(buf.raw[:count.value], "little")
    finally:
        for z in (zx, zn, zr):
            G.__gmpz_clear(ctypes.byref(z))


SHARED_INVERSE_BITS = 1 << 16    # up to here three host products cost less than an inversion (Python's % is quadratic, libgmp's invert is not)


def mod_inverses(xs, n, use_gmp=None):
    """[mod_inverse(x, n) for x in xs], 0 where there is none.  Below SHARED_INVERSE_BITS one inversion serves all of them (Montgomery's
    trick on the host: three products a value); when that one fails, some value has no inverse and they are inverted one by one."""
    xs = [int(x) % n for x in xs]
    if len(xs) > 1 and int(n).bit_length() <= SHARED_INVERSE_BITS:
        prefix = [1]
        for x in xs:
            prefix.append(prefix[-1] * x % n)
        u = mod_inverse(prefix[-1], n, use_gmp) if prefix[-1] else 0
        if u:
            out = [0] * len(xs)
            for i in range(len(xs) - 1, -1, -1):
                out[i] = u * prefix[i] % n
                u = u * xs[i] % n
            return out
    return [mod_inverse(x, n, use_gmp) if x else 0 for x in xs]


def suyama(sigma, n, use_gmp=None):
    """(x0, a24, 1) of the curve of `sigma` modulo n with the start point affine, or (0, 0, g) when the one inversion fails: g = gcd of
    its argument and n, a factor of n (n itself for a degenerate sigma)"""
    u = (sigma * sigma - 5) % n
    v = 4 * sigma % n
    u3, v3 = u * u * u % n, v * v * v % n
    den = 16 * u3 * v % n                       # a24's denominator; the inverted value is den v^3
    inv = mod_inverse(den * v3 % n, n, use_gmp)
    if inv == 0:
        return 0, 0, big_gcd(den * v3 % n, n, use_gmp)
    x0 = u3 * den % n * inv % n
    a24 = pow(v - u, 3, n) * (3 * u + v) % n * v3 % n * inv % n
    return x0, a24, 1


# ---- engine operations, with the compositions for objects that lack the fused ones ---------------------------------------------------

def _factor(a):
    return () if a == 1 else (a,)


class _Ops:
    def __init__(self, eng, use_fused=True):
        self.e = eng
        self.squarings = self.products = self.prepares = 0
        self.has_prepare = bool(use_fused and getattr(eng, "square_mul_prepare", None))
        self.fused = bool(self.has_prepare and getattr(eng, "square_mul_prepare_is_fused", lambda: False)())
        self.has_addsub = getattr(eng, "addsub", None) is not None
        self.has_mul_copy = getattr(eng, "mul_copy", None) is not None
        self.has_mul_sum = getattr(eng, "mul_sum", None) is not None
        self.fused_sum = bool(self.has_mul_sum and getattr(eng, "mul_sum_is_fused", lambda: False)())

    # a: the small factor of the engine's products; a call without one is issued without one
    def sq(self, r, a=1):
        self.e.square_mul(r, *_factor(a))
        self.squarings += 1

    def mul(self, dst, img, a=1):
        self.e.mul(dst, img, *_factor(a))
        self.products += 1

    def mul_copy(self, dst, img, dst_copy, a=1):
        """dst = a dst img, dst_copy = the same"""
        if self.has_mul_copy:
            self.e.mul_copy(dst, img, dst_copy, *_factor(a))
        else:
            self.e.mul(dst, img, *_factor(a)); self.e.copy(dst_copy, dst)
        self.products += 1

    def mul_sum(self, dst, img_a, img_b, tmp):
        """dst = dst (a + b) for two images: the engine's mul_sum (one product where its plan has the fused sum), else the composition"""
        if self.has_mul_sum:
            self.e.mul_sum(dst, img_a, img_b, tmp)
            self.products += 1 if self.fused_sum else 2
        else:
            self.e.copy(tmp, dst); self.mul(dst, img_a); self.mul(tmp, img_b); self.e.add(dst, tmp)

    def prep(self, dst, src):
        self.e.set_multiplicand(dst, src)
        self.prepares += 1

    def sq_prep(self, src, img, a=1):
        """img = the image of src, src = a src^2"""
        if self.has_prepare:
            self.e.square_mul_prepare(src, img, *_factor(a))
        else:
            self.prep(img, src)
            self.e.square_mul(src, *_factor(a))
        self.squarings += 1

    def addsub(self, s, d, a, b):
        """s = a + b, d = a - b; s, d, a, b four different registers"""
        if self.has_addsub:
            self.e.addsub(s, d, a, b)
        else:
            self.e.copy(s, a); self.e.add(s, b)
            self.e.copy(d, a); self.e.sub_reg(d, b)

    def sub_to(self, dst, a, b):
        self.e.copy(dst, a); self.e.sub_reg(dst, b)


class _IO:
    """what a run of curves reads and writes on its engine, for both drivers: by_lane=False, one curve on the engine as it is; by_lane=True,
    curve l in lane l of an engine with `count` lanes.  batch: stretches of calls run inside eng.batch() where the object has one."""

    def __init__(self, eng, count, by_lane, batch):
        self.e, self.lanes, self.by_lane = eng, range(count), by_lane
        self.batching = bool(batch and getattr(eng, "batch", None))
        self.launches0 = eng.batch_stats()[1] if self.batching else 0

    def batched(self):
        return self.e.batch() if self.batching else contextlib.nullcontext()

    def launches(self):
        """{"launches": batch launches since the start} of a batched run, nothing otherwise"""
        return {"launches": self.e.batch_stats()[1] - self.launches0} if self.batching else {}

    def put(self, reg, values):
        if not self.by_lane:
            self.e.set_int(reg, values[0])
            return
        if getattr(self.e, "set_ints", None):
            self.e.set_ints(reg, values)         # every lane in one upload and one launch (include/mi355_lanewise.h)
            return
        self.e.set(reg, 0)       # a lane is written into a register of residues; the register may hold an image of the last batch
        for l in self.lanes:
            self.e.set_int(reg, values[l], lane=l)

    def get(self, reg):
        if self.by_lane and getattr(self.e, "get_ints", None):
            return self.e.get_ints(reg)          # every lane in one launch sequence (include/mi355_lanewise.h)
        return [self.e.get_int(reg, lane=l) for l in self.lanes] if self.by_lane else [self.e.get_int(reg)]


class _Curve:
    """x-only arithmetic on the curve whose a24 is the image in R_A24; a point is a pair of registers (X, Z)"""

    def __init__(self, ops):
        self.o, self.e = ops, ops.e

    def dbl_tail(self, out):
        """out = the double of the point whose (X + Z)^2 is in R_S and (X - Z)^2 in R_D"""
        o, e = self.o, self.e
        X, Z = out
        o.sub_to(Z, R_S, R_D)                   # t = ss - dd
        o.prep(R_IT, R_D)
        e.copy(X, R_S); o.mul(X, R_IT)          # X' = ss dd
        e.copy(R_W, Z); o.mul(R_W, R_A24); e.add(R_W, R_D)
        o.prep(R_W, R_W)
        o.mul(Z, R_W)                           # Z' = t (dd + a24 t)

    def dbl(self, out, pt):
        o = self.o
        o.addsub(R_S, R_D, pt[0], pt[1])
        o.sq(R_S); o.sq(R_D)
        self.dbl_tail(out)

    def add(self, out, p1, p2, diff):
        """out = p1 + p2 where diff = p1 - p2, all projective; out may be any of them"""
        o, e = self.o, self.e
        o.addsub(R_U, R_V, p1[0], p1[1])
        o.addsub(R_S, R_D, p2[0], p2[1])
        o.prep(R_IS, R_S); o.prep(R_ID, R_D)
        o.mul(R_V, R_IS); o.mul(R_U, R_ID)      # a = (X1 - Z1)(X2 + Z2), b = (X1 + Z1)(X2 - Z2)
        o.addsub(R_S, R_D, R_V, R_U)
        o.sq(R_S); o.sq(R_D)
        o.prep(R_IT, diff[1]); o.mul(R_S, R_IT)  # X' = Zd (a + b)^2
        o.prep(R_IT, diff[0]); o.mul(R_D, R_IT)  # Z' = Xd (a - b)^2
        e.copy(out[0], R_S); e.copy(out[1], R_D)

    def ladder_step(self, a, b):
        """a = 2 a, b = a + b, where b - a is the start point (x0 : 1) whose x0 is the image in R_X0"""
        o = self.o
        o.addsub(R_S, R_D, a[0], a[1])
        o.addsub(R_U, R_V, b[0], b[1])
        o.sq_prep(R_S, R_IS); o.sq_prep(R_D, R_ID)
        o.mul(R_V, R_IS); o.mul(R_U, R_ID)
        o.addsub(b[0], b[1], R_V, R_U)
        o.sq(b[0]); o.sq(b[1]); o.mul(b[1], R_X0)
        self.dbl_tail(a)

    def small_ladder(self, r0, r1, m, pt):
        """(r0, r1) = (m pt, (m + 1) pt), m >= 1, pt projective and none of r0, r1"""
        self.e.copy(r0[0], pt[0]); self.e.copy(r0[1], pt[1])
        self.dbl(r1, pt)
        for i in range(m.bit_length() - 2, -1, -1):
            if (m >> i) & 1:
                self.add(r0, r0, r1, pt); self.dbl(r1, r1)
            else:
                self.add(r1, r0, r1, pt); self.dbl(r0, r0)


def _stage2_affine(eng, ops, cv, p, b1, b2, D, failed, g1, g2, batched, get, put, use_gmp, inverse="host"):
    """_stage2 with stage2="affine" (the module's docstring): tables of x-coordinates, one mul_sum per pair.
    inverse="engine": a block's inverses by lanecross.invert and the Z product in a register (the module's docstring, "Engine inverse").
    -> the keys an affine run adds to its results"""
    mp = (1 << p) - 1
    lanes = range(len(failed))
    Q = (R_XQ, R_ZQ)
    info = {"stage2": "affine", "fused_sum": ops.fused_sum, "normalised": 0}
    on_engine = inverse == "engine"
    if on_engine:
        from . import lanecross
        info.update({"inverse": "engine", "inverse_fallbacks": 0})
    pairs = stage2_pairs(b1, b2, D)
    if not pairs or not any(g1[l] != mp for l in lanes if not failed[l]):
        return info
    J = residues(D)
    triple = [tuple(FIXED_REGISTERS + 3 * i + r for r in range(3)) for i in range(len(J))]      # X_j, Z_j, c_j
    slot = {j: triple[i][0] for i, j in enumerate(J)}                                            # ... and then the image of -x_j
    free = [r for t in triple for r in t[1:]]
    giant = [tuple(free[3 * i:3 * i + 3]) for i in range(max(1, len(free) // 3))]
    zacc = [1] * len(failed)
    if on_engine:        # behind the table: the Z product, then lanecross.invert's copy, image of 1 and an image a level
        R_ZACC = FIXED_REGISTERS + 3 * len(J)
        cross = list(range(R_ZACC + 1, R_ZACC + 1 + lanecross.registers_needed(len(failed))))

    def normalise(block, negate):
        """block: register triples (X, Z, C) with a point (X : Z) in the first two.  Afterwards X holds the image of x = X / Z (of -x
        when negate) and Z and C are spent.  Montgomery's trick on the engine: prefix products c_i = c_(i-1) Z_i up, one inversion per
        lane on the host, inv_i = u c_(i-1) and u <- u Z_i down.  At most 4 products and 4 set_multiplicand per point."""
        c = [block[0][1]] + [t[2] for t in block[1:]]            # c_1 is Z_1 itself
        for i in range(1, len(block)):
            X, Z, C = block[i]
            ops.prep(Z, Z); eng.copy(C, c[i - 1]); ops.mul(C, Z)
        done = False
        if on_engine:
            ops.prep(R_IT, c[-1]); ops.mul(R_ZACC, R_IT)         # the Z product stays on the engine
            done = lanecross.invert(eng, c[-1], R_U, cross, negate, use_gmp, ops)[0]
            info["inverse_fallbacks"] += not done                # some lane's c_m has no inverse: this block the host's way
        if not done:
            cms = get(c[-1])
            if not on_engine:
                for l, cm in enumerate(cms):
                    zacc[l] = zacc[l] * cm % mp
            us = [u or 1 for u in mod_inverses(cms, mp, use_gmp)]    # a lane without an inverse rides along on 1: its factor is in zacc
            put(R_U, [mp - u for u in us] if negate else us)
        for i in range(len(block) - 1, 0, -1):
            X, Z, C = block[i]
            ops.prep(R_IT, R_U); ops.mul(c[i - 1], R_IT)         # inv_i = u c_(i-1)
            ops.mul(R_U, Z)                                      # u <- u Z_i
            ops.prep(c[i - 1], c[i - 1]); ops.mul(X, c[i - 1])   # x_i = X_i inv_i
            ops.prep(X, X)
        X = block[0][0]
        ops.prep(R_IT, R_U); ops.mul(X, R_IT); ops.prep(X, X)    # inv_1 = u
        info["normalised"] += len(block)

    with batched():
        if on_engine:
            lanecross.prepare_one(eng, cross[1])
            eng.set(R_ZACC, 1)
        two = (R_X2, R_Z2)
        cv.dbl(two, Q)
        # baby points: the odd multiples of Q as residues, then one block of the normalisation: the table holds images of -x_j
        prev, cur, nxt = (R_XG0, R_ZG0), (R_XG1, R_ZG1), (R_XG2, R_ZG2)
        for r in (0, 1):
            eng.copy(prev[r], Q[r]); eng.copy(cur[r], Q[r])
        for j in range(1, J[-1] + 1, 2):
            if j in slot:
                eng.copy(slot[j], cur[0]); eng.copy(slot[j] + 1, cur[1])
            if j + 2 <= J[-1]:
                cv.add(nxt, cur, two, prev)
                prev, cur, nxt = cur, nxt, prev
        normalise(triple, True)
        eng.set(R_A, 1)
        # giant steps from k = 1 on (the k = 0 pairs are the Z_j, which are in zacc): cur = k D Q, nxt = (k + 1) D Q, in blocks
        k, k1 = max(min(pairs), 1), max(pairs)
        if k <= k1:
            DQ = (R_XD, R_ZD)
            cv.small_ladder(DQ, (R_XG0, R_ZG0), D, Q)
            cur, nxt, spare = (R_XG0, R_ZG0), (R_XG1, R_ZG1), (R_XG2, R_ZG2)
            cv.small_ladder(cur, nxt, k, DQ)
        while k <= k1:
            block = []
            while k <= k1 and len(block) < len(giant):
                if pairs.get(k):
                    t = giant[len(block)]
                    eng.copy(t[0], cur[0]); eng.copy(t[1], cur[1])
                    block.append((k, t))
                if k + 1 < k1:
                    cv.add(spare, nxt, DQ, cur)
                    cur, nxt, spare = nxt, spare, cur
                else:
                    cur, nxt = nxt, cur
                k += 1
            if block:
                normalise([t for _, t in block], False)
            for kk, t in block:
                for j in pairs[kk]:
                    ops.mul_sum(R_A, t[0], slot[j], R_T)         # A <- A (x_k + (-x_j))
        if on_engine:                                            # A zacc, formed on the engine beside A
            ops.prep(R_IT, R_ZACC); eng.copy(R_T, R_A); ops.mul(R_T, R_IT)
    for l, acc in enumerate(get(R_T if on_engine else R_A)):
        if not failed[l] and g1[l] != mp:
            v = acc * zacc[l] % mp
            g = mp if v == 0 else big_gcd(v, mp, use_gmp)
            g2[l] = g // big_gcd(g, g1[l], use_gmp)
    return info


def _stage2(eng, ops, cv, p, b1, b2, D, failed, g1, g2, batched, get, use_gmp, put=None, stage2="projective", inverse="host"):
    """Stage 2 on the stage-1 point in (R_XQ, R_ZQ) of the Montgomery curve whose a24 is the image in R_A24, for both drivers (this one
    and ecm_edwards): the table of baby points, the giant steps and the accumulator, then g2[l] for every lane that has a stage 2.
    batched() opens a batch or nothing, get(reg) reads every lane, put(reg, values) writes every lane (stage2="affine" only).
    inverse: "host" or, for stage2="affine" on an object with mul_sibling, "engine".
    -> the keys the mode adds to the results (none for "projective")"""
    _check_engine_inverse(eng, inverse, stage2)
    if stage2 == "affine":
        return _stage2_affine(eng, ops, cv, p, b1, b2, D, failed, g1, g2, batched, get, put, use_gmp, inverse)
    mp = (1 << p) - 1
    lanes = range(len(failed))
    Q = (R_XQ, R_ZQ)
    if not any(g1[l] != mp for l in lanes if not failed[l]):
        return
    J = residues(D)
    slot = {j: (FIXED_REGISTERS + 2 * i, FIXED_REGISTERS + 2 * i + 1) for i, j in enumerate(J)}
    pairs = stage2_pairs(b1, b2, D)
    if pairs:
        with batched():
            two = (R_X2, R_Z2)
            cv.dbl(two, Q)
            # baby points: the odd multiples of Q; cur = j Q, prev = (j - 2) Q ((-1) Q has the x of Q)
            prev, cur, nxt = (R_XG0, R_ZG0), (R_XG1, R_ZG1), (R_XG2, R_ZG2)
            for r in (0, 1):
                eng.copy(prev[r], Q[r]); eng.copy(cur[r], Q[r])
            for j in range(1, J[-1] + 1, 2):
                if j in slot:
                    ops.prep(slot[j][0], cur[0]); ops.prep(slot[j][1], cur[1])
                if j + 2 <= J[-1]:
                    cv.add(nxt, cur, two, prev)
                    prev, cur, nxt = cur, nxt, prev
            # giant steps: cur = k D Q, nxt = (k + 1) D Q
            DQ = (R_XD, R_ZD)
            cv.small_ladder(DQ, (R_XG0, R_ZG0), D, Q)
            k0, k1 = min(pairs), max(pairs)
            cur, nxt, spare = (R_XG0, R_ZG0), (R_XG1, R_ZG1), (R_XG2, R_ZG2)
            if k0 == 0:
                eng.set(cur[0], 1); eng.set(cur[1], 0)
                eng.copy(nxt[0], DQ[0]); eng.copy(nxt[1], DQ[1])
            else:
                cv.small_ladder(cur, nxt, k0, DQ)
            eng.set(R_A, 1)
            for k in range(k0, k1 + 1):
                for j in pairs.get(k, ()):
                    eng.copy(R_T, cur[0]); ops.mul(R_T, slot[j][1])      # X_k Z_j
                    eng.copy(R_W, cur[1]); ops.mul(R_W, slot[j][0])      # Z_k X_j
                    eng.sub_reg(R_T, R_W)
                    ops.prep(R_T, R_T)
                    ops.mul(R_A, R_T)
                if k + 1 < k1:
                    if k == 0:
                        cv.dbl(spare, DQ)        # the difference would be 0 Q
                    else:
                        cv.add(spare, nxt, DQ, cur)
                    cur, nxt, spare = nxt, spare, cur
                else:
                    cur, nxt = nxt, cur
        for l, acc in enumerate(get(R_A)):
            if not failed[l] and g1[l] != mp:   # (a curve whose stage 1 gave Mp itself has no stage 2)
                g = mp if acc == 0 else big_gcd(acc, mp, use_gmp)
                g2[l] = g // big_gcd(g, g1[l], use_gmp)


def _wheel(eng, b1, b2, D, mode, size):
    """the D of a run on `eng` (given, or the largest the engine's registers and the interval allow), checked against its registers"""
    have = getattr(eng, "reg_count", None)
    stage2 = b2 > b1
    if stage2:
        if D is None:
            D = max([d for d in D_CHOICES if have is None or registers_needed(d, mode, **size) <= have] or [0])
            D = min(D, choose_D(eng.n, b1, b2, stage2=mode, **size)) if D else 0
        if D not in D_CHOICES:
            raise ValueError("stage 2 needs D in %s and an engine with registers_needed(D) registers" % (D_CHOICES,))
    need = registers_needed(D, mode, **size) if stage2 else FIXED_REGISTERS
    if have is not None and have < need:
        raise ValueError("the engine has %d registers, ECM with D = %s needs %d" % (have, D if stage2 else None, need))
    return D


class EcmStopped(Exception):
    """stage 1 stopped at stop_after and its checkpoint is written; .path: the checkpoint, .step: the steps of stage 1 that are done"""

    def __init__(self, path, step):
        Exception.__init__(self, "ECM stage 1 stopped after step %d; checkpoint %s" % (step, path))
        self.path, self.step = path, step


class _Restart:
    """the checkpoints of a stage 1, for both drivers (this one and ecm_edwards).  A step is one scalar digit below the leading one: a
    ladder step here, a NAF digit there.  With no path it says "go to the end" once and is never heard of again: nothing it does touches
    the engine unless a checkpoint is due."""

    def __init__(self, path, every, stop_after, form, p, b1, b2, D, sigmas, failed, scalar, group, get, regs):
        if every < 0 or stop_after < 0:
            raise ValueError("checkpoint_every and stop_after are numbers of steps, 0 for none")
        if (every or stop_after) and not path:
            raise ValueError("checkpoint_every and stop_after need checkpoint=, the file the state goes to")
        self.path, self.every, self.stop_after, self.get, self.regs = path, every, stop_after, get, regs
        self.start, self.resumed = 0, False
        if path:
            bits, digest = ecm_files.scalar_digest(scalar)
            self.header = {"p": p, "b1": b1, "b2": b2, "D": D, "curve": form, "sigmas": [int(s) for s in sigmas],
                           "substitutes": [l for l, bad in enumerate(failed) if bad], "scalar_bits": bits, "scalar_sha256": digest,
                           "group": group}

    def load(self, steps):
        """the registers' values of an existing checkpoint (then .start is its step, of the run's `steps`), None without one;
        CheckpointError when the file is another run's.  The engine is not touched."""
        if not self.path or not os.path.exists(self.path):
            return None
        header, values = ecm_files.read_checkpoint(self.path)
        for k, what in (("p", "exponent"), ("b1", "B1"), ("curve", "curve form"), ("sigmas", "sigmas (or their number: one a lane)"),
                        ("substitutes", "substitute lanes"), ("scalar_bits", "stage-1 scalar (B1, and B2 and D below 11)"),
                        ("scalar_sha256", "stage-1 scalar (B1, and B2 and D below 11)"), ("group", "group of curves")):
            if header[k] != self.header[k]:
                raise ecm_files.CheckpointError("%s is the checkpoint of another run: its %s is not this run's" % (self.path, what))
        if header["registers"] != len(self.regs) or not 0 <= header["next"] - 1 <= steps:
            raise ecm_files.CheckpointError("%s: %d registers at digit %d do not fit this run" % (self.path, header["registers"], header["next"]))
        self.start, self.resumed = header["next"] - 1, True
        return values

    def mark(self, step, steps):
        """the step up to which the run goes on from `step` before it looks here again"""
        m = steps
        if self.every:
            m = min(m, (step // self.every + 1) * self.every)
        if self.stop_after > step:
            m = min(m, self.stop_after)
        return m

    def reached(self, step, steps):
        """after the batch that ended at `step` is closed: write what is due; at stop_after raise EcmStopped"""
        if not self.path or step <= self.start:
            return
        stop = step == self.stop_after
        if stop or (self.every and step % self.every == 0 and step < steps):
            ecm_files.write_checkpoint(self.path, dict(self.header, next=step + 1), [self.get(r) for r in self.regs])
        if stop:
            raise EcmStopped(self.path, step)

    def finish(self):
        """a normal end: the file has served"""
        if self.path and os.path.exists(self.path):
            os.remove(self.path)

    def more(self):
        return {"resumed_at": self.start} if self.resumed else {}


def _save_stage1(eng, ops, get, p, b1, sigmas, failed, g1, zs, path, inverse, use_gmp):
    """The resume lines of a finished stage 1 whose point is in (R_XQ, R_ZQ), zs = the lanes' Z_Q: x = X_Q / Z_Q for every curve that
    has one -- its start was set up, stage 1 found nothing and Z_Q is invertible -- appended to `path`.  The inverses come from the host
    (mod_inverses) or, for inverse="engine", from lanecross.invert in the temporaries of the ladder, which are free now; where some lane's
    Z_Q has no inverse that one cannot succeed, and the host does it.  R_XQ, R_ZQ and the constants stay.  -> {lane: x}"""
    mp = (1 << p) - 1
    want = [l for l in range(len(sigmas)) if not failed[l] and g1[l] == 1 and zs[l] % mp]
    xs = {}
    if not want:
        return xs
    done = False
    if inverse == "engine":
        from . import lanecross
        work = [R_X2, R_Z2, R_XD, R_ZD, R_XG0, R_ZG0, R_XG1, R_ZG1, R_XG2, R_ZG2, R_S, R_D, R_W, R_T, R_IS, R_ID, R_IT, R_A]
        work = work[:lanecross.registers_needed(len(sigmas))]
        lanecross.prepare_one(eng, work[1])
        done = lanecross.invert(eng, R_ZQ, R_U, work, False, use_gmp, ops)[0]
        if done:
            ops.prep(R_U, R_U); eng.copy(R_V, R_XQ); ops.mul(R_V, R_U)
            values = get(R_V)
            xs = {l: values[l] for l in want}
    if not done:
        xq = get(R_XQ)
        xs = {l: xq[l] * u % mp for l, u in zip(want, mod_inverses([zs[l] for l in want], mp, use_gmp)) if u}
    ecm_files.append_resume_lines(path, [ecm_files.resume_line(p, sigmas[l], b1, xs[l]) for l in sorted(xs)])
    return xs


LADDER = (R_XA, R_ZA, R_XB, R_ZB)            # the state of an interrupted stage 1


def _run_curves(eng, p, b1, b2, sigmas, D, use_fused, use_gmp, by_lane, batch=False, mode="projective", inverse="host",
                checkpoint=None, checkpoint_every=0, stop_after=0, save=None, group=0):
    """The curves of `sigmas` through one sequence of engine calls: the ladder bits come from B1 and the stage-2 pairs from (B1, B2, D),
    so only the data differ.  by_lane=False: one curve on an engine used as it is (run).  by_lane=True: curve l in lane l of an engine
    with len(sigmas) lanes (run_lanes); every engine call then acts on all of them.  batch: the ladder and the stage-2 loops run inside
    eng.batch() where the object has one (else as without).  mode: the stage 2, "projective" or "affine"; inverse: who inverts in the affine
    one, "host" or "engine".  checkpoint, checkpoint_every, stop_after, save, group: run().  -> one result per curve"""
    _check_mode(mode)
    _check_engine_inverse(eng, inverse, mode)
    size = {"lanes": len(sigmas), "inverse": inverse} if inverse != "host" else {}
    if b1 < 2:
        raise ValueError("B1 must be at least 2")
    if min(sigmas) < SIGMA_MIN:
        raise ValueError("sigma must be at least %d" % SIGMA_MIN)
    mp = (1 << p) - 1
    stage2 = b2 > b1
    D = _wheel(eng, b1, b2, D, mode, size)
    e = stage1_exponent(b1)
    if stage2:   # the primes in (B1, B2] that divide D have no residue class in stage 2
        for q in (2, 3, 5, 7, 11):
            if D % q == 0 and b1 < q <= b2:
                if save:
                    raise ValueError("save: with B1 = %d < 11 and a stage 2 over D = %d the stage-1 scalar also takes the prime %d, so the "
                                     "line would claim a B1 it does not describe; save a stage-1-only run" % (b1, D, q))
                e *= q
    ops = _Ops(eng, use_fused)
    cv = _Curve(ops)
    lanes = range(len(sigmas))
    io = _IO(eng, len(sigmas), by_lane, batch)
    batched, put, get = io.batched, io.put, io.get

    def results(g1, g2, more2=None, xs=None):
        more = {**(more2 or {}), **io.launches()}
        return [{"p": p, "b1": b1, "b2": b2 if stage2 else 0, "D": D if stage2 else None, "sigma": sigmas[l],
                 "factors": [f for f in (g1[l], g2[l]) if 1 < f < mp], "g1": g1[l], "g2": g2[l],
                 "squarings": ops.squarings, "products": ops.products, "prepares": ops.prepares, "fused": ops.fused, **more,
                 **({"x": xs[l]} if xs and l in xs else {})} for l in lanes]

    setup = [suyama(s, mp, use_gmp) for s in sigmas]
    failed = [g != 1 for _, _, g in setup]   # the inversion failed: its argument shares g with Mp, which is the curve's result
    g1 = [g if bad else 1 for (_, _, g), bad in zip(setup, failed)]
    g2 = [1] * len(sigmas)
    if all(failed):
        return results(g1, g2)
    if any(failed):              # such a lane rides along on a valid curve whose outcome is dropped
        s = SIGMA_MIN
        while suyama(s, mp, use_gmp)[2] != 1:
            s += 1
        setup = [suyama(s, mp, use_gmp) if bad else c for c, bad in zip(setup, failed)]

    # ---- stage 1: the ladder, in one stretch or, with checkpoints, in stretches that end where one is due ----
    restart = _Restart(checkpoint, checkpoint_every, stop_after, "montgomery", p, b1, b2 if stage2 else 0, D if stage2 else None,
                       sigmas, failed, e, group, get, LADDER)
    steps = e.bit_length() - 1                   # step k works on bit steps - 1 - k
    state = restart.load(steps)                  # a checkpoint of another run is refused here, before anything is written
    put(R_A24, [c[1] for c in setup]); ops.prep(R_A24, R_A24)
    put(R_X0, [c[0] for c in setup]); ops.prep(R_X0, R_X0)
    a, b = (R_XA, R_ZA), (R_XB, R_ZB)
    if state is None:
        put(R_XA, [c[0] for c in setup]); eng.set(R_ZA, 1)
    else:
        for reg, values in zip(LADDER, state):
            put(reg, values)
    step = restart.start
    while True:
        upto = restart.mark(step, steps)
        with batched():
            if state is None and step == 0:
                cv.dbl(b, a)                     # (a, b) = (P, 2 P)
            for i in range(steps - 1 - step, steps - 1 - upto, -1):
                if (e >> i) & 1:
                    cv.ladder_step(b, a)
                else:
                    cv.ladder_step(a, b)
            if upto == steps:
                eng.copy(R_XQ, a[0]); eng.copy(R_ZQ, a[1])
        step = upto
        restart.reached(step, steps)
        if step == steps:
            break
    zs = get(R_ZQ)
    for l, z in enumerate(zs):
        if not failed[l]:
            g1[l] = mp if z == 0 else big_gcd(z, mp, use_gmp)
    xs = _save_stage1(eng, ops, get, p, b1, sigmas, failed, g1, zs, save, inverse, use_gmp) if save else None

    more2 = None
    if stage2:
        more2 = _stage2(eng, ops, cv, p, b1, b2, D, failed, g1, g2, batched, get, use_gmp, put, mode, inverse)
    restart.finish()
    return results(g1, g2, {**(more2 or {}), **restart.more()}, xs)


def run(eng, p, b1, b2=0, sigma=SIGMA_MIN, D=None, use_fused=True, use_gmp=None, batch=False, stage2="projective", inverse="host",
        checkpoint=None, checkpoint_every=0, stop_after=0, save=None, group=0):
    """One curve of ECM on 2^p - 1 with bounds B1 and B2 (B2 <= B1: stage 1 only) on `eng`, an engine for exponent p with at least
    FIXED_REGISTERS registers (stage 1) or registers_needed(D) (stage 2).  use_fused=False forces set_multiplicand + square_mul in
    place of square_mul_prepare.  Afterwards registers R_XQ, R_ZQ hold the stage-1 point.  batch=True: the ladder and the stage-2 loops
    run inside eng.batch() (an engine with one-launch products); the result then has "launches", the batch launches it took.
    stage2="affine": stage 2 on normalised x-coordinates, one mul_sum per pair (the module's docstring); the engine then needs
    registers_needed(D, "affine") registers and the result of a run with a stage 2 has "stage2": "affine", "fused_sum" (the engine's
    mul_sum is one product) and "normalised" (points normalised).  The prime factors it finds are those of the projective stage 2 and
    those modulo which a baby or giant point is the point at infinity.  It is meant for small exponents on lane engines: every block of
    points costs one modular inversion per lane on the host, which at exponents in the millions is minutes.
    inverse="engine" (with stage2="affine", on an object with mul_sibling): a block's inverses by Montgomery's trick across the lanes on
    the engine, one host inversion a block whatever the lane count, and the Z product kept in a register (prmers_amd/lanecross.py); the
    engine then needs registers_needed(D, "affine", lanes, "engine") registers and the result has "inverse": "engine" and
    "inverse_fallbacks", the blocks that went the host's way because some lane's product had no inverse.  Same g1, g2 and accumulator.
    checkpoint (a path), checkpoint_every, stop_after (ladder steps; the module's docstring, "Restart"): every checkpoint_every steps, and
    when stop_after steps are done, the batch ends, the four ladder registers are read and the file is replaced; at stop_after the run
    then raises EcmStopped.  Where the file exists when the run begins, stage 1 goes on from it -- after the header has been compared with
    this run's p, B1, scalar, curve form, sigmas and group (CheckpointError, the engine untouched) -- and the result has "resumed_at",
    the step.  A stop_after that the checkpoint is past already is not met again.  A normal end removes the file.  group: the index of
    this group of curves in ecm()'s sequence, kept in the header.
    save (a path): after stage 1 the resume line of the curve (prmers_amd/ecm_files.py) is appended to that file and the result has "x",
    the affine x of the stage-1 point -- unless stage 1 found a factor or the start's inversion failed: then there is no line.  The inverse
    of Z_Q comes from the host, or for inverse="engine" from lanecross.invert.  Refused where the stage-1 scalar holds more than E(B1).
    -> {p, b1, b2, D, sigma, factors, g1, g2, squarings, products, prepares, fused}"""
    return _run_curves(eng, p, b1, b2, [sigma], D, use_fused, use_gmp, False, batch, stage2, inverse,
                       checkpoint, checkpoint_every, stop_after, save, group)[0]


def run_lanes(eng, p, b1, b2, sigmas, D=None, use_fused=True, use_gmp=None, batch=False, stage2="projective", inverse="host",
              checkpoint=None, checkpoint_every=0, stop_after=0, save=None, group=0):
    """len(sigmas) == eng.lanes curves at once on an engine with lanes (Engine(..., lanes=B)), curve l in lane l: the engine calls of ONE
    run(), each of which acts on every lane.  x0 and a24 are written, and the stage-1 Z and the stage-2 accumulator read back, for all lanes
    at once where the engine has set_ints / get_ints (lane by lane otherwise) and gcd'd lane by lane.  stage2 and inverse as for run().  A curve whose inversion fails reports that factor as run() does; its lane carries a valid curve whose
    outcome is dropped.  -> one result per curve in the shape of run(); squarings, products and prepares are those of the batch, which
    are those of one curve.  checkpoint, checkpoint_every, stop_after, save, group as for run(): one checkpoint holds every lane (the
    registers are read with get_ints and written back with set_ints), and every lane that has a line gets it, in lane order."""
    sigmas = list(sigmas)
    if len(sigmas) != getattr(eng, "lanes", 1) or not sigmas:
        raise ValueError("run_lanes needs one sigma per lane: %d given, the engine has %d lanes" % (len(sigmas), getattr(eng, "lanes", 1)))
    return _run_curves(eng, p, b1, b2, sigmas, D, use_fused, use_gmp, True, batch, stage2, inverse,
                       checkpoint, checkpoint_every, stop_after, save, group)


def run_saved(eng, lines, b2, D=None, stage2="projective", inverse="host", batch=False, use_gmp=None):
    """Stage 2 alone, on stage-1 results from resume lines: `lines` are parsed lines (ecm_files.parse_resume_line) of one p and one b1, one
    per lane of `eng` (one line on an engine without lanes).  a24 comes from each sigma, R_XQ <- x, R_ZQ <- 1, then the stage 2 of run().
    The lines' stage 1 ran to E(B1) exactly, so a prime of (B1, B2] that divides D -- there is one only for B1 < 11 -- would be covered
    by nothing: that is refused.  -> one result per line in the shape of run_lanes(), with g1 = 1"""
    lines = list(lines)
    count = getattr(eng, "lanes", 1)
    if len(lines) != count or not lines:
        raise ValueError("run_saved needs one line per lane: %d given, the engine has %d lanes" % (len(lines), count))
    p, b1 = lines[0]["p"], lines[0]["b1"]
    if any((l["p"], l["b1"]) != (p, b1) for l in lines) or p != eng.p:
        raise ValueError("run_saved needs lines of one p, the engine's, and one B1")
    if b2 <= b1:
        raise ValueError("run_saved runs stage 2: B2 must be above the lines' B1 = %d" % b1)
    _check_mode(stage2)
    _check_engine_inverse(eng, inverse, stage2)
    sigmas = [l["sigma"] for l in lines]
    if min(sigmas) < SIGMA_MIN:
        raise ValueError("sigma must be at least %d" % SIGMA_MIN)
    size = {"lanes": count, "inverse": inverse} if inverse != "host" else {}
    D = _wheel(eng, b1, b2, D, stage2, size)
    for q in (2, 3, 5, 7, 11):
        if D % q == 0 and b1 < q <= b2:
            raise ValueError("the lines' stage 1 ran to B1 = %d and stage 2 over D = %d has no residue class for the prime %d" % (b1, D, q))
    mp = (1 << p) - 1
    setup = [suyama(s, mp, use_gmp) for s in sigmas]
    if any(g != 1 for _, _, g in setup):
        raise ValueError("a line names a sigma whose curve cannot be set up modulo 2^%d - 1: no stage 1 can have ended on it" % p)
    ops = _Ops(eng)
    io = _IO(eng, count, count > 1, batch)
    failed, g1, g2 = [False] * count, [1] * count, [1] * count
    io.put(R_A24, [c[1] for c in setup]); ops.prep(R_A24, R_A24)
    io.put(R_XQ, [l["x"] for l in lines]); eng.set(R_ZQ, 1)
    more = _stage2(eng, ops, _Curve(ops), p, b1, b2, D, failed, g1, g2, io.batched, io.get, use_gmp, io.put, stage2, inverse) or {}
    return [{"p": p, "b1": b1, "b2": b2, "D": D, "sigma": sigmas[l], "factors": [f for f in (g2[l],) if 1 < f < mp], "g1": 1, "g2": g2[l],
             "squarings": ops.squarings, "products": ops.products, "prepares": ops.prepares, "fused": ops.fused, **more, **io.launches()}
            for l in range(count)]


def ecm_saved(path, b2, lanes=1, D=None, plan=None, device=0, budget=DEFAULT_BUDGET, onelaunch=False, batch=False, stage2="projective",
              inverse="host"):
    """run_saved() for a file of resume lines: the lines are grouped by (p, B1) and run `lanes` at a time on a fresh prmers_amd.Engine
    with that many lanes; a short last group is padded by repeating its first line and the padding's results are dropped.
    -> {"factors": all of them, "curves": lines run, "results": one per line, each group's in the file's order}"""
    from .engine import Engine, resolve_plan
    _check_mode(stage2)
    _check_inverse(inverse, stage2)
    if lanes < 1:
        raise ValueError("lanes must be at least 1")
    if batch and not (onelaunch or "onelaunch" in (plan or "")):
        raise ValueError("batch needs an engine with one-launch products: say onelaunch=True (--onelaunch) as well")
    if onelaunch:
        plan = (plan + "," if plan else "") + "onelaunch"
    size = {"lanes": lanes, "inverse": inverse} if inverse != "host" else {}
    groups = {}
    for line in ecm_files.read_resume_file(path):
        groups.setdefault((line["p"], line["b1"]), []).append(line)
    out = []
    for (p, b1), lines in groups.items():
        d = D
        if d is None:
            n = int(resolve_plan(p, plan).split("n=")[1].split(":")[0])
            d = choose_D(n, b1, b2, budget // lanes, stage2, **size)
        with Engine(p, registers_needed(d, stage2, **size), device=device, plan=plan, lanes=lanes) as eng:
            for at in range(0, len(lines), lanes):
                part = lines[at:at + lanes]
                res = run_saved(eng, part + [part[0]] * (lanes - len(part)), b2, d, stage2, inverse, batch)
                out.extend(res[:len(part)])
    return {"factors": sorted({f for r in out for f in r["factors"]}), "curves": len(out), "results": out}


def ecm(p, b1, b2=0, sigma=None, curves=1, D=None, plan=None, device=0, budget=DEFAULT_BUDGET, seed=0, lanes=1, onelaunch=False, batch=False,
        curve="montgomery", check_every=0, stage2="projective", inverse="host", checkpoint=None, checkpoint_every=0, stop_after=0, save=None):
    """`curves` curves of run() on a fresh prmers_amd.Engine sized for the chosen D, until one finds a factor.  sigma: the first curve's
    (None: drawn like the others, from random.Random(seed)).  -> the result of the last curve run, with "sigmas": every sigma used.
    lanes = B > 1: the curves run B at a time through run_lanes() on one engine with B lanes (whole batches: `curves` rounded up to a
    multiple of B), sigmas drawn from the same generator in the same order, until a batch in which some lane finds a factor.  -> the
    result of that batch's first curve with a factor (of the last curve run when there is none), "factors": those of all its lanes,
    "sigmas": every sigma of every batch run, "batch": the last batch's results, one per lane.
    onelaunch: the engine is created with the plan token of that name (every product one launch; p <= 204799).
    batch: run() / run_lanes() with batch=True; needs onelaunch (or the token in `plan`) and implies nothing.
    curve: "montgomery" (the ladder of this module) or "edwards": stage 1 in twisted Edwards coordinates with an on-curve check every
    check_every NAF digits and at its end (prmers_amd/ecm_edwards.py: slower per bit, but a wrong result is seen); the results then carry
    that driver's further keys.
    stage2: "projective" or "affine" (run()); D and the engine's registers are chosen for it.
    inverse: "host" or, with stage2="affine", "engine" (run()); the registers are chosen for it too.
    checkpoint, checkpoint_every, stop_after: those of run(), for whichever group of curves is running (a curve, or `lanes` of them); the
    header keeps the group's index.  Where the file exists, the groups before its index are skipped -- they found nothing, or the call
    would have ended -- their sigmas are drawn all the same, and the group's own are compared with the header's: another seed, sigma or
    lane count is refused (CheckpointError).  EcmStopped passes through.  save: run()'s, every group appends its lines."""
    from .engine import Engine, resolve_plan
    _check_mode(stage2)
    _check_inverse(inverse, stage2)
    mode = {} if stage2 == "projective" else {"stage2": stage2}
    size = {}
    if inverse != "host":
        mode["inverse"] = inverse
        size = {"lanes": lanes, "inverse": inverse}
    if curve not in ("montgomery", "edwards"):
        raise ValueError('curve must be "montgomery" or "edwards"')
    if check_every and curve != "edwards":
        raise ValueError("check_every belongs to curve=\"edwards\": a Montgomery ladder has no invariant to check")
    if curve == "edwards":
        from . import ecm_edwards

        def run_one(eng, s, **kw):
            return ecm_edwards.run(eng, p, b1, b2, s, D, check_every=check_every, batch=batch, **mode, **kw)

        def run_many(eng, ss, **kw):
            return ecm_edwards.run_lanes(eng, p, b1, b2, ss, D, check_every=check_every, batch=batch, **mode, **kw)
    else:
        def run_one(eng, s, **kw):
            return run(eng, p, b1, b2, s, D, batch=batch, **mode, **kw)

        def run_many(eng, ss, **kw):
            return run_lanes(eng, p, b1, b2, ss, D, batch=batch, **mode, **kw)
    if lanes < 1:
        raise ValueError("lanes must be at least 1")
    if batch and not (onelaunch or "onelaunch" in (plan or "")):
        raise ValueError("batch needs an engine with one-launch products: say onelaunch=True (--onelaunch) as well")
    if onelaunch:
        plan = (plan + "," if plan else "") + "onelaunch"
    if b2 > b1 and D is None:
        n = int(resolve_plan(p, plan).split("n=")[1].split(":")[0])
        D = choose_D(n, b1, b2, budget // lanes, stage2, **size)
    regs = registers_needed(D, stage2, **size) if b2 > b1 else FIXED_REGISTERS
    rng = random.Random(seed)
    sigmas = []
    res = None

    def draw():
        s = sigma if (not sigmas and sigma is not None) else rng.randrange(SIGMA_MIN, 1 << 32)
        sigmas.append(s)
        return s
    if (checkpoint_every or stop_after) and not checkpoint:
        raise ValueError("checkpoint_every and stop_after need checkpoint=, the file the state goes to")
    keep = {"save": save} if save else {}
    first = 0                                    # the first group to run: the checkpoint's when there is one
    if checkpoint or checkpoint_every or stop_after:
        keep.update(checkpoint=checkpoint, checkpoint_every=checkpoint_every, stop_after=stop_after)
        if checkpoint and os.path.exists(checkpoint):
            first = ecm_files.read_checkpoint(checkpoint)[0]["group"]
            if not 0 <= first < -(-max(1, curves) // lanes):
                raise ecm_files.CheckpointError("%s is the checkpoint of another run: its group %d is none of this call's" % (checkpoint, first))

    def group(c):
        return dict(keep, group=c) if "checkpoint" in keep else keep
    if lanes == 1:
        with Engine(p, regs, device=device, plan=plan) as eng:
            for c in range(max(1, curves)):
                s = draw()
                if c < first:
                    continue
                res = run_one(eng, s, **group(c))
                if res["factors"]:
                    break
    else:
        with Engine(p, regs, device=device, plan=plan, lanes=lanes) as eng:
            for c in range(0, max(1, curves), lanes):
                ss = [draw() for _ in range(lanes)]
                if c // lanes < first:
                    continue
                out = run_many(eng, ss, **group(c // lanes))
                found = [r for r in out if r["factors"]]
                res = dict(found[0] if found else out[-1])
                res["factors"] = sorted({f for r in out for f in r["factors"]})
                res["batch"] = out
                if found:
                    break
    res["sigmas"] = sigmas
    return res


EXIT_STOPPED = 3              # 0: a factor, 1: none, 2: the arguments (argparse), 3: stopped at --stop-after with the checkpoint written


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m prmers_amd.ecm", description="ECM factoring of 2^P - 1 (Montgomery curves, stages 1 and 2) on an MI355X")
    ap.add_argument("p", type=int, nargs="?", default=None)
    ap.add_argument("b1", type=int, nargs="?", default=None)
    ap.add_argument("b2", type=int, nargs="?", default=0)
    ap.add_argument("--sigma", type=int, default=None, help="Suyama parameter of the first curve (default: drawn from the seeded generator)")
    ap.add_argument("--curves", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--D", type=int, choices=D_CHOICES, default=None, help="stage-2 wheel (default: the largest whose register file fits --budget-gib)")
    ap.add_argument("--budget-gib", type=float, default=DEFAULT_BUDGET / 2**30)
    ap.add_argument("--plan", default=None)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--lanes", type=int, default=1, help="curves per batch: an engine with this many lanes runs them in one launch sequence")
    ap.add_argument("--onelaunch", action="store_true", help="plan token onelaunch: every product of the engine is one launch (p <= 204799)")
    ap.add_argument("--batch", action="store_true", help="the ladder and the stage-2 loops as batches, one launch for a run of operations (needs --onelaunch)")
    ap.add_argument("--curve", choices=("montgomery", "edwards"), default="montgomery",
                    help="edwards: stage 1 in twisted Edwards coordinates with an on-curve check and roll-back (slower per bit)")
    ap.add_argument("--check-every", type=int, default=0, help="with --curve edwards: NAF digits between two checks (0: only at the end of stage 1)")
    ap.add_argument("--stage2", choices=STAGE2_MODES, default="projective",
                    help="affine: stage 2 on x-coordinates normalised on the engine, one fused product per pair (small exponents, lane engines)")
    ap.add_argument("--inverse", choices=INVERSE_MODES, default="host",
                    help="with --stage2 affine: engine = the inverses of a block across the lanes on the engine, one host inversion a block")
    ap.add_argument("--save", metavar="FILE", default=None, help="append the resume line of every curve whose stage 1 ended without a factor (GMP-ECM / Prime95 format)")
    ap.add_argument("--checkpoint", metavar="FILE", default=None, help="the stage-1 checkpoint: written there, and stage 1 goes on from it where it exists")
    ap.add_argument("--checkpoint-every", type=int, default=0, metavar="STEPS", help="stage-1 steps between two checkpoints (default: none are written)")
    ap.add_argument("--stop-after", type=int, default=0, metavar="STEPS",
                    help="write the checkpoint when this many stage-1 steps are done and exit with code %d; the same command again goes on from it" % EXIT_STOPPED)
    ap.add_argument("--resume-file", nargs=2, metavar=("FILE", "B2"), default=None,
                    help="in place of P B1: stage 2 to B2 on the stage-1 results of the file's resume lines, --lanes at a time")
    a = ap.parse_args(argv)
    if a.resume_file:
        if a.p is not None:
            ap.error("--resume-file FILE B2 stands in place of P B1 [B2]")
        for name in ("sigma", "save", "checkpoint", "checkpoint_every", "stop_after", "check_every"):
            if getattr(a, name):
                ap.error("--resume-file runs stage 2 only: --%s has nothing to act on" % name.replace("_", "-"))
        try:
            b2 = int(a.resume_file[1])
        except ValueError:
            ap.error("--resume-file FILE B2: B2 must be an integer")
        res = ecm_saved(a.resume_file[0], b2, a.lanes, a.D, a.plan, a.device, int(a.budget_gib * 2**30), a.onelaunch, a.batch, a.stage2, a.inverse)
        print(json.dumps(res))
        return 0 if res["factors"] else 1
    if a.p is None or a.b1 is None:
        ap.error("P and B1 are needed (or --resume-file FILE B2)")
    more = {"batch": True} if a.batch else {}
    if a.curve != "montgomery":
        more["curve"] = a.curve
    if a.check_every:
        more["check_every"] = a.check_every
    if a.stage2 != "projective":
        more["stage2"] = a.stage2
    if a.inverse != "host":
        more["inverse"] = a.inverse
    for name in ("save", "checkpoint", "checkpoint_every", "stop_after"):
        if getattr(a, name):
            more[name] = getattr(a, name)
    try:
        res = ecm(a.p, a.b1, a.b2, a.sigma, a.curves, a.D, a.plan, a.device, int(a.budget_gib * 2**30), a.seed, a.lanes, a.onelaunch, **more)
    except EcmStopped as stop:
        print(json.dumps({"stopped_at": stop.step, "checkpoint": stop.path}))
        return EXIT_STOPPED
    print(json.dumps(res))
    return 0 if res["factors"] else 1


if __name__ == "__main__":
    sys.exit(main())
