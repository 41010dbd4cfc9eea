"""Timing behind DESIGN.md 7c (needs an MI355X); one JSON line.

  python tools/time_ecm.py [P] [REPS] [ROUNDS]     default P = 136279841, 50 ladder steps per batch, 5 rounds

One Montgomery ladder step of ECM stage 1 (prmers_amd/ecm.py ladder_step: one doubling and one differential addition) two ways in ONE
process, alternating batch by batch so that clock and box drift hit both alike:
  fused     s^2 and d^2 through Engine.square_mul_prepare, which keeps the images of s and d (34 sweeps by count)
  composed  set_multiplicand + square_mul for each of them (38 sweeps)
Both walk the same ladder from the same curve on register sets of their own.  Wall time per step from the host clock around batches that
end synchronised; the two points are compared at the end.  No threshold: the numbers go into DESIGN.md."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class _Shift:
    """an engine seen through a register offset: two independent register sets on one engine"""

    def __init__(self, eng, base, fused):
        self._e, self._b, self._fused = eng, base, fused
        self.p, self.n = eng.p, eng.n

    def _call(self, name, regs, *rest):
        return getattr(self._e, name)(*[r + self._b for r in regs], *rest)

    def set(self, d, a): self._call("set", (d,), a)
    def set_int(self, d, v): self._call("set_int", (d,), v)
    def copy(self, d, s): self._call("copy", (d, s))
    def add(self, d, s): self._call("add", (d, s))
    def sub_reg(self, d, s): self._call("sub_reg", (d, s))
    def addsub(self, s, d, a, b): self._call("addsub", (s, d, a, b))
    def square_mul(self, r, a=1): self._call("square_mul", (r,), a)
    def set_multiplicand(self, d, s): self._call("set_multiplicand", (d, s))
    def mul(self, d, s, a=1): self._call("mul", (d, s), a)
    def square_mul_prepare(self, s, i, a=1): self._call("square_mul_prepare", (s, i), a)
    def square_mul_prepare_is_fused(self): return self._e.square_mul_prepare_is_fused()


def main():
    from prmers_amd import Engine, ecm
    p = int(sys.argv[1]) if len(sys.argv) > 1 else 136279841
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    R = ecm.FIXED_REGISTERS
    a, b = (ecm.R_XA, ecm.R_ZA), (ecm.R_XB, ecm.R_ZB)
    with Engine(p, 2 * R) as e:
        curves = {}
        for name, base, fused in (("fused", 0, True), ("composed", R, False)):
            v = _Shift(e, base, fused)
            ops = ecm._Ops(v, fused)
            cv = ecm._Curve(ops)
            # any curve serves a timing: small values in place of Suyama's (which would cost an inversion modulo 2^p - 1)
            v.set(ecm.R_A24, 12345); v.set_multiplicand(ecm.R_A24, ecm.R_A24)
            v.set(ecm.R_X0, 7); v.set_multiplicand(ecm.R_X0, ecm.R_X0)
            v.set(ecm.R_XA, 7); v.set(ecm.R_ZA, 1)
            cv.dbl(b, a)
            curves[name] = cv
        for cv in curves.values():                                         # code objects, clocks
            for i in range(6):
                cv.ladder_step(a, b) if i & 1 else cv.ladder_step(b, a)
        e.sync()
        ms = {name: [] for name in curves}
        for _ in range(rounds):
            for name, cv in curves.items():
                e.sync()
                t = time.perf_counter()
                for i in range(reps):
                    cv.ladder_step(a, b) if i & 1 else cv.ladder_step(b, a)
                e.sync()
                ms[name].append(round(1e3 * (time.perf_counter() - t) / reps, 4))
        same = all(e.is_equal(r, r + R) for r in a + b)
        med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
        print(json.dumps({"p": p, "n": e.n, "plan": e.describe(), "fused": e.square_mul_prepare_is_fused(), "steps_per_batch": reps,
                          "ms_per_step": ms, "median_ratio_fused_over_composed": round(med["fused"] / med["composed"], 4),
                          "results_equal": bool(same)}))
        return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
