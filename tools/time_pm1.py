"""Timing behind DESIGN.md 7b (needs an MI355X); one JSON line.

  python tools/time_pm1.py [P] [REPS] [ROUNDS]     default P = 136279841, 200 steps per batch, 5 rounds

The inner step of P-1 stage 2, A <- A (X - Y), three ways in ONE process, alternating batch by batch so that clock and box drift hit
all three alike:
  mul_sum   Engine.mul_sum(A, img X, img (Mp - Y), tmp): the row sweep adds the two images (one product where the plan allows it)
  addsub    sub_reg of the residues, set_multiplicand of the difference, mul: the step with the operations the engine had before
  two_mul   copy(tmp, A); mul(A, img X); mul(tmp, img N); add(A, tmp): what mul_sum falls back to where the plan has no room
Wall time per step from the host clock around batches that end synchronised; the three results are compared at the end."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from prmers_amd import Engine
    p = int(sys.argv[1]) if len(sys.argv) > 1 else 136279841
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    rng = np.random.default_rng(7)
    A, X, Y, XI, NI, T, D, A2, A3 = range(9)
    with Engine(p, 9) as e:
        def rand(r):
            wc = (p + 31) // 32
            w = np.frombuffer(rng.bytes(wc * 4), dtype="<u4").copy()
            if p % 32:
                w[-1] &= (1 << (p % 32)) - 1
            e.set_words(r, w)
        rand(X); rand(Y)
        for r in (A, A2, A3):
            e.set(r, 3)
        e.set_multiplicand(XI, X)
        e.set(NI, 0); e.sub_reg(NI, Y); e.set_multiplicand(NI, NI)        # the image of Mp - Y

        def mul_sum(a):
            e.mul_sum(a, XI, NI, T)

        def addsub(a):
            e.copy(D, X); e.sub_reg(D, Y); e.set_multiplicand(D, D); e.mul(a, D)

        def two_mul(a):
            e.copy(T, a); e.mul(a, XI); e.mul(T, NI); e.add(a, T)
        paths = (("mul_sum", mul_sum, A), ("addsub", addsub, A2), ("two_mul", two_mul, A3))
        for _, f, a in paths:                                              # code objects, clocks
            for _ in range(10):
                f(a)
        for r in (A, A2, A3):
            e.set(r, 3)
        e.sync()
        ms = {name: [] for name, _, _ in paths}
        for _ in range(rounds):
            for name, f, a in paths:
                e.sync()
                t = time.perf_counter()
                for _ in range(reps):
                    f(a)
                e.sync()
                ms[name].append(round(1e3 * (time.perf_counter() - t) / reps, 4))
        same = e.is_equal(A, A2) and e.is_equal(A, A3)
        print(json.dumps({"p": p, "n": e.n, "plan": e.describe(), "fused": e.mul_sum_is_fused(), "steps_per_batch": reps,
                          "ms_per_step": ms, "results_equal": bool(same)}))
        return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
