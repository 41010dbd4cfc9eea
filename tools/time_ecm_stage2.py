"""Timing behind DESIGN.md 7c and 7e (needs an MI355X); one JSON line.

  python tools/time_ecm_stage2.py [P] [LANES] [B1] [B2] [ROUNDS]     default 1277, 512 lanes, B1 = 50, B2 = 5000, 5 rounds

ECM stage 2 alone (prmers_amd/ecm.py _stage2) three ways in ONE process, alternating round by round on the same engine and the same stage-1
points, at D = 210 and at D = 30 (few baby points, many giant points: the unfavourable end for the normalisation):
  projective     A <- A (X_k Z_j - X_j Z_k): three products and a set_multiplicand per pair (11 sweeps by count)
  affine         points normalised on the engine (20 sweeps a point, one host inversion per lane and block), one mul_sum per pair (3 sweeps)
  affine_engine  the same with inverse="engine": a block's inverses across the lanes on the engine (prmers_amd/lanecross.py: 2 ceil(log2 B)
                 products by a sibling lane's image, one lane read, one host inversion, one broadcast write) and the Z product in a register
The engine has one-launch products and both run batched.  Wall time of a whole stage 2 from the host clock; it ends in the read of the
accumulator, which synchronises, and it includes the host's inversions and gcds, which are part of the price.  Then the write of one
value per lane two ways, Engine.set_ints against the loop over set_int(lane=l), the same way.  No threshold: the numbers go into
DESIGN.md."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


MODES = {"projective": ("projective", "host"), "affine": ("affine", "host"), "affine_engine": ("affine", "engine")}


def stage2(e, ecm, p, b1, b2, D, way, lanes):
    """one stage 2 on the stage-1 point the engine holds -> (ms, g2 per lane, the keys the mode adds, products, prepares)"""
    mode, inverse = MODES[way]
    failed, g1, g2 = [False] * lanes, [1] * lanes, [1] * lanes
    ops = ecm._Ops(e)
    io = ecm._IO(e, lanes, True, True)
    e.sync()
    t = time.perf_counter()
    more = ecm._stage2(e, ops, ecm._Curve(ops), p, b1, b2, D, failed, g1, g2, io.batched, io.get, None, io.put, mode, inverse)
    ms = 1e3 * (time.perf_counter() - t)
    return ms, g2, more or {}, ops.products, ops.prepares, io.launches().get("launches")


def median(v):
    return sorted(v)[len(v) // 2]


def measure(e, p, lanes, b1, b2, rounds, reps=20):
    from prmers_amd import ecm
    from prmers_amd.pm1 import stage2_pairs
    mp = (1 << p) - 1
    sigmas = list(range(ecm.SIGMA_MIN, ecm.SIGMA_MIN + lanes))
    ecm.run_lanes(e, p, b1, 0, sigmas, batch=True)           # the stage-1 points, and a24 as an image: stage 2 leaves both alone
    out = {"p": p, "n": e.n, "lanes": lanes, "b1": b1, "b2": b2, "rounds": rounds, "stage2": {}}
    for D in (210, 30):
        for mode in MODES:                                   # code objects, clocks, the lane-wise scratch
            stage2(e, ecm, p, b1, b2, D, mode, lanes)
        ms = {mode: [] for mode in MODES}
        last = {}
        for _ in range(rounds):
            for mode in MODES:
                r = stage2(e, ecm, p, b1, b2, D, mode, lanes)
                ms[mode].append(round(r[0], 3))
                last[mode] = r
        pairs = stage2_pairs(b1, b2, D)
        same = all(a % b == 0 for a, b in zip(last["affine"][1], last["projective"][1])) and last["affine_engine"][1] == last["affine"][1]
        out["stage2"]["D=%d" % D] = {
            "pairs": sum(len(js) for js in pairs.values()), "pairs_k0": len(pairs.get(0, ())), "ms": ms,
            "median_ms": {m: median(v) for m, v in ms.items()},
            "median_ratio_affine_over_projective": round(median(ms["affine"]) / median(ms["projective"]), 4),
            "median_ratio_affine_engine_over_projective": round(median(ms["affine_engine"]) / median(ms["projective"]), 4),
            "median_ratio_affine_engine_over_affine": round(median(ms["affine_engine"]) / median(ms["affine"]), 4),
            "affine_engine": last["affine_engine"][2],
            "products": {m: last[m][3] for m in ms}, "prepares": {m: last[m][4] for m in ms}, "launches": {m: last[m][5] for m in ms},
            "affine": last["affine"][2], "affine_g2_is_a_multiple_of_projective_g2": bool(same),
            "lanes_with_a_factor": sum(1 for g in last["affine"][1] if 1 < g < mp)}
    # the write of one value per lane
    vals = [pow(3, l + 2, mp) for l in range(lanes)]
    reg = ecm.R_T
    ways = {"set_ints": lambda: e.set_ints(reg, vals), "per_lane": lambda: [e.set_int(reg, v, lane=l) for l, v in enumerate(vals)]}
    e.set(reg, 0)
    for f in ways.values():
        f()
    wms = {k: [] for k in ways}
    ok = True
    for _ in range(rounds):
        for k, f in ways.items():
            e.sync()
            t = time.perf_counter()
            for _ in range(reps):
                f()
            e.sync()
            wms[k].append(round(1e3 * (time.perf_counter() - t) / reps, 4))
            ok = ok and e.get_ints(reg) == vals
    out["write"] = {"ms_per_write": wms, "median_ms": {k: median(v) for k, v in wms.items()}, "values_read_back": bool(ok),
                    "median_ratio_set_ints_over_per_lane": round(median(wms["set_ints"]) / median(wms["per_lane"]), 5)}
    return out


def main():
    from prmers_amd import Engine, ecm
    arg = [int(a) for a in sys.argv[1:]] + [None] * 5
    p, lanes, b1, b2, rounds = (a if a is not None else d for a, d in zip(arg, (1277, 512, 50, 5000, 5)))
    with Engine(p, ecm.registers_needed(210, "affine", lanes, "engine"), lanes=lanes, onelaunch=True) as e:
        out = measure(e, p, lanes, b1, b2, rounds)
        out["plan"] = e.describe()
    print(json.dumps(out))
    return 0 if out["write"]["values_read_back"] and all(d["affine_g2_is_a_multiple_of_projective_g2"] for d in out["stage2"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
