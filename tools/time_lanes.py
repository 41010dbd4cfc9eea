"""Ladder throughput of engines with lanes (needs an MI355X); one JSON line per lane count.

  python tools/time_lanes.py P B1 [--lanes 1,8,64,512] [--rounds 3] [--plan SPEC] [--batch] [--baseline-lib PATH] [--curve montgomery|edwards]

The metric is Montgomery-ladder steps per second, summed over lanes: the stage-1 ladder of ECM with bound B1 (ecm._Curve.ladder_step
over the bits of ecm.stage1_exponent(B1)) on an engine with B lanes does B curves' steps per call.  The baseline is a plain Engine --
from the library at --baseline-lib (a build of the parent commit, loaded through MI355_ENGINE_LIB) when given, else from this build.
Every measurement is a fresh child process (one engine, warm-up, timed ladders, host clock between two syncs); the rounds alternate
baseline, B1, B2, ... so that every lane count is measured next to the baseline in time.  The figure reported per lane count is the
median over the rounds, and its ratio to the baseline's median.  --batch (with --plan onelaunch): every timed ladder runs inside
Engine.batch(), a run of register operations per launch (include/mi355_batch.h); the baseline stays what it is.
--curve edwards: the timed walk is ecm_edwards' stage 1 instead, a doubling per digit of the NAF of the same exponent and an addition on
its non-zero digits (no checks inside the timed part); a step is then a NAF digit, which is a bit of the exponent as a ladder step is.
Every child with lanes then also times one on-curve check: the two sides (sides_ms), their comparison through Engine.equal_lanes
(equal_lanes_ms) and the same comparison lane by lane through get_int (get_int_ms), each the median of five."""
import argparse
import contextlib
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child_edwards(p, b1, lanes, plan, min_seconds, batch):
    from prmers_amd import Engine, ecm, ecm_edwards as ed
    import prmers_amd
    import statistics as st
    digits = ed.naf(ecm.stage1_exponent(b1))[1:]
    rng = random.Random(5)
    with Engine(p, ed.FIXED_REGISTERS, plan=plan, lanes=lanes) as e:
        ops = ecm._Ops(e)
        cv = ed._Edwards(ops)
        for r in range(ed.R_IZ):
            e.set_int(r, rng.getrandbits(p))            # every lane: the work does not depend on the data
        for r in range(ed.R_IA, ed.R_IZ):
            ops.prep(r, r)

        def walk():
            with (e.batch() if batch else contextlib.nullcontext()):
                for d in digits:
                    cv.dbl()
                    if d:
                        cv.add(d)
        walk(); e.sync()
        steps, t0 = 0, time.perf_counter()
        while True:
            walk(); e.sync()
            steps += len(digits)
            dt = time.perf_counter() - t0
            if dt >= min_seconds:
                break
        more = {}
        if e.lanes > 1:
            def timed(f):
                ts = []
                for _ in range(5):
                    e.sync(); t = time.perf_counter(); f(); e.sync(); ts.append((time.perf_counter() - t) * 1e3)
                return round(st.median(ts), 3)
            cv.sides(); e.equal_lanes(ed.R_L, ed.R_R)       # scratch, code objects
            more = {"sides_ms": timed(cv.sides), "equal_lanes_ms": timed(lambda: e.equal_lanes(ed.R_L, ed.R_R)),
                    "get_int_ms": timed(lambda: [e.get_int(ed.R_L, lane=l) == e.get_int(ed.R_R, lane=l) for l in range(e.lanes)])}
        print(json.dumps({"p": p, "b1": b1, "lanes": lanes, "curve": "edwards", "plan": e.describe(), "fused": ops.fused,
                          "steps_per_ladder": len(digits), "additions_per_ladder": sum(1 for d in digits if d),
                          "steps": steps, "seconds": round(dt, 4), "lane_steps_per_s": round(steps * lanes / dt, 1),
                          "lib": prmers_amd.LIB_PATH, **more, **({"batch": True, "launches": e.batch_stats()[1]} if batch else {})}))


def child(p, b1, lanes, plan, min_seconds, batch=False, curve="montgomery"):
    if curve == "edwards":
        return child_edwards(p, b1, lanes, plan, min_seconds, batch)
    from prmers_amd import Engine, ecm
    import prmers_amd
    bits = ecm.stage1_exponent(b1).bit_length() - 1
    rng = random.Random(5)
    with Engine(p, ecm.FIXED_REGISTERS, plan=plan, lanes=lanes) as e:
        ops = ecm._Ops(e)
        cv = ecm._Curve(ops)
        for r in (ecm.R_A24, ecm.R_X0, ecm.R_XA, ecm.R_ZA, ecm.R_XB, ecm.R_ZB):
            e.set_int(r, rng.getrandbits(p))            # every lane: the ladder's work does not depend on the data
        ops.prep(ecm.R_A24, ecm.R_A24); ops.prep(ecm.R_X0, ecm.R_X0)
        a, b = (ecm.R_XA, ecm.R_ZA), (ecm.R_XB, ecm.R_ZB)

        def steps_of_a_ladder():
            for i in range(bits):
                if i & 1:
                    cv.ladder_step(b, a)
                else:
                    cv.ladder_step(a, b)

        def ladder():
            if batch:
                with e.batch():
                    steps_of_a_ladder()
            else:
                steps_of_a_ladder()
        ladder(); e.sync()                                # code objects, clocks
        steps, t0 = 0, time.perf_counter()
        while True:
            ladder(); e.sync()
            steps += bits
            dt = time.perf_counter() - t0
            if dt >= min_seconds:
                break
        print(json.dumps({"p": p, "b1": b1, "lanes": lanes, "plan": e.describe(), "fused": ops.fused, "steps_per_ladder": bits,
                          "steps": steps, "seconds": round(dt, 4), "lane_steps_per_s": round(steps * lanes / dt, 1),
                          "lib": prmers_amd.LIB_PATH, **({"batch": True, "launches": e.batch_stats()[1]} if batch else {})}))


def measure(p, b1, lanes, plan, min_seconds, lib, batch=False, curve="montgomery"):
    env = dict(os.environ)
    env.pop("MI355_ENGINE_LIB", None)
    if lib:
        env["MI355_ENGINE_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), str(p), str(b1), "--child", str(lanes), "--min-seconds", str(min_seconds)]
    if plan:
        cmd += ["--plan", plan]
    if batch:
        cmd += ["--batch"]
    if curve != "montgomery":
        cmd += ["--curve", curve]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        return {"lanes": lanes, "error": (out.stderr.strip().splitlines() or ["exit %d" % out.returncode])[-1]}
    return json.loads(out.stdout.strip().splitlines()[-1])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("p", type=int)
    ap.add_argument("b1", type=int)
    ap.add_argument("--lanes", default="1,8,64,512")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--plan", default=None)
    ap.add_argument("--baseline-lib", default=None, help="libmi355_engine.so of the parent commit (default: this build, without lanes)")
    ap.add_argument("--batch", action="store_true", help="the timed ladders run inside Engine.batch() (needs --plan onelaunch); never the baseline")
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--curve", choices=("montgomery", "edwards"), default="montgomery", help="edwards: the NAF walk of ecm_edwards, baseline included")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.child is not None:
        child(a.p, a.b1, a.child, a.plan, a.min_seconds, a.batch, a.curve)
        return 0
    lane_counts = [int(x) for x in a.lanes.split(",")]
    runs = {"baseline": []}
    runs.update({b: [] for b in lane_counts})
    for _ in range(a.rounds):
        for key, b, lib in [("baseline", 1, a.baseline_lib)] + [(b, b, None) for b in lane_counts]:
            runs[key].append(measure(a.p, a.b1, b, a.plan, a.min_seconds, lib, a.batch and key != "baseline", a.curve))
            if "error" in runs[key][-1]:                 # a fault or a refusal ends the session: nothing more is started on the device
                print(json.dumps(runs[key][-1]))
                return 1
    base = statistics.median(r["lane_steps_per_s"] for r in runs["baseline"])
    print(json.dumps({"p": a.p, "b1": a.b1, "lanes": "baseline", "plan": runs["baseline"][0]["plan"], "lib": runs["baseline"][0]["lib"],
                      "lane_steps_per_s": base, "all": [r["lane_steps_per_s"] for r in runs["baseline"]]}))
    for b in lane_counts:
        med = statistics.median(r["lane_steps_per_s"] for r in runs[b])
        check = {k: statistics.median(r[k] for r in runs[b]) for k in ("sides_ms", "equal_lanes_ms", "get_int_ms") if k in runs[b][0]}
        print(json.dumps({"p": a.p, "b1": a.b1, "lanes": b, "plan": runs[b][0]["plan"], "lane_steps_per_s": med,
                          "ratio_to_baseline": round(med / base, 2), "all": [r["lane_steps_per_s"] for r in runs[b]],
                          **({"curve": a.curve} if a.curve != "montgomery" else {}), **check}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
