"""What the reverse-mode gradient costs a step: trm_step_record and trm_adjoint_backward against trm_step (finalize = 1) on the resident
multi-step program, and for scale trm_step_tangent, on the heat-only workload -- the N145 land mask (56 951 columns) x 32 levels,
fp64, NoFlow, Value on the top temperature (tests/workloads.py, config "heat") -- at the library's default steps per launch.  The tape
of `steps` steps is steps x 14.6 MB.

Every leg is timed the same way: wall clock around one synchronous call over `steps` steps, after a warm-up.  Every timed region runs
in a child process of its own under `timeout`; the order of the legs is drawn at random per round (as profiles/tools/tangent_cost.py
does), and the median over the rounds is reported.  One box, one session.

    python profiles/tools/adjoint_cost.py [--rounds 7] [--steps 200]
"""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LEGS = ("step", "record", "backward", "tangent")


def child(leg, steps):
    """one timed region in this process: us per step"""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import numpy as np
    import workloads as W
    lat, lon = W.columns_from_mask("N145")
    w = W.make_workload("heat", lat, lon, 32)
    d = W.setup_device(w, steps_per_launch=0)
    d.closure()
    ones = np.ones((w["Nz"], w["Nh"]))
    if leg == "tangent":
        d.open_tangent()
        d.set_tangent("internal_energy", ones)
        run = lambda n: d.step_tangent(w["dt"], n)      # noqa: E731
    elif leg == "step":
        run = lambda n: d.step(w["dt"], n, finalize=True)      # noqa: E731
    else:
        d.open_adjoint(steps)
        run = lambda n: d.step_record(w["dt"], n)       # noqa: E731
    if leg in ("record", "backward"):                   # warm-up: one launch of the default 50 steps each way
        run(50)
        d.adjoint_backward()
    else:
        run(50)
    if leg == "backward":
        run(steps)
        d.set_cotangent("temperature", ones)
        t0 = time.perf_counter()
        d.adjoint_backward()
        t1 = time.perf_counter()
    else:
        t0 = time.perf_counter()
        run(steps)
        t1 = time.perf_counter()
    assert d.status() == 0
    return 1e6 * (t1 - t0) / steps


def run_child(leg, steps):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", leg, "--steps", str(steps)]
    out = subprocess.run(["timeout", "-k", "10", "120"] + cmd, capture_output=True, text=True, cwd=ROOT)
    if out.returncode != 0:
        raise SystemExit(f"child {cmd} failed ({out.returncode}):\n{out.stderr[-2000:]}")
    return float(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--child", choices=LEGS, default=None)
    a = ap.parse_args()
    if a.child is not None:
        print(child(a.child, a.steps))
        return
    rng = random.Random(20261016)
    t = {leg: [] for leg in LEGS}
    for _ in range(a.rounds):
        order = list(LEGS)
        rng.shuffle(order)
        for leg in order:
            t[leg].append(run_child(leg, a.steps))
    med = {leg: statistics.median(t[leg]) for leg in LEGS}
    print(json.dumps(dict(workload="heat N145 x 32 fp64", rounds=a.rounds, steps=a.steps,
                          **{f"us_per_step_{leg}": round(med[leg], 3) for leg in LEGS},
                          **{f"ratio_{leg}": round(med[leg] / med["step"], 3) for leg in LEGS[1:]})))


if __name__ == "__main__":
    main()
