"""What the heat + Richards reverse mode costs a step: trm_step_record and trm_adjoint_backward (TRM_OPT_DERIVATIVE_RICHARDS_ADJOINT,
k_column_record_rich / k_column_adjoint_rich) against trm_step (finalize = 1) on the resident multi-step program, with trm_step_tangent
(k_column_tangent_rich) for scale, on the benchmarked model -- the N145 land mask (56 951 columns) x 32 levels, fp64, heat + Richards,
Value on the top temperature (tests/workloads.py, config "richards") -- at the library's default steps per launch.  A tape slot is two
fields, 29.2 MB at this size: the tape of the timed steps is allocated once, outside the timed region.  The cotangents are dense in all
five fields, the seeds dense in the internal energy and in the saturation.

All four legs are timed the same way: wall clock around one synchronous call over `steps` steps, after a warm-up (backward: around the
sweep over a tape of `steps` recorded steps).  Every timed region runs in a child process of its own under `timeout`; the order of the
four legs is drawn at random per round (as profiles/tools/tangent_richards_cost.py does), and the median over the rounds is reported.

    python profiles/tools/adjoint_richards_cost.py [--rounds 7] [--steps 100]
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
    w = W.make_workload("richards", lat, lon, 32)
    d = W.setup_device(w, steps_per_launch=0)
    d.save_state()
    shape = (w["Nz"], w["Nh"])

    def arm():
        if leg == "tangent":
            d.set_tangent("internal_energy", np.ones(shape))
            d.set_tangent("saturation", np.full(shape, 1e-3))
        if leg in ("record", "backward"):
            d.open_adjoint(max(steps, 50))
    if leg == "tangent":
        d.set_option("derivative_richards", 1)
        d.open_tangent()
    if leg in ("record", "backward"):
        d.set_option("derivative_richards_adjoint", 1)
    arm()
    run = {"step": lambda n: d.step(w["dt"], n, finalize=True), "tangent": lambda n: d.step_tangent(w["dt"], n),
           "record": lambda n: d.step_record(w["dt"], n), "backward": lambda n: d.step_record(w["dt"], n)}[leg]
    run(50)                                             # warm-up: one launch of the default 50 steps
    if leg == "backward":
        d.adjoint_backward()
    # (the explicit Richards scheme at dt = 60 s dries the top cells of this workload out within 250 steps: the timed steps start from
    #  the initial state again, and stay inside the 150 steps bench.py trusts)
    d.restore_state()
    arm()
    if leg == "backward":
        d.step_record(w["dt"], steps)
        for name, scale in (("internal_energy", 1e-6), ("saturation", 1.0), ("temperature", 1e-1), ("liquid_water_fraction", 1.0), ("pressure_head", 1e-2)):
            d.set_cotangent(name, np.full(shape, scale))
        d.synchronize()
        run = lambda n: d.adjoint_backward()             # noqa: E731
    t0 = time.perf_counter()
    run(steps)
    d.synchronize()
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
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--child", choices=LEGS, default=None)
    a = ap.parse_args()
    if a.child is not None:
        print(child(a.child, a.steps))
        return
    rng = random.Random(20261021)
    t = {leg: [] for leg in LEGS}
    for _ in range(a.rounds):
        order = list(LEGS)
        rng.shuffle(order)
        for leg in order:
            t[leg].append(run_child(leg, a.steps))
    us = {leg: statistics.median(t[leg]) for leg in LEGS}
    print(json.dumps(dict(workload="heat + Richards N145 x 32 fp64", us_per_step_primal=round(us["step"], 3), us_per_step_record=round(us["record"], 3),
                          us_per_step_backward=round(us["backward"], 3), us_per_step_tangent=round(us["tangent"], 3),
                          record_ratio=round(us["record"] / us["step"], 3), backward_ratio=round(us["backward"] / us["step"], 3),
                          rounds=a.rounds, steps=a.steps)))


if __name__ == "__main__":
    main()
