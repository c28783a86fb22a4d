"""What the hydraulic-parameter gradients cost the heat + Richards backward sweep: trm_adjoint_backward with the parameter gradients open
(TRM_OPT_DERIVATIVE_RICHARDS_PARAMS, k_column_adjoint_rich_params and the reduction launch that ends the sweep) against the same call
without them (k_column_adjoint_rich), both on this library, on the benchmarked model -- the N145 land mask (56 951 columns) x 32 levels,
fp64, heat + Richards, Value on the top temperature (tests/workloads.py, config "richards") -- at the library's default steps per
launch.  The commit before the parameter gradients measured 24.5 us per taped step for the sweep without them
(profiles/tools/adjoint_richards_cost.py, DESIGN 4.8 "Richards"); the figure is printed beside the two for comparison, not measured here.

Both legs are timed the same way: wall clock around one synchronous trm_adjoint_backward over a tape of `steps` recorded steps, after a
warm-up sweep; the cotangents are dense in all five fields.  Every timed region runs in a child process of its own under `timeout`; the
order of the two legs is drawn at random per round, and the median over the rounds is reported.

    python profiles/tools/adjoint_richards_params_cost.py [--rounds 7] [--steps 100]
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
LEGS = ("backward", "backward_params")
PARENT_US_PER_STEP_BACKWARD = 24.5


def child(leg, steps):
    """one timed region in this process: us per taped step"""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import numpy as np
    import workloads as W
    lat, lon = W.columns_from_mask("N145")
    w = W.make_workload("richards", lat, lon, 32)
    d = W.setup_device(w, steps_per_launch=0)
    d.save_state()
    shape = (w["Nz"], w["Nh"])
    d.set_option("derivative_richards_adjoint", 1)
    if leg == "backward_params":
        d.set_option("derivative_richards_params", 1)

    def arm(n):
        d.open_adjoint(max(steps, 50))
        if leg == "backward_params":
            d.open_param_gradient()
        d.step_record(w["dt"], n)
        for name, scale in (("internal_energy", 1e-6), ("saturation", 1.0), ("temperature", 1e-1), ("liquid_water_fraction", 1.0), ("pressure_head", 1e-2)):
            d.set_cotangent(name, np.full(shape, scale))
        d.synchronize()
    arm(50)                                             # warm-up: one record launch and one sweep of the default 50 steps
    d.adjoint_backward()
    # (the timed steps start from the initial state again, and stay inside the 150 steps bench.py trusts)
    d.restore_state()
    arm(steps)
    t0 = time.perf_counter()
    d.adjoint_backward()
    d.synchronize()
    t1 = time.perf_counter()
    assert d.status() == 0
    assert bool(d.last_program().get("hydraulic_parameter_gradient")) == (leg == "backward_params")
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
    print(json.dumps(dict(workload="heat + Richards N145 x 32 fp64", us_per_step_backward=round(us["backward"], 3),
                          us_per_step_backward_params=round(us["backward_params"], 3), params_ratio=round(us["backward_params"] / us["backward"], 3),
                          us_per_step_backward_parent_commit=PARENT_US_PER_STEP_BACKWARD, rounds=a.rounds, steps=a.steps)))


if __name__ == "__main__":
    main()
