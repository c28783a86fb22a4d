"""What the heat + Richards forward-mode tangent costs a step: trm_step_tangent (TRM_OPT_DERIVATIVE_RICHARDS, k_column_tangent_rich)
against trm_step (finalize = 1) on the resident multi-step program, on the benchmarked model -- the N145 land mask (56 951 columns) x 32
levels, fp64, heat + Richards, Value on the top temperature (tests/workloads.py, config "richards") -- at the library's default steps per
launch.  The seeds are dense in the internal energy and in the saturation.

Both legs are timed the same way: wall clock around one synchronous call of `steps` steps, after a warm-up.  Every timed region runs
in a child process of its own under `timeout`; the order of the two legs of a pair is drawn at random per round (as
profiles/tools/average_cost.py does), and the median over the rounds is reported.

    python profiles/tools/tangent_richards_cost.py [--rounds 7] [--steps 100]
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


def child(tangent, steps):
    """one timed region in this process: us per step"""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import numpy as np
    import workloads as W
    lat, lon = W.columns_from_mask("N145")
    w = W.make_workload("richards", lat, lon, 32)
    d = W.setup_device(w, steps_per_launch=0)
    d.save_state()

    def seed():
        d.set_tangent("internal_energy", np.ones((w["Nz"], w["Nh"])))
        d.set_tangent("saturation", np.full((w["Nz"], w["Nh"]), 1e-3))
    if tangent:
        d.set_option("derivative_richards", 1)
        d.open_tangent()
        seed()
        run = lambda n: d.step_tangent(w["dt"], n)      # noqa: E731
    else:
        run = lambda n: d.step(w["dt"], n, finalize=True)      # noqa: E731
    run(50)                                             # warm-up: one launch of the default 50 steps
    # (the explicit Richards scheme at dt = 60 s dries the top cells of this workload out within 250 steps: the timed steps start from
    #  the initial state again, and stay inside the 150 steps bench.py trusts)
    d.restore_state()
    if tangent:
        seed()
    t0 = time.perf_counter()
    run(steps)
    t1 = time.perf_counter()
    assert d.status() == 0
    return 1e6 * (t1 - t0) / steps


def run_child(tangent, steps):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(int(tangent)), "--steps", str(steps)]
    out = subprocess.run(["timeout", "-k", "10", "120"] + cmd, capture_output=True, text=True, cwd=ROOT)
    if out.returncode != 0:
        raise SystemExit(f"child {cmd} failed ({out.returncode}):\n{out.stderr[-2000:]}")
    return float(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--child", type=int, default=None)
    a = ap.parse_args()
    if a.child is not None:
        print(child(bool(a.child), a.steps))
        return
    rng = random.Random(20261020)
    t = {False: [], True: []}
    for _ in range(a.rounds):
        order = [False, True]
        rng.shuffle(order)
        for tangent in order:
            t[tangent].append(run_child(tangent, a.steps))
    base, tan = statistics.median(t[False]), statistics.median(t[True])
    print(json.dumps(dict(workload="heat + Richards N145 x 32 fp64", us_per_step_primal=round(base, 3), us_per_step_tangent=round(tan, 3),
                          ratio=round(tan / base, 3), rounds=a.rounds, steps=a.steps)))


if __name__ == "__main__":
    main()
