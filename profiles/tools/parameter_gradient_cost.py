"""What the derivatives with respect to the thermal parameters cost: trm_adjoint_backward with and without trm_adjoint_param_open on
the per-step tape and on a checkpointed tape of K = 16, and trm_step_tangent with and without parameter seeds (trm_tangent_param_set),
on the workload of profiles/tools/adjoint_checkpoint_cost.py -- the N145 land mask (56 951 columns) x 32 levels, fp64, NoFlow, Value on the
top temperature (tests/workloads.py, config "heat") -- at the library's default steps per launch.

Timed as that tool does: wall clock around one synchronous call over `steps` steps, after a warm-up of the same call.  Every variant
runs in a child process of its own under `timeout`; the order of the variants is drawn at random per round, and the median over the
rounds is reported.  One box, one session.

    python profiles/tools/parameter_gradient_cost.py [--rounds 7] [--steps 200]
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
# (call, checkpoint interval -- 0: the per-step tape, with parameter gradients / seeds)
VARIANTS = [("backward", 0, 0), ("backward", 0, 1), ("backward", 16, 0), ("backward", 16, 1), ("tangent", 0, 0), ("tangent", 0, 1)]


def name_of(v):
    call, K, par = v
    if call == "tangent":
        return "trm_step_tangent" + (", parameter seeds" if par else "")
    return "trm_adjoint_backward, " + ("per-step tape" if K == 0 else f"K={K}") + (", parameter gradients" if par else "")


def child(v, steps):
    """one variant in this process: us per step of the call"""
    call, K, par = v
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import numpy as np
    import workloads as W
    lat, lon = W.columns_from_mask("N145")
    w = W.make_workload("heat", lat, lon, 32)
    d = W.setup_device(w, steps_per_launch=0)
    d.closure()
    ones = np.ones((w["Nz"], w["Nh"]))
    if call == "tangent":
        d.open_tangent()
        d.set_tangent("internal_energy", ones)
        if par:
            d.set_param_tangent({"k_mineral": 1.0, "c_mineral": 1.0})
        d.step_tangent(w["dt"], min(50, steps))          # warm-up: one launch of the default 50 steps
        t0 = time.perf_counter()
        d.step_tangent(w["dt"], steps)
        t1 = time.perf_counter()
        assert d.status() == 0 and d.last_program()["parameter_seeds"] == bool(par)
        return 1e6 * (t1 - t0) / steps
    d.open_adjoint(steps if K == 0 else -(-steps // K), checkpoint_every=K or None)
    if par:
        d.open_param_gradient()
    d.step_record(w["dt"], min(50, steps))               # warm-up: one launch of the default 50 steps each way
    d.adjoint_backward()
    d.step_record(w["dt"], steps)
    d.set_cotangent("temperature", ones)
    t0 = time.perf_counter()
    d.adjoint_backward()
    t1 = time.perf_counter()
    prog = d.last_program()
    assert d.status() == 0 and prog["checkpointed"] == (K > 0) and prog["parameter_gradient"] == bool(par)
    return 1e6 * (t1 - t0) / steps


def run_child(i, steps):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(i), "--steps", str(steps)]
    out = subprocess.run(["timeout", "-k", "10", "120"] + cmd, capture_output=True, text=True, cwd=ROOT)
    if out.returncode != 0:
        raise SystemExit(f"child {cmd} failed ({out.returncode}):\n{out.stderr[-2000:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--child", type=int, choices=range(len(VARIANTS)), default=None)
    a = ap.parse_args()
    if a.child is not None:
        print(json.dumps(child(VARIANTS[a.child], a.steps)))
        return
    rng = random.Random(20261018)
    t = {i: [] for i in range(len(VARIANTS))}
    for r in range(a.rounds):
        order = list(t)
        rng.shuffle(order)
        for i in order:
            t[i].append(run_child(i, a.steps))
        print(f"round {r + 1} of {a.rounds}", file=sys.stderr, flush=True)
    rows = [dict(call=name_of(VARIANTS[i]), us_per_step=round(statistics.median(t[i]), 3), min=round(min(t[i]), 3), max=round(max(t[i]), 3))
            for i in t]
    print(json.dumps(dict(workload="heat N145 x 32 fp64", rounds=a.rounds, steps=a.steps, rows=rows)))


if __name__ == "__main__":
    main()
