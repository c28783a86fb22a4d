"""What thermal-parameter derivatives of a run driven by a boundary time series cost (TRM_OPT_DERIVATIVE_SERIES_PARAMS, the ride
RIDE_PARAM_SERIES): trm_step_tangent, trm_adjoint_backward on the per-step tape and on a checkpointed tape of K = 16, each on three
rides of the same build -- the series ride (node seeds / gradients, TRM_OPT_DERIVATIVE_SERIES), the parameter ride (constant boundary,
parameter seeds / the parameter gradient open) and the new ride with both -- on the workload of series_derivative_cost.py: the N145
land mask (56 951 columns) x 32 levels, fp64, NoFlow, a Value series on the top temperature with `--nodes` nodes spread over the run,
every node holding the workload's constant surface temperature.  With `--parent-library PATH` the series ride of another build of the
library (the parent commit's: its instances are unchanged, so it must be level with this build's) is timed in the same rounds.

Timed as that tool does: wall clock around one synchronous call over `steps` steps at the library's default 50 steps per launch, after
a warm-up of the same call.  Every variant runs in a child process of its own under `timeout`; the order of the variants is drawn at
random per round, and the median over the rounds is reported.  One box, one session.

    python profiles/tools/param_series_cost.py [--rounds 7] [--steps 200] [--nodes 21] [--parent-library PATH]
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
CALLS = [("tangent", 0), ("backward", 0), ("backward", 16)]
# (call, checkpoint interval -- 0: the per-step tape, ride, the other build's library)
VARIANTS = [(call, K, ride, False) for call, K in CALLS for ride in ("series", "params", "both")] + [(call, K, "series", True) for call, K in CALLS]
TOP = ("temperature", "top")


def name_of(v):
    call, K, ride, parent = v
    what = {"series": "series ride", "params": "parameter ride (constant boundary)", "both": "parameters with a series"}[ride]
    head = "trm_step_tangent" if call == "tangent" else "trm_adjoint_backward, " + ("per-step tape" if K == 0 else f"K={K}")
    return head + ", " + what + (", parent build" if parent else "")


def child(v, steps, nodes):
    """one variant in this process: us per step of the call"""
    call, K, ride, _ = v
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import numpy as np
    import workloads as W
    lat, lon = W.columns_from_mask("N145")
    w = W.make_workload("heat", lat, lon, 32)
    d = W.setup_device(w, steps_per_launch=0)
    d.closure()
    warm = min(50, steps)                                # warm-up: one launch of the default 50 steps
    series, with_params = ride != "params", ride != "series"
    if series:
        kind, value = w["bcs"][TOP]
        times = np.linspace(0.0, (steps + warm) * w["dt"], nodes)
        d.set_bc_series(*TOP, kind, times, np.broadcast_to(np.asarray(value, dtype=np.float64), (nodes, w["Nh"])).copy())
        d.set_option("derivative_series", 1)
        if with_params:
            d.set_option("derivative_series_params", 1)
    ones = np.ones((w["Nz"], w["Nh"]))
    seeds = {"k_mineral": 1.0, "c_water": 1.0e5}
    if call == "tangent":
        d.open_tangent()
        d.set_tangent("internal_energy", ones)
        if series:
            d.set_bc_series_tangent(*TOP, np.ones((nodes, w["Nh"])))
        else:
            d.set_bc_tangent(*TOP, 1.0)
        if with_params:
            d.set_param_tangent(seeds)
        d.step_tangent(w["dt"], warm)
        t0 = time.perf_counter()
        d.step_tangent(w["dt"], steps)
        t1 = time.perf_counter()
        prog = d.last_program()
        assert d.status() == 0 and prog["boundary_seeds"] and prog["series"] == series and prog["parameter_seeds"] == with_params
        return 1e6 * (t1 - t0) / steps
    d.open_adjoint(steps if K == 0 else -(-steps // K), checkpoint_every=K or None)
    if with_params:
        d.open_param_gradient()
    else:
        d.open_bc_gradient()
    d.step_record(w["dt"], warm)                         # warm-up each way
    d.adjoint_backward()
    d.step_record(w["dt"], steps)
    d.set_cotangent("temperature", ones)
    t0 = time.perf_counter()
    d.adjoint_backward()
    t1 = time.perf_counter()
    prog = d.last_program()
    assert d.status() == 0 and prog["checkpointed"] == (K > 0) and prog["boundary_gradient"] and prog["series"] == series
    assert prog["parameter_gradient"] == with_params
    return 1e6 * (t1 - t0) / steps


def run_child(i, steps, nodes, parent_library):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(i), "--steps", str(steps), "--nodes", str(nodes)]
    env = dict(os.environ)
    if VARIANTS[i][3]:
        env["TRM_LIBRARY"] = os.path.abspath(parent_library)
    out = subprocess.run(["timeout", "-k", "10", "120"] + cmd, capture_output=True, text=True, cwd=ROOT, env=env)
    if out.returncode != 0:
        raise SystemExit(f"child {cmd} failed ({out.returncode}):\n{out.stderr[-2000:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--nodes", type=int, default=21)
    ap.add_argument("--parent-library", default=None)
    ap.add_argument("--child", type=int, choices=range(len(VARIANTS)), default=None)
    a = ap.parse_args()
    if a.child is not None:
        print(json.dumps(child(VARIANTS[a.child], a.steps, a.nodes)))
        return
    rng = random.Random(20261018)
    t = {i: [] for i, v in enumerate(VARIANTS) if a.parent_library or not v[3]}
    for r in range(a.rounds):
        order = list(t)
        rng.shuffle(order)
        for i in order:
            t[i].append(run_child(i, a.steps, a.nodes, a.parent_library))
        print(f"round {r + 1} of {a.rounds}", file=sys.stderr, flush=True)
    rows = [dict(call=name_of(VARIANTS[i]), us_per_step=round(statistics.median(t[i]), 3), min=round(min(t[i]), 3), max=round(max(t[i]), 3))
            for i in t]
    print(json.dumps(dict(workload="heat N145 x 32 fp64", rounds=a.rounds, steps=a.steps, nodes=a.nodes, rows=rows)))


if __name__ == "__main__":
    main()
