"""What an attached soil-moisture record costs the heat + Richards backward sweep (TRM_OPT_DERIVATIVE_RICHARDS_RECORD,
k_column_adjoint_rich_record / k_column_adjoint_rich_params_record), in the method of adjoint_richards_params_cost.py: trm_adjoint_backward
on the benchmarked model -- the N145 land mask (56 951 columns) x 32 levels, fp64, heat + Richards, Value on the top temperature
(tests/workloads.py, config "richards") -- at the library's default steps per launch, over a tape of 100 recorded steps.

Legs, each without and with the hydraulic-parameter gradients open (TRM_OPT_DERIVATIVE_RICHARDS_PARAMS), and each on this library and,
as `parent/...`, on the parent commit's (--parent-lib: a libterrarium_hip.so built from it, which must know the record option):
    none      no record attached
    sparse    a record with a sample every 12 steps (positions 0, 12, ..., 96) on four levels
    dense     a record with a sample at every step (positions 0 ... 100) on four levels
A record's observations are the initial saturation moved by 0.05, its weights 1.  Every timed region -- wall clock around one synchronous
trm_adjoint_backward after a warm-up sweep, the cotangents dense in all five fields -- runs in a child process of its own under
`timeout`; the order of the legs is drawn at random per round; the median over the rounds is reported with the range.  With a parent
library every leg gets a verdict, `within_noise`: this library's median is no more than the parent leg's own range (max - min) of the
same run above the parent's median; the tool fails if one is not.

    python profiles/tools/adjoint_richards_record_cost.py --parent-lib build/parent/libterrarium_hip.so [--rounds 7] [--steps 100] [--out FILE]
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
RECORDS = ("none", "sparse", "dense")
PARENT = "parent/"
OWN_LEGS = tuple(f"{record}{suffix}" for suffix in ("", "+params") for record in RECORDS)
LEGS = OWN_LEGS + tuple(PARENT + leg for leg in OWN_LEGS)
LEVELS = (0, 10, 21, 31)


def positions(record, steps):
    return list(range(0, steps + 1, 12)) if record == "sparse" else list(range(steps + 1))


def child(leg, steps):
    """one timed region in this process: us per taped step"""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import numpy as np
    import workloads as W
    leg = leg[len(PARENT):] if leg.startswith(PARENT) else leg          # (the library is the parent's through TRM_LIBRARY)
    record, params = leg.split("+")[0], leg.endswith("+params")
    lat, lon = W.columns_from_mask("N145")
    w = W.make_workload("richards", lat, lon, 32)
    d = W.setup_device(w, steps_per_launch=0)
    d.save_state()
    shape = (w["Nz"], w["Nh"])
    d.set_option("derivative_richards_adjoint", 1)
    if params:
        d.set_option("derivative_richards_params", 1)
    if record in ("sparse", "dense"):
        d.set_option("derivative_richards_record", 1)
        pos = positions(record, steps)
        observed = np.broadcast_to(d.get("saturation_water_ice")[list(LEVELS)] + 0.05, (len(pos), len(LEVELS), w["Nh"]))

    def arm(n, attach):
        d.open_adjoint(max(steps, 50))
        if params:
            d.open_param_gradient()
        if attach:
            d.attach_record(pos, LEVELS, observed)
        d.step_record(w["dt"], n)
        for name, scale in (("internal_energy", 1e-6), ("saturation", 1.0), ("temperature", 1e-1), ("liquid_water_fraction", 1.0), ("pressure_head", 1e-2)):
            d.set_cotangent(name, np.full(shape, scale))
        d.synchronize()
    attach = record in ("sparse", "dense")
    arm(steps, attach)                                  # warm-up: the record launches and one sweep of the timed shape
    d.adjoint_backward()
    # (the timed steps start from the initial state again, and stay inside the 150 steps bench.py trusts)
    d.restore_state()
    arm(steps, attach)
    t0 = time.perf_counter()
    d.adjoint_backward()
    d.synchronize()
    t1 = time.perf_counter()
    assert d.status() == 0
    assert bool(d.last_program().get("hydraulic_parameter_gradient")) == params
    if attach:
        assert d.record_info()[:2] == (len(pos), len(LEVELS)) and float(d.record_misfit().min()) > 0.0
    return 1e6 * (t1 - t0) / steps


def run_child(leg, steps, parent_lib):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", leg, "--steps", str(steps)]
    env = dict(os.environ)
    if leg.startswith(PARENT):
        env["TRM_LIBRARY"] = os.path.abspath(parent_lib)
    out = subprocess.run(["timeout", "-k", "10", "120"] + cmd, capture_output=True, text=True, cwd=ROOT, env=env)
    if out.returncode != 0:
        raise SystemExit(f"child {cmd} failed ({out.returncode}):\n{out.stderr[-2000:]}")
    return float(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--parent-lib", default=None, help="libterrarium_hip.so of the parent commit; without it the parent legs are left out")
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    ap.add_argument("--child", choices=LEGS, default=None)
    a = ap.parse_args()
    if a.child is not None:
        print(child(a.child, a.steps))
        return
    legs = [leg for leg in LEGS if a.parent_lib or not leg.startswith(PARENT)]
    rng = random.Random(20261021)
    t = {leg: [] for leg in legs}
    for done in range(a.rounds):
        order = list(legs)
        rng.shuffle(order)
        for leg in order:
            t[leg].append(run_child(leg, a.steps, a.parent_lib))
        print(f"round {done + 1} of {a.rounds}", file=sys.stderr, flush=True)
    result = dict(workload="heat + Richards N145 x 32 fp64", rounds=a.rounds, steps=a.steps, levels=list(LEVELS), unit="us per taped step",
                  legs={leg: dict(median=round(statistics.median(t[leg]), 3), min=round(min(t[leg]), 3), max=round(max(t[leg]), 3)) for leg in legs})
    if a.parent_lib:
        for leg in OWN_LEGS:
            own, parent = t[leg], t[PARENT + leg]
            result["legs"][leg]["within_noise"] = statistics.median(own) <= statistics.median(parent) + (max(parent) - min(parent))
    text = json.dumps(result)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    slower = [leg for leg in OWN_LEGS if a.parent_lib and not result["legs"][leg]["within_noise"]]
    if slower:
        raise SystemExit(f"slower than the parent's library by more than the parent's own range: {slower}")


if __name__ == "__main__":
    main()
