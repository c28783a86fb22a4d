"""What a temperature record costs the backward sweep when it is attached (trm_adjoint_observe_record) and not registered position by
position (trm_adjoint_observe_misfit): trm_adjoint_backward over 240 taped steps on the checkpointed tape of the default interval
(K = 16) on the heat-only workload -- the N145 land mask (56 951 columns) x 32 levels, fp64, NoFlow, Value on the top temperature
(tests/workloads.py, config "heat") -- at the library's default steps per launch, with a sample every `--every` steps (12, and 1: a
sample at every step) on four levels.  Variants:
    parent           the library of the parent commit (--parent-lib, loaded through TRM_LIBRARY), no observation: the yardstick
    null             this library, no record: its spread against `parent` is the noise floor
    per_position     this library, trm_adjoint_observe_misfit at every sample: a launch boundary, an injection and a slot per position
    attached_host    this library, the record attached once from host arrays, outside the timed window
    attached_device  this library, the record attached once from device arrays (no copy)
The record side (trm_step_record and whatever is registered on the way) and the sweep are timed apart, wall clock around the
synchronous calls after a warm-up of every call, as profiles/tools/adjoint_observation_cost.py does; the slots the tape used ride
along.  Every variant runs in a child process of its own under `timeout`; the order is drawn at random per round; median of the rounds
with the range.  One box, one session.

    python profiles/tools/adjoint_record_cost.py [--rounds 7] [--steps 240] [--every 12] [--parent-lib PATH]
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
LEVELS = (16, 24, 28, 31)         # rows of the host layout: four sensors in the upper half of the 32 levels
K = 16                            # TRM_ADJOINT_DEFAULT_INTERVAL
VARIANTS = ("parent", "null", "per_position", "attached_host", "attached_device")


def child(variant, steps, every):
    """one variant in this process: (us of the record side, us of the backward sweep, slots used)"""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import numpy as np
    import workloads as W
    lat, lon = W.columns_from_mask("N145")
    w = W.make_workload("heat", lat, lon, 32)
    d = W.setup_device(w, steps_per_launch=0)
    d.closure()
    ones = np.ones((w["Nz"], w["Nh"]))
    positions = list(range(every, steps + 1, every))
    per_position, attached = variant == "per_position", variant.startswith("attached")
    obs = np.full((len(LEVELS), w["Nh"]), 1.5)
    if per_position:
        stretches = [b - a for a, b in zip([0] + positions, positions + [steps]) if b > a]
        slots = sum(-(-s // K) for s in stretches)
    else:
        slots = -(-steps // K)
    d.open_adjoint(slots, checkpoint_every=K)
    if attached:
        full = np.full((len(positions), len(LEVELS), w["Nh"]), 1.5)
        if variant == "attached_device":
            import torch
            full = torch.as_tensor(full, device=torch.device("cuda", int(d.grid.device)))
            torch.cuda.synchronize()
        d.attach_record(positions, LEVELS, full)

    def record():
        at = 0
        if per_position:
            for p in positions:
                d.step_record(w["dt"], p - at)
                d.observe_misfit(LEVELS, obs)
                at = p
        if steps > at:
            d.step_record(w["dt"], steps - at)

    record()                                              # warm-up of every call the timed window makes, on the tape of the run itself
    d.adjoint_backward()
    t0 = time.perf_counter()
    record()
    t1 = time.perf_counter()
    used = d.adjoint_checkpoints()[1]
    assert used == slots
    if per_position:
        assert d.adjoint_observations()[0] == len(positions) and np.all(d.misfit() > 0)
    d.set_cotangent("temperature", ones)
    t2 = time.perf_counter()
    d.adjoint_backward()
    t3 = time.perf_counter()
    assert d.status() == 0 and d.last_program()["backward"] and np.any(d.cotangent("internal_energy") != 0.0)
    if attached:
        assert np.all(d.record_misfit() > 0) and d.adjoint_observations() == (0, 0)
    return 1e6 * (t1 - t0), 1e6 * (t3 - t2), used


def run_child(variant, steps, every, parent_lib):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", variant, "--steps", str(steps), "--every", str(every)]
    env = dict(os.environ)
    if variant == "parent":
        env["TRM_LIBRARY"] = os.path.abspath(parent_lib)
    out = subprocess.run(["timeout", "-k", "10", "120"] + cmd, capture_output=True, text=True, cwd=ROOT, env=env)
    if out.returncode != 0:
        raise SystemExit(f"child {cmd} failed ({out.returncode}):\n{out.stderr[-2000:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=240)
    ap.add_argument("--every", type=int, default=12)
    ap.add_argument("--parent-lib", default=None, help="libterrarium_hip.so built from the parent commit")
    ap.add_argument("--child", choices=VARIANTS, default=None)
    a = ap.parse_args()
    if a.child is not None:
        print(json.dumps(child(a.child, a.steps, a.every)))
        return
    variants = [v for v in VARIANTS if v != "parent" or a.parent_lib]
    rng = random.Random(20261019)
    t = {v: [] for v in variants}
    for r in range(a.rounds):
        order = list(variants)
        rng.shuffle(order)
        for v in order:
            t[v].append(run_child(v, a.steps, a.every, a.parent_lib))
        print(f"round {r + 1} of {a.rounds}", file=sys.stderr, flush=True)

    def stats(xs):
        return dict(median=round(statistics.median(xs), 1), min=round(min(xs), 1), max=round(max(xs), 1))

    rows = {v: dict(us_record=stats([x[0] for x in t[v]]), us_backward=stats([x[1] for x in t[v]]), slots=int(t[v][0][2])) for v in variants}
    yardstick = rows["parent" if a.parent_lib else "null"]["us_backward"]["median"]
    print(json.dumps(dict(workload="heat N145 x 32 fp64", rounds=a.rounds, steps=a.steps, every=a.every, levels=list(LEVELS), interval=K, rows=rows,
                          over_yardstick={v: round(rows[v]["us_backward"]["median"] / yardstick, 4) for v in variants})))


if __name__ == "__main__":
    main()
