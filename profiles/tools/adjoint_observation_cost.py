"""What observations cost the backward sweep: trm_adjoint_backward over 240 taped steps on the checkpointed tape of the default interval
(K = 16), with a misfit observation every 12 steps on four levels (trm_adjoint_observe_misfit) against the sweep of the same run
without observations, on the heat-only workload -- the N145 land mask (56 951 columns) x 32 levels, fp64, NoFlow, Value on the top
temperature (tests/workloads.py, config "heat") -- at the library's default steps per launch.

An observation closes the open segment and the sweep stops at every observed position: 240 steps are 15 segments of 16 without
observations and 20 of 12 with them, plus 20 injection launches of 4 x 56 951 threads each.  Variants:
    plain     this library, no observation: 15 backward launches
    observed  this library, 20 observations: 20 backward launches, 20 injections (and the 20 misfit launches in the record's time)
    parent    the library of the parent commit (--parent-lib, loaded through TRM_LIBRARY), no observation: the yardstick

Timed as profiles/tools/adjoint_checkpoint_cost.py does: wall clock around the synchronous trm_adjoint_backward, after a warm-up of
every call.  Every variant runs in a child process of its own under `timeout`; the order is drawn at random per round, and the median
over the rounds is reported.  One box, one session.

    python profiles/tools/adjoint_observation_cost.py [--rounds 7] [--steps 240] [--every 12] [--parent-lib PATH]
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


def child(variant, steps, every):
    """one variant in this process: (us of the record with its registrations, us of the backward sweep, launches of the sweep)"""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import numpy as np
    import workloads as W
    lat, lon = W.columns_from_mask("N145")
    w = W.make_workload("heat", lat, lon, 32)
    d = W.setup_device(w, steps_per_launch=0)
    d.closure()
    observed = variant == "observed"
    ones = np.ones((w["Nz"], w["Nh"]))
    obs = np.full((len(LEVELS), w["Nh"]), 1.5)
    positions = list(range(every, steps + 1, every)) if observed else []
    stretches = [b - a for a, b in zip([0] + positions, positions + [steps]) if b > a]
    slots = sum(-(-s // K) for s in stretches)
    d.open_adjoint(slots, checkpoint_every=K)

    def record():
        at = 0
        for p in positions:
            d.step_record(w["dt"], p - at)
            d.observe_misfit(LEVELS, obs)
            at = p
        if steps > at:
            d.step_record(w["dt"], steps - at)

    d.step_record(w["dt"], min(50, steps))               # warm-up of every call the timed window makes
    if observed:
        d.observe_misfit(LEVELS, obs)
    d.adjoint_backward()
    t0 = time.perf_counter()
    record()
    t1 = time.perf_counter()
    assert d.adjoint_checkpoints() == (K, slots, slots)
    if observed:
        assert d.adjoint_observations()[0] == len(positions) and np.all(d.misfit() > 0)
    d.set_cotangent("temperature", ones)
    t2 = time.perf_counter()
    d.adjoint_backward()
    t3 = time.perf_counter()
    assert d.status() == 0 and d.last_program()["backward"] and np.any(d.cotangent("internal_energy") != 0.0)
    return 1e6 * (t1 - t0), 1e6 * (t3 - t2), slots + len(positions)


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
    ap.add_argument("--child", choices=("plain", "observed", "parent"), default=None)
    a = ap.parse_args()
    if a.child is not None:
        print(json.dumps(child(a.child, a.steps, a.every)))
        return
    variants = ["plain", "observed"] + (["parent"] if a.parent_lib else [])
    rng = random.Random(20261019)
    t = {v: [] for v in variants}
    for r in range(a.rounds):
        order = list(variants)
        rng.shuffle(order)
        for v in order:
            t[v].append(run_child(v, a.steps, a.every, a.parent_lib))
        print(f"round {r + 1} of {a.rounds}", file=sys.stderr, flush=True)
    rows = {v: dict(us_record=round(statistics.median(x[0] for x in t[v]), 1), us_backward=round(statistics.median(x[1] for x in t[v]), 1),
                    us_backward_min=round(min(x[1] for x in t[v]), 1), us_backward_max=round(max(x[1] for x in t[v]), 1),
                    sweep_launches=int(t[v][0][2])) for v in variants}
    yardstick = rows["parent" if a.parent_lib else "plain"]["us_backward"]
    print(json.dumps(dict(workload="heat N145 x 32 fp64", rounds=a.rounds, steps=a.steps, every=a.every, levels=list(LEVELS), interval=K,
                          rows=rows, observed_over_yardstick=round(rows["observed"]["us_backward"] / yardstick, 4),
                          plain_over_yardstick=round(rows["plain"]["us_backward"] / yardstick, 4))))


if __name__ == "__main__":
    main()
