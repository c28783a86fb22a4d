"""What a checkpointed tape costs the reverse-mode gradient: trm_step_record and trm_adjoint_backward on the per-step tape and on
checkpointed tapes of interval K in {1, 4, 8, 16, 32}, with the bytes of tape each needs, on the heat-only workload -- the N145 land
mask (56 951 columns) x 32 levels, fp64, NoFlow, Value on the top temperature (tests/workloads.py, config "heat") -- at the library's
default steps per launch.  One slot is 14.6 MB; the per-step tape of `steps` steps has `steps` of them, a checkpointed one
ceil(steps / K).

Timed as profiles/tools/adjoint_cost.py does: wall clock around one synchronous call over `steps` steps, after a warm-up of both
calls.  Every tape runs in a child process of its own under `timeout` (its record, then its backward sweep); the order of the tapes is
drawn at random per round, and the median over the rounds is reported.  One box, one session.

    python profiles/tools/adjoint_checkpoint_cost.py [--rounds 7] [--steps 200]
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
TAPES = (0, 1, 4, 8, 16, 32)      # 0: the per-step tape


def slots(K, steps):
    return steps if K == 0 else -(-steps // K)


def child(K, steps):
    """one tape in this process: (us per step of the record, us per step of the backward sweep, bytes of tape)"""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import numpy as np
    import workloads as W
    lat, lon = W.columns_from_mask("N145")
    w = W.make_workload("heat", lat, lon, 32)
    d = W.setup_device(w, steps_per_launch=0)
    d.closure()
    ones = np.ones((w["Nz"], w["Nh"]))
    d.open_adjoint(slots(K, steps), checkpoint_every=K or None)
    d.step_record(w["dt"], min(50, steps))              # warm-up: one launch of the default 50 steps each way
    d.adjoint_backward()
    t0 = time.perf_counter()
    d.step_record(w["dt"], steps)
    t1 = time.perf_counter()
    assert d.adjoint_checkpoints() == (K, slots(K, steps), slots(K, steps))
    d.set_cotangent("temperature", ones)
    t2 = time.perf_counter()
    d.adjoint_backward()
    t3 = time.perf_counter()
    assert d.status() == 0 and d.last_program()["checkpointed"] == (K > 0)
    return 1e6 * (t1 - t0) / steps, 1e6 * (t3 - t2) / steps, slots(K, steps) * w["Nh"] * w["Nz"] * 8      # (32 levels: no padding)


def run_child(K, steps):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(K), "--steps", str(steps)]
    out = subprocess.run(["timeout", "-k", "10", "120"] + cmd, capture_output=True, text=True, cwd=ROOT)
    if out.returncode != 0:
        raise SystemExit(f"child {cmd} failed ({out.returncode}):\n{out.stderr[-2000:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--child", type=int, choices=TAPES, default=None)
    a = ap.parse_args()
    if a.child is not None:
        print(json.dumps(child(a.child, a.steps)))
        return
    rng = random.Random(20261017)
    t = {K: [] for K in TAPES}
    for r in range(a.rounds):
        order = list(TAPES)
        rng.shuffle(order)
        for K in order:
            t[K].append(run_child(K, a.steps))
        print(f"round {r + 1} of {a.rounds}", file=sys.stderr, flush=True)
    rows = []
    for K in TAPES:
        rows.append(dict(tape="per-step" if K == 0 else f"K={K}", tape_bytes=int(t[K][0][2]),
                         us_per_step_record=round(statistics.median(x[0] for x in t[K]), 3),
                         us_per_step_backward=round(statistics.median(x[1] for x in t[K]), 3)))
    print(json.dumps(dict(workload="heat N145 x 32 fp64", rounds=a.rounds, steps=a.steps, rows=rows)))


if __name__ == "__main__":
    main()
