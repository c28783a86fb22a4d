"""What open time averages cost a step: run! (trm_step, finalize = 0) on C3 -- the N145 land mask (56 951 columns) x 32 levels,
fp64, Richards -- with and without averages of temperature, saturation and liquid fraction, on the resident multi-step program
(the library's default steps per launch) and on the per-step path (steps per launch 1).

Every timed region runs in a child process of its own under `timeout`; the order of the two legs of a pair is drawn at random
per round (as profiles/tools/ab_libs.sh does), and the median over the rounds is reported.

    python profiles/tools/average_cost.py [--rounds 10] [--steps 100]
"""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FIELDS = ("temperature", "saturation_water_ice", "liquid_water_fraction")


def child(spl, averaged, steps):
    """one timed region in this process: us per step"""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import workloads as W
    lat, lon = W.columns_from_mask("N145")
    w = W.make_workload("richards", lat, lon, 32)
    d = W.setup_device(w, steps_per_launch=spl)
    if averaged:
        for f in FIELDS:
            d.open_average(f)
    d.step(w["dt"], 10, finalize=False)        # warm-up (bench.py's)
    ms = d.step_timed(w["dt"], steps, finalize=False)
    if averaged:
        assert d.average(0)[2] == 10 + steps
    return 1000.0 * ms / steps


def run_child(spl, averaged, steps):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(spl), str(int(averaged)), "--steps", str(steps)]
    out = subprocess.run(["timeout", "-k", "10", "120"] + cmd, capture_output=True, text=True, cwd=ROOT)
    if out.returncode != 0:
        raise SystemExit(f"child {cmd} failed ({out.returncode}):\n{out.stderr[-2000:]}")
    return float(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--child", nargs=2, default=None)
    a = ap.parse_args()
    if a.child:
        print(child(int(a.child[0]), bool(int(a.child[1])), a.steps))
        return
    rng = random.Random(20261015)
    result = {}
    for spl, label in ((0, "resident_program"), (1, "per_step")):
        t = {False: [], True: []}
        for _ in range(a.rounds):
            order = [False, True]
            rng.shuffle(order)
            for averaged in order:
                t[averaged].append(run_child(spl, averaged, a.steps))
        base, avg = statistics.median(t[False]), statistics.median(t[True])
        result[label] = dict(us_per_step_plain=round(base, 3), us_per_step_averaged=round(avg, 3),
                             overhead_pct=round(100.0 * (avg / base - 1.0), 1), rounds=a.rounds, steps=a.steps)
    print(json.dumps(dict(workload="C3 N145 x 32 fp64 Richards", averaged=list(FIELDS), **result)))


if __name__ == "__main__":
    main()
