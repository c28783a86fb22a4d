"""What sampling T and dT at the positions of a temperature record costs a tangent run when the record is attached
(trm_tangent_record_attach) and not read the old way, one trm_step_tangent and a full-field download per position: trm_step_tangent over
240 steps on the heat-only workload -- the N145 land mask (56 951 columns) x 32 levels, fp64, NoFlow, Value on the top temperature
(tests/workloads.py, config "heat") -- at the library's default steps per launch, with a sample every `--every` steps (12, and 1: a sample
at every step) on four levels.  Variants:
    parent           the library of the parent commit (--parent-lib, loaded through TRM_LIBRARY), no record: the yardstick
    null             this library, no record: the kernels are the parent's, so its spread against `parent` is the noise floor
    attached         this library, the record attached once outside the timed window; the timed window is one trm_step_tangent and the
                     two downloads of the samples
    per_position     this library, no record: per position one trm_step_tangent to it and the downloads of T and dT (the whole fields)
Two figures per variant: the trm_step_tangent calls alone, and the whole window with the downloads that bring T and dT at the positions
to the host (the attached record's two sample arrays; per position two whole fields).  Wall clock around the synchronous calls after a
warm-up of every call; every variant runs in a child process of its own under
`timeout`; the order is drawn at random per round; median of the rounds with the range.  One box, one session.  With --example the
synthetic record of examples/borehole_calibration_gauss_newton.py (one record_jvp) is timed against that of
examples/borehole_calibration_dense.py (240 trm.run(steps=1) calls and downloads) as well.

    python profiles/tools/tangent_record_cost.py [--rounds 7] [--steps 240] [--every 12] [--parent-lib PATH] [--example]
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
VARIANTS = ("parent", "null", "attached", "per_position")


def child(variant, steps, every):
    """one variant in this process: (us of the trm_step_tangent calls, us with the downloads of T and dT at the positions as well)"""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import numpy as np
    import workloads as W
    lat, lon = W.columns_from_mask("N145")
    w = W.make_workload("heat", lat, lon, 32)
    d = W.setup_device(w, steps_per_launch=0)
    d.closure()
    d.save_state()
    positions = list(range(every, steps + 1, every))
    dU = np.ones((w["Nz"], w["Nh"]))
    d.open_tangent()
    if variant == "attached":
        d.attach_tangent_record(positions, LEVELS)

    def run():
        d.restore_state()
        d.set_tangent("internal_energy", dU)
        if variant == "attached":
            d.rewind_tangent_record()
        t0 = time.perf_counter()
        out, stepping = None, 0.0
        if variant == "per_position":
            at, out = 0, []
            for p in positions + ([steps] if steps > positions[-1] else []):
                t1 = time.perf_counter()
                d.step_tangent(w["dt"], p - at)
                stepping += time.perf_counter() - t1
                at = p
                if p in positions:
                    out.append((d.get("temperature")[list(LEVELS)], d.tangent("temperature")[list(LEVELS)]))
        else:
            d.step_tangent(w["dt"], steps)
            stepping = time.perf_counter() - t0
            if variant == "attached":
                out = d.tangent_record("temperature"), d.tangent_record("tangent")
        return (1e6 * stepping, 1e6 * (time.perf_counter() - t0)), out

    run()                                                  # warm-up of every call the timed window makes
    us, out = run()
    assert d.status() == 0 and d.last_program()["family"] == "column_tangent"
    if variant == "attached":
        assert not np.any(np.isnan(out[0])) and np.any(out[1] != 0.0) and d.tangent_record_info()[2] == steps
    return us


def example_child(which):
    """us of the synthetic record of an example: `gauss_newton` (one record_jvp) or `dense` (240 run(steps=1) calls and downloads)"""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "examples")]
    import importlib
    ex = importlib.import_module("borehole_calibration_" + which)
    ex.synthetic_record()                                  # warm-up
    t0 = time.perf_counter()
    ex.synthetic_record()
    return 1e6 * (time.perf_counter() - t0)


def run_child(args, parent_lib=None):
    cmd = [sys.executable, os.path.abspath(__file__)] + args
    env = dict(os.environ)
    if parent_lib:
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
    ap.add_argument("--example", action="store_true", help="also time the synthetic records of the two calibration examples")
    ap.add_argument("--child", choices=VARIANTS, default=None)
    ap.add_argument("--example-child", choices=("gauss_newton", "dense"), default=None)
    a = ap.parse_args()
    if a.child is not None:
        print(json.dumps(child(a.child, a.steps, a.every)))
        return
    if a.example_child is not None:
        print(json.dumps(example_child(a.example_child)))
        return
    variants = [v for v in VARIANTS if v != "parent" or a.parent_lib]
    examples = ["gauss_newton", "dense"] if a.example else []
    rng = random.Random(20261020)
    t = {v: [] for v in variants + examples}
    for r in range(a.rounds):
        order = variants + examples
        rng.shuffle(order)
        for v in order:
            if v in examples:
                t[v].append(run_child(["--example-child", v]))
            else:
                t[v].append(run_child(["--child", v, "--steps", str(a.steps), "--every", str(a.every)], a.parent_lib if v == "parent" else None))
        print(f"round {r + 1} of {a.rounds}", file=sys.stderr, flush=True)

    def stats(xs):
        return dict(median=round(statistics.median(xs), 1), min=round(min(xs), 1), max=round(max(xs), 1))

    rows = {v: dict(us_step=stats([x[0] for x in t[v]]), us_with_downloads=stats([x[1] for x in t[v]])) for v in variants}
    yardstick = rows["parent" if a.parent_lib else "null"]["us_step"]["median"]
    out = dict(workload="heat N145 x 32 fp64", rounds=a.rounds, steps=a.steps, every=a.every, levels=list(LEVELS), rows=rows,
               step_over_yardstick={v: round(rows[v]["us_step"]["median"] / yardstick, 4) for v in variants},
               with_downloads_over_yardstick={v: round(rows[v]["us_with_downloads"]["median"] / yardstick, 4) for v in variants})
    if examples:
        out["example_record_us"] = {v: stats(t[v]) for v in examples}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
