"""Whether two libraries give the same bits on the heat + Richards backward sweep: this tree's against the parent commit's
(--parent-lib, loaded through TRM_LIBRARY as the cost tools do).  With -ffp-contract=off -fno-fast-math a kernel whose floating-point
statements stand in the same order gives the same bits whatever its schedule, so the required result is zero differing bits: a condition,
not a tolerance.

Cases: those of tests/richards_cases.py at Nz in {3, 32, 33, 64} x 13 columns -- the three hydraulics, both boundary sets -- six steps of
60 s in launches of 4 and 2 (steps_per_launch = 4), under a dense final cotangent on all five fields.  Sweeps: trm_adjoint_backward alone,
with the hydraulic-parameter gradients, with a soil-moisture record, with both.  The record: positions (0, 3, 5, 6) -- 0 and n among
them, 3 and 5 inside a launch -- on tests/richards_cases.one_hot_levels, the observations the initial saturation moved by 0.03 ... 0.12,
weights in 0.5 ... 2, one sample a gap (NaN).  Compared byte for byte: gU, gsat, the seven parameter gradients, the residuals and the
misfit.  Every (library, sweep) runs in a child process of its own under `timeout`.

    python profiles/tools/adjoint_richards_parity.py --parent-lib build/parent/libterrarium_hip.so [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SWEEPS = ("plain", "params", "record", "params+record")
SIZES = (3, 32, 33, 64)
POSITIONS = (0, 3, 5, 6)
BY_FIELD = (("internal_energy", 1e-6), ("saturation", 1.0), ("temperature", 1e-1), ("liquid_water_fraction", 1.0), ("pressure_head", 1e-2))


def child(sweep, out):
    """every case under one sweep in this process: the result arrays into the .npz `out`"""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import numpy as np
    import richards_cases as RC
    import terrarium_jl_amd as trm
    params, record = "params" in sweep, "record" in sweep
    assert RC.STEPS == POSITIONS[-1]
    arrays = {}
    for case in RC.CASES:
        Nz, Nh, hyd, bcset = case
        if Nz not in SIZES or Nh != RC.NH or bcset == "repair":
            continue
        p, U0, sat, bcs, _ = RC.inputs(case)
        d = trm.DeviceState(trm.ColumnGrid(trm.PrescribedSpacing(dz=[RC.DZ] * Nz), Nh), p)
        d.set_option("steps_per_launch", RC.SPL)
        d.set_option("derivative_richards_adjoint", 1)
        d.set_option("derivative_richards_params", 1 if params else 0)
        d.set_option("derivative_richards_record", 1 if record else 0)
        d.set("saturation_water_ice", sat)
        d.set("internal_energy", U0)
        for (var, side), (kind, value) in bcs.items():
            d.set_bc(var, side, kind, value)
        d.closure()
        d.open_adjoint(RC.STEPS)
        d.step_record(RC.DT, RC.STEPS)
        if record:
            levels = RC.one_hot_levels(Nz)
            rng = np.random.default_rng(30 + Nz)
            shape = (len(POSITIONS), len(levels), Nh)
            observed = sat[levels][None] + rng.choice([-1.0, 1.0], shape) * rng.uniform(0.03, 0.12, shape)
            observed[1, 0, 0] = np.nan
            d.attach_record(list(POSITIONS), levels, observed, rng.uniform(0.5, 2.0, shape))
        if params:
            d.open_param_gradient()
        rng = np.random.default_rng(3000 + Nz)
        for name, scale in BY_FIELD:
            d.set_cotangent(name, rng.normal(0.0, scale, (Nz, Nh)))
        d.adjoint_backward()
        assert bool(d.last_program().get("hydraulic_parameter_gradient")) == params
        key = RC.case_id(case)
        arrays[f"{key}/gU"], arrays[f"{key}/gsat"] = d.cotangent("internal_energy"), d.cotangent("saturation")
        assert np.any(arrays[f"{key}/gsat"] != 0.0)
        if params:
            arrays[f"{key}/params"] = np.stack([d.param_gradient(name) for name in trm._capi.HYDRAULIC_PARAMS])
        if record:
            arrays[f"{key}/residuals"], arrays[f"{key}/misfit"] = d.record_residuals(), d.record_misfit()
            assert float(arrays[f"{key}/misfit"].min()) > 0.0
    np.savez(out, **{k: np.ascontiguousarray(v, dtype=np.float64) for k, v in arrays.items()})


def run_child(sweep, library, out):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", sweep, "--out", out]
    env = dict(os.environ)
    if library:
        env["TRM_LIBRARY"] = os.path.abspath(library)
    done = subprocess.run(["timeout", "-k", "10", "120"] + cmd, capture_output=True, text=True, cwd=ROOT, env=env)
    if done.returncode != 0:
        raise SystemExit(f"child {cmd} failed ({done.returncode}):\n{done.stderr[-2000:]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libterrarium_hip.so of the parent commit")
    ap.add_argument("--out", default=None, help="the JSON result (of a child: its .npz)")
    ap.add_argument("--child", choices=SWEEPS, default=None)
    a = ap.parse_args()
    if a.child is not None:
        child(a.child, a.out)
        return
    if not a.parent_lib:
        raise SystemExit("--parent-lib is required")
    import numpy as np
    result = dict(cases=f"Nz {list(SIZES)} x 13 columns, three hydraulics, both boundary sets; six steps in launches of 4 and 2", sweeps={})
    differing = 0
    with tempfile.TemporaryDirectory() as tmp:
        for sweep in SWEEPS:
            files = {}
            for who, library in (("this", None), ("parent", a.parent_lib)):
                files[who] = os.path.join(tmp, f"{who}_{sweep}.npz")
                run_child(sweep, library, files[who])
            this, parent = np.load(files["this"]), np.load(files["parent"])
            assert sorted(this.files) == sorted(parent.files) and this.files
            per = {}
            for key in this.files:
                what = key.split("/")[1]
                x, y = this[key].view(np.uint64), parent[key].view(np.uint64)
                assert x.shape == y.shape and x.size
                entry = per.setdefault(what, dict(arrays=0, values=0, differing_bits=0))
                entry["arrays"] += 1
                entry["values"] += int(x.size)
                entry["differing_bits"] += int(np.unpackbits((x ^ y).view(np.uint8)).sum())
            result["sweeps"][sweep] = per
            differing += sum(e["differing_bits"] for e in per.values())
    result["differing_bits"] = differing
    text = json.dumps(result)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if differing:
        raise SystemExit("the libraries differ: a floating-point statement of the sweep changed its place")


if __name__ == "__main__":
    main()
