"""sha256 of the tangents / gradients and TRM_INFO_LAST_PROGRAM of every (ride, tape, layout) of the derivative launches: what a
host-side change of the launch layer must leave bit for bit.  Rides: none, boundary values, thermal parameters, boundary series, and
thermal parameters with a boundary series (derivative_series_params); the tangent, and the adjoint on the per-step tape and on a checkpointed tape of K = 4; Nz = 24 (32 lanes per column) and 40 (64).
Each of them once more with a record attached: the tangent with a tangent record (the T and dT samples), the adjoint on both tapes with a
temperature record (the residuals, the misfit, the gradients).  The records sample position 0, a launch boundary and the last position.
    python profiles/tools/derivative_outputs.py OUTFILE      (library: TRM_LIBRARY, or the tree's)
Run once per library and compare the two files (profiles/r13/derivative_outputs_sha256.txt)."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import workloads as W

lat, lon = W.columns_from_mask("N72")
sel = np.linspace(0, lat.size - 1, 203).astype(int)
TOP = ("temperature", "top")
STEPS, SPL, NODES = 23, 8, 5
POSITIONS = [0, SPL, STEPS]     # the first state, a launch boundary (and a checkpoint of K = 4), the last position
lines = []


def put(combo, name, a):
    lines.append(f"{hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()}  {combo}/{name}")


def prog(combo, what, d):
    lines.append(f"{d.get_option('info_last_program') & 0xffffffff:#010x}  {combo}/last_program_{what}")


def levels_of(Nz):
    return [0, Nz // 2, Nz - 1]


def fresh(Nz, ride):
    w = W.make_workload("heat", lat[sel], lon[sel], Nz)
    d = W.setup_device(w, steps_per_launch=SPL)
    d.closure()
    if ride in ("series", "param_series"):
        kind, value = w["bcs"][TOP]
        times = np.linspace(0.0, STEPS * w["dt"], NODES)
        vals = np.asarray(value, dtype=np.float64)[None, :] + np.linspace(-2.0, 3.0, NODES)[:, None]
        d.set_bc_series(*TOP, kind, times, vals.copy())
        d.set_option("derivative_series", 1)
        if ride == "param_series":
            d.set_option("derivative_series_params", 1)
    return w, d


for Nz in (24, 40):
    for ride in ("none", "bc", "param", "series", "param_series"):
        for record in (False, True):
            rng = np.random.default_rng(7)
            w, d = fresh(Nz, ride)
            Nh = w["Nh"]
            combo = f"tangent{'_record' if record else ''}/{ride}/Nz{Nz}"
            d.open_tangent()
            d.set_tangent("internal_energy", rng.standard_normal((Nz, Nh)))
            if ride in ("bc", "param"):
                d.set_bc_tangent(*TOP, rng.standard_normal(Nh))
            if ride in ("param", "param_series"):
                d.set_param_tangent({"k_water": 1.0, "k_mineral": -0.5, "c_ice": 2.0e3, "c_organic": 1.0e3})
            if ride in ("series", "param_series"):
                d.set_bc_series_tangent(*TOP, rng.standard_normal((NODES, Nh)))
            d.tangent_closure()
            for name in ("temperature", "liquid_water_fraction"):
                put(combo, "closure_" + name, d.tangent(name))
            if record:
                d.attach_tangent_record(POSITIONS, levels_of(Nz))
            d.step_tangent(w["dt"], STEPS)
            prog(combo, "step", d)
            for name in ("internal_energy", "temperature", "liquid_water_fraction"):
                put(combo, name, d.tangent(name))
            put(combo, "state_temperature", d.get("temperature"))
            if record:
                put(combo, "record_temperature", d.tangent_record("temperature"))
                put(combo, "record_tangent", d.tangent_record("tangent"))
            assert d.status() == 0
        for K, record in ((0, False), (4, False), (0, True), (4, True)):
            rng = np.random.default_rng(11)
            w, d = fresh(Nz, ride)
            combo = f"adjoint{'_record' if record else ''}/{ride}/{'step' if K == 0 else 'ckpt'}/Nz{Nz}"
            d.open_adjoint(STEPS if K == 0 else -(-STEPS // K), checkpoint_every=K or None)
            if ride == "bc":
                d.open_bc_gradient()
            if ride in ("param", "param_series"):
                d.open_param_gradient()
            if record:      # (its own generator: the cotangents below are those of the run without a record)
                rrng = np.random.default_rng(13)
                shape = (len(POSITIONS), 3, Nh)
                observed = rrng.normal(0.0, 2.0, shape)
                observed[1, 1, ::7] = np.nan        # gaps
                weight = rrng.uniform(0.5, 2.0, shape)
                weight[2, 0, ::5] = 0.0
                d.attach_record(POSITIONS, levels_of(Nz), observed, weight)
            d.step_record(w["dt"], STEPS)
            prog(combo, "record", d)
            d.set_cotangent("temperature", rng.standard_normal((Nz, Nh)))
            d.set_cotangent("liquid_water_fraction", rng.standard_normal((Nz, Nh)))
            d.set_cotangent("internal_energy", rng.standard_normal((Nz, Nh)))
            d.adjoint_backward()
            prog(combo, "backward", d)
            put(combo, "internal_energy", d.cotangent("internal_energy"))
            if record:
                put(combo, "record_residuals", d.record_residuals())
                put(combo, "record_misfit", d.record_misfit())
            if ride in ("bc", "param"):
                put(combo, "bc_temperature_top", d.bc_gradient(*TOP))
            if ride in ("param", "param_series"):
                for name in ("k_water", "k_mineral", "c_ice", "c_organic"):
                    put(combo, "param_" + name, d.param_gradient(name))
            if ride in ("series", "param_series"):
                put(combo, "series_temperature_top", d.bc_series_gradient(*TOP))
            assert d.status() == 0

os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
open(sys.argv[1], "w").write("\n".join(lines) + "\n")
print(len(lines), "lines")
