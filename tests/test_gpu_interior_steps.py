"""TRM_OPT_INTERIOR_STEPS: inside one trm_step call the fp64 heat + Richards launches but the last store internal_energy, saturation,
surface_excess_water and the water table alone (k_column_psi<PSI_INTERIOR>), and the launch behind one derives the pressure head at
entry.  Nothing a caller can observe may change: every check here is byte identity against a context with the option off -- every
compared field, the status word, the clock, TRM_INFO_LAST_PROGRAM -- plus TRM_INFO_INTERIOR_LAUNCHES, which must be what the host rule
predicts (Ops::step): a launch goes interior if it is not the call's last, derives T / liq and defers their stores, and the stored
pressure_head / water_table are a step launch's.

The deriving instance is forced at test sizes with derive_closure_fields = 1.  A context's first step after trm_initialize reads T / liq
as stored, so a fresh context's call of n steps has max(0, n - 2) interior launches, a later call n - 1.

Shapes, the smallest at which the lane mapping can go wrong: 5 columns (odd: the last wave's second column is a clamped copy) and 67
(nine workgroups, the last partial); 32 levels, 30 (idle lanes) and 40 (64 lanes per column, one column per wave)."""
import os
import subprocess
import sys

import numpy as np
import pytest

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:      # (the child process of the staged case runs this file as a script)
    sys.path.insert(0, _ROOT)

import terrarium_jl_amd as trm
import workloads as W

pytestmark = pytest.mark.gpu

SHAPES = [(5, 32), (5, 30), (5, 40), (67, 32), (67, 30), (67, 40)]


def _workload(hydraulics="default", ncol=67, Nz=32, config="richards", dtype=np.float64):
    lat, lon = W.columns_from_mask("N72")
    sel = np.linspace(0, lat.size - 1, ncol).astype(int)
    return W.make_workload(config, lat[sel], lon[sel], Nz, dtype=dtype, hydraulics=hydraulics)


def _device(w, interior, derive=1, **options):
    d = W.setup_device(w)
    d.set_option("derive_closure_fields", derive)
    d.set_option("interior_steps", interior)
    for k, v in options.items():
        d.set_option(k, v)
    return d


def _pair(w, **options):
    """(context with the option off, context with it on), identical otherwise"""
    return _device(w, 0, **options), _device(w, 1, **options)


def count(d): return d.get_option("info_interior_launches")


def _same(w, off, on):
    assert on.status() == off.status()
    assert on.clock() == off.clock()
    assert on.last_program() == off.last_program()
    for name in W.compared_fields(w):
        x, y = off.get(name), on.get(name)
        assert x.tobytes() == y.tobytes(), name
    assert count(off) == 0


# ---- 1. call lengths ---------------------------------------------------------------------------------------------------------------
def _call_lengths(ncol, Nz, hydraulics, n, staged=None):
    w = _workload(hydraulics, ncol, Nz)
    for finalize in (False, True):
        for asynchronous in (0, 1):
            off, on = _pair(w, asynchronous=asynchronous)
            for s in (off, on):
                s.step(w["dt"], n, finalize=finalize)
            assert count(on) == max(0, n - 2)
            _same(w, off, on)
            if staged is not None:
                assert on.last_program()["staged"] == staged and on.last_program()["scalar_inputs"] == (not staged)
            for s in (off, on):      # (a second call: its first launch derives, so every launch but the last goes interior)
                s.step(w["dt"], n, finalize=finalize)
            assert count(on) == max(0, n - 2) + n - 1
            assert on.last_program()["derive"] == "T_liq"
            _same(w, off, on)


@pytest.mark.parametrize("n", [1, 2, 3, 7, 40])
@pytest.mark.parametrize("hydraulics", ["default", "vg"])
@pytest.mark.parametrize("ncol,Nz", SHAPES)
def test_call_lengths(ncol, Nz, hydraulics, n):
    _call_lengths(ncol, Nz, hydraulics, n)


@pytest.mark.parametrize("hydraulics", ["default", "vg"])
@pytest.mark.parametrize("ncol,Nz", SHAPES)
def test_two_calls_equal_one(ncol, Nz, hydraulics):
    """2 + 5 steps in two calls, 7 in one, and 7 with the option off"""
    w = _workload(hydraulics, ncol, Nz)
    off, one, two = _device(w, 0), _device(w, 1), _device(w, 1)
    off.step(w["dt"], 7, finalize=False)
    one.step(w["dt"], 7, finalize=False)
    two.step(w["dt"], 2, finalize=False)
    assert count(two) == 0
    two.step(w["dt"], 5, finalize=False)
    assert (count(one), count(two)) == (5, 4)
    _same(w, off, one)
    _same(w, off, two)


def test_staged_instances_in_a_child_process():
    """The staged + vector-input instances (what HBM-resident states take): TRM_STAGED_SMALL=1 TRM_SCALAR_INPUTS=0 are read once per
    process, hence the child process, which runs the call-length cases of one 32-lane and one 64-lane shape."""
    env = dict(os.environ, TRM_STAGED_SMALL="1", TRM_SCALAR_INPUTS="0")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--staged-child"], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "staged child ok" in out.stdout


def _staged_child():
    for ncol, Nz in ((5, 30), (67, 32), (67, 40)):
        for hydraulics in ("default", "vg"):
            for n in (3, 7):
                _call_lengths(ncol, Nz, hydraulics, n, staged=True)
    print("staged child ok")


# ---- 2. every signature ------------------------------------------------------------------------------------------------------------
SIGNATURES = [("closed", 0), ({}, 2), ({("internal_energy", "bottom"): ("flux", 0.05)}, 6), ({("saturation_water_ice", "top"): ("flux", -2.0e-7)}, 34)]


@pytest.mark.parametrize("hydraulics,Nz", [("default", 32), ("vg", 40)])
@pytest.mark.parametrize("extra,signature", SIGNATURES)
def test_every_signature(extra, signature, hydraulics, Nz):
    w = _workload(hydraulics, 67, Nz)
    if extra == "closed":
        w["bcs"].clear()
    else:
        for key, (kind, value) in extra.items():
            w["bcs"][key] = (kind, np.full(w["Nh"], value))
    off, on = _pair(w)
    assert on.get_option("info_bc_signature") == signature
    for s in (off, on):
        s.step(w["dt"], 6, finalize=False)
        s.step(w["dt"], 5, finalize=True)
    assert count(on) == 4 + 4
    assert on.last_program()["bc_signature"] == signature
    _same(w, off, on)


def test_top_temperature_series_changing_every_step():
    w = _workload("default", 67, 32)
    off, on = _pair(w)
    times = w["dt"] * np.arange(12)
    vals = np.stack([w["T0"] + 3.0 * np.sin(0.9 * k) - 0.2 * k for k in range(12)])
    for s in (off, on):
        s.set_bc_series("temperature", "top", "value", times, vals, "linear")
        s.step(w["dt"], 9, finalize=False)
    assert count(on) == 7
    _same(w, off, on)
    assert off.get("temperature").tobytes() != _device(w, 0).get("temperature").tobytes()


# ---- 3. status parity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hydraulics", ["default", "vg"])
def test_status_parity(hydraulics):
    """A time step of 3.0e4 s on this workload drives the composition out of its bounds in the second step (found with the CPU oracle:
    its status reads 0 after step 1 and TRM_STATUS_COMPOSITION from step 2 on, both hydraulics).  With interior launches the flag of a
    state is raised by the entry derivation of the launch behind the one that produced it (ColumnArgs::check_entry)."""
    w = _workload(hydraulics, 5, 32)
    dt = 3.0e4
    off, on = _pair(w)
    for n in (1, 3, 2, 4):      # (step 2 is the first launch of the second call: an interior launch)
        for s in (off, on):
            s.step(dt, n, finalize=False)
        assert on.status() == off.status(), n
    assert off.status() != 0
    assert count(on) == 0 + 2 + 1 + 3
    _same(w, off, on)
    # the first launch of a call does not check the state it reads (the launch that produced it has), interior or not
    for s in (off, on):
        s.set_status(0)
        s.step(dt, 3, finalize=False)
    assert on.status() == off.status()
    _same(w, off, on)
    for s in (off, on):
        s.set_status(0)
        s.step(dt, 1, finalize=False)
    assert on.status() == off.status()


# ---- 4. must not go interior ---------------------------------------------------------------------------------------------------------
def _never_interior(w, off, on, step="step", n=4):
    for _ in range(2):
        for s in (off, on):
            getattr(s, step)(w["dt"], n, finalize=False)
        assert count(on) == 0
    _same(w, off, on)


@pytest.mark.parametrize("field", ["internal_energy", "temperature", "pressure_head", "surface_excess_water"])
def test_not_interior_with_an_open_average(field):
    w = _workload()
    off, on = _pair(w)
    h = [s.open_average(field) for s in (off, on)]
    _never_interior(w, off, on)
    (a, wa, na), (b, wb, nb) = off.average(h[0]), on.average(h[1])
    assert a.tobytes() == b.tobytes() and (wa, na) == (wb, nb)
    for s, x in zip((off, on), h):      # closed: the next call goes interior
        s.close_average(x)
        s.step(w["dt"], 4, finalize=False)
    assert count(on) == 3
    _same(w, off, on)


def test_not_interior_with_a_tangent_state():
    w = _workload(config="heat")
    off, on = _pair(w)
    on.open_tangent()
    _never_interior(w, off, on)


@pytest.mark.parametrize("case", ["land", "land_launch_pair", "heun", "fp32", "fp32_unpacked", "generic_boundary", "defer_off", "write_kf_off", "derive_off",
                                  "runtime_kinds", "unfused", "multi_step_program"])
def test_not_interior(case):
    w = _workload(config="land" if case.startswith("land") else "richards", dtype=np.float32 if case.startswith("fp32") else np.float64)
    options = {"land_launch_pair": dict(surface_in_launch=0), "fp32_unpacked": dict(packed_f32=0), "defer_off": dict(defer_closure_stores=0),
               "write_kf_off": dict(write_kf_every_step=0), "derive_off": dict(derive_closure_fields=0), "runtime_kinds": dict(bc_signature=0),
               "unfused": dict(step_kernel="unfused"), "multi_step_program": dict(steps_per_launch=0)}.get(case, {})
    off, on = _pair(w, **options)
    if case == "generic_boundary":
        for s in (off, on):
            s.set_bc("pressure_head", "bottom", "gradient", np.full(w["Nh"], 0.25))
        assert on.get_option("info_generic_boundary_kernels") == 1
    _never_interior(w, off, on, step="step_heun" if case == "heun" else "step")


@pytest.mark.parametrize("field", ["internal_energy", "pressure_head", "water_table"])
def test_not_interior_with_an_escaped_device_pointer(field):
    w = _workload()
    off, on = _pair(w)
    for s in (off, on):
        s.step(w["dt"], 3, finalize=False)
    assert count(on) == 1
    for s in (off, on):
        s.device_array(field)
    for _ in range(2):
        for s in (off, on):
            s.step(w["dt"], 4, finalize=False)
        assert count(on) == 1
    _same(w, off, on)


@pytest.mark.parametrize("field", ["pressure_head", "water_table"])
def test_an_uploaded_field_is_read_not_derived(field):
    """an upload of pressure_head or water_table in front of a call: its first launch reads what the caller stored (the results depend
    on it), and only the launches behind it may go interior"""
    w = _workload()
    off, on, untouched = _device(w, 0), _device(w, 1), _device(w, 0)
    for s in (off, on, untouched):
        s.step(w["dt"], 3, finalize=False)
    x = off.get(field)
    x = x - 0.37 * (1.0 + np.arange(x.shape[-1]) % 3)
    for s in (off, on):
        s.set(field, x)
        s.step(w["dt"], 2, finalize=False)
    untouched.step(w["dt"], 2, finalize=False)
    assert count(on) == 1                   # (the first call's; none in the two-step call behind the upload)
    _same(w, off, on)
    if field == "pressure_head":            # (the upload is not a no-op: a launch that derived the pressure head would miss it)
        assert off.get("saturation_water_ice").tobytes() != untouched.get("saturation_water_ice").tobytes()
    for s in (off, on):
        s.set(field, x)
        s.step(w["dt"], 4, finalize=False)
    assert count(on) == 1 + 2
    _same(w, off, on)


@pytest.mark.parametrize("call", ["compute_auxiliary", "closure", "update_state", "initialize"])
def test_state_functions_between_calls(call):
    w = _workload()
    off, on = _pair(w)
    for s in (off, on):
        s.step(w["dt"], 3, finalize=False)
        getattr(s, call)()
        s.step(w["dt"], 2, finalize=False)
    assert count(on) == 1
    _same(w, off, on)


# ---- 5. snapshots, DeviceGroup ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hydraulics", ["default", "vg"])
def test_save_and_restore_around_calls(hydraulics):
    w = _workload(hydraulics)
    off, on = _pair(w)
    for s in (off, on):
        s.step(w["dt"], 3, finalize=False)
        s.save_state()
        s.step(w["dt"], 4, finalize=False)
    assert count(on) == 1 + 3
    _same(w, off, on)
    for s in (off, on):
        s.restore_state()
    _same(w, off, on)
    for s in (off, on):      # (the restored pressure head is read as stored by the first launch)
        s.step(w["dt"], 2, finalize=False)
    assert count(on) == 4
    _same(w, off, on)
    for s in (off, on):
        s.step(w["dt"], 5, finalize=True)
    assert count(on) == 4 + 4
    _same(w, off, on)


def test_device_group_deals_one_step_calls():
    w = _workload(ncol=66)
    halves = [W.shard_workload(w, 0, 33), W.shard_workload(w, 33, 66)]
    off = [_device(h, 0) for h in halves]
    group = trm.DeviceGroup([_device(h, 1) for h in halves])
    group.step(w["dt"], 7, finalize=False)
    group.step(w["dt"], 2, finalize=True)
    for s in off:
        s.step(w["dt"], 7, finalize=False)
        s.step(w["dt"], 2, finalize=True)
    assert [count(s) for s in group.states] == [0, 0]
    for h, a, b in zip(halves, off, group.states):
        _same(h, a, b)


if __name__ == "__main__":
    if "--staged-child" in sys.argv:
        _staged_child()
