"""TRM_OPT_DEFER_CLOSURE_STORES: a deriving per-step launch leaves temperature / liquid_water_fraction unstored and the library
materialises them in front of whatever touches field memory next.  Nothing a caller can observe may change: every check here is
byte identity against a context that stores them at every step (option 0), plus the two info keys that say what the library did
(TRM_INFO_CLOSURE_STORED, TRM_INFO_MATERIALIZATIONS).

The deriving instance is forced at test sizes with derive_closure_fields = 1.  A context's first step after trm_initialize reads
T / liq as stored (temperature is the user's then), so deferral starts with the second step.  Only ForwardEuler defers: the Heun
program reads T / liq as stored and always stores them."""
import types

import numpy as np
import pytest

import terrarium_jl_amd as trm
import workloads as W

pytestmark = pytest.mark.gpu

PHYSICS = {"c3": ("richards", "default"), "c3vg": ("richards", "vg"), "c4": ("land", "default"), "c4vg": ("land", "vg"), "heat": ("heat", "default")}
NCOL = 333      # (odd: the last wave holds one real column and one clamped copy)


def _workload(physics, ncol=NCOL, Nz=32):
    config, hyd = PHYSICS[physics]
    lat, lon = W.columns_from_mask("N72")
    sel = np.linspace(0, lat.size - 1, ncol).astype(int)
    return W.make_workload(config, lat[sel], lon[sel], Nz, hydraulics=hyd)


def _device(w, defer, derive=1, **options):
    d = W.setup_device(w)
    d.set_option("derive_closure_fields", derive)
    d.set_option("defer_closure_stores", defer)
    for k, v in options.items():
        d.set_option(k, v)
    return d


def _pair(physics, **options):
    """(workload, eager context, deferring context), identical but for the option"""
    w = _workload(physics)
    return w, _device(w, 0, **options), _device(w, 1, **options)


def stored(d): return d.get_option("info_closure_stored")
def launches(d): return d.get_option("info_materializations")


def _same_state(w, a, b):
    for name in W.compared_fields(w):
        x, y = a.get(name), b.get(name)
        assert x.tobytes() == y.tobytes(), name
    assert a.status() == b.status()
    assert a.clock() == b.clock()


def _deferring(w, e, d, k=3):
    """k steps on both; the deferring context has deferred, the eager one never does.  Returns its launch count so far."""
    for s in (e, d):
        s.step(w["dt"], k, finalize=False)
    assert stored(e) == 1 and launches(e) == 0
    assert stored(d) == 0, "the deriving per-step launch did not defer"
    assert d.get_option("info_closure_consistent") == 1      # ("the next step may derive" stays 1 while deferred)
    assert d.last_program() == e.last_program()
    assert d.last_program()["derive"] == "T_liq"
    return launches(d)


def _flushed_once(d, m0):
    assert stored(d) == 1
    assert launches(d) == m0 + 1


# ---- 1. bit identity -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("asynchronous", [0, 1])
@pytest.mark.parametrize("finalize", [False, True])
@pytest.mark.parametrize("nsteps", [1, 2, 7, 40])
@pytest.mark.parametrize("physics", ["c3", "c3vg", "c4", "c4vg", "heat"])
def test_bit_identity(physics, nsteps, finalize, asynchronous):
    w, e, d = _pair(physics, asynchronous=asynchronous)
    for s in (e, d):
        s.step(w["dt"], nsteps, finalize=finalize)
    assert stored(d) == (1 if nsteps == 1 else 0)
    assert d.status() == e.status()                  # (reads no field memory: materialises nothing)
    assert d.last_program() == e.last_program()
    assert stored(d) == (1 if nsteps == 1 else 0)
    _same_state(w, e, d)
    assert stored(d) == 1 and launches(d) == (0 if nsteps == 1 else 1)
    assert launches(e) == 0


@pytest.mark.parametrize("physics", ["c4", "c4vg"])
def test_bit_identity_launch_pair(physics):
    """the LandModel on the k_surface + k_column pair (surface_in_launch = 0) instead of k_column_land"""
    w, e, d = _pair(physics, surface_in_launch=0)
    _deferring(w, e, d, 7)
    assert d.last_program()["family"] == "column_euler"
    _same_state(w, e, d)


def test_bit_identity_one_call_per_step():
    w, e, d = _pair("c3")
    for _ in range(9):
        e.step(w["dt"], 1, finalize=False)
        d.step(w["dt"], 1, finalize=False)
    assert stored(d) == 0 and launches(d) == 0
    _same_state(w, e, d)
    assert launches(d) == 1


# ---- 2. flush matrix -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", ["temperature", "liquid_water_fraction"])
@pytest.mark.parametrize("how", ["download", "download_rows", "download_ring"])
def test_flush_on_download(how, field):
    w, e, d = _pair("c3")
    if how == "download_ring":
        idx = np.arange(NCOL, dtype=np.int64) * 2
        for s in (e, d):
            s.set_ring_grid(2 * NCOL, idx)
    m0 = _deferring(w, e, d)
    read = {"download": lambda s: s.get(field), "download_rows": lambda s: s.get_rows(field, 3, 5),
            "download_ring": lambda s: s.get_ring(field, fill=-1.0)}[how]
    x, y = read(e), read(d)
    assert x.tobytes() == y.tobytes()
    _flushed_once(d, m0)
    _same_state(w, e, d)
    assert launches(d) == m0 + 1


@pytest.mark.parametrize("op", ["max", "sum", "min"])
def test_flush_on_reduce(op):
    w, e, d = _pair("c3")
    m0 = _deferring(w, e, d)
    assert e.reduce("temperature", op).tobytes() == d.reduce("temperature", op).tobytes()
    _flushed_once(d, m0)


@pytest.mark.parametrize("physics", ["c3", "c4"])
@pytest.mark.parametrize("call", ["update_state", "compute_auxiliary", "closure"])
def test_flush_on_state_function(call, physics):
    w, e, d = _pair(physics)
    m0 = _deferring(w, e, d)
    for s in (e, d):
        getattr(s, call)()
    _flushed_once(d, m0)
    _same_state(w, e, d)
    for name in ("tend_internal_energy", "tend_saturation_water_ice"):
        if call == "update_state":
            assert e.get(name).tobytes() == d.get(name).tobytes(), name


@pytest.mark.parametrize("physics", ["c3", "c4"])
@pytest.mark.parametrize("what", ["unfused_step", "heun_step", "multi_step", "generic_boundary_step", "derive_off_step"])
def test_flush_on_other_step(what, physics):
    w, e, d = _pair(physics)
    m0 = _deferring(w, e, d)
    for s in (e, d):
        if what == "unfused_step":
            s.set_option("step_kernel", "unfused")
            s.step(w["dt"], 2, finalize=False)
        elif what == "heun_step":
            s.step_heun(w["dt"], 2, finalize=False)
        elif what == "multi_step":
            s.set_option("steps_per_launch", 0)
            s.step(w["dt"], 5, finalize=False)
        elif what == "generic_boundary_step":
            # (trm_set_bc touches no field memory and materialises nothing: the step that follows does, in front of k_step_wave)
            s.set_bc("pressure_head", "bottom", "gradient", np.full(NCOL, 0.25))
            assert s.get_option("info_generic_boundary_kernels") == 1
            if s is d:
                assert stored(d) == 0
            s.step(w["dt"], 2, finalize=False)
        else:
            s.set_option("derive_closure_fields", 0)
            s.step(w["dt"], 2, finalize=False)
    _flushed_once(d, m0)
    assert d.last_program() == e.last_program()
    assert d.last_program()["derive"] == "none" or d.last_program()["family"] not in ("column_euler", "column_land")
    _same_state(w, e, d)
    assert launches(d) == m0 + 1


@pytest.mark.parametrize("option,value", [("step_kernel", "unfused"), ("derive_closure_fields", 0), ("derive_closure_fields", 2), ("defer_closure_stores", 0)])
def test_flush_on_option_switch(option, value):
    w, e, d = _pair("c3")
    m0 = _deferring(w, e, d)
    d.set_option(option, value)
    _flushed_once(d, m0)
    e.set_option(option, value)
    _same_state(w, e, d)
    for s in (e, d):
        s.step(w["dt"], 3, finalize=True)
    assert stored(d) == 1 and launches(d) == m0 + 1
    _same_state(w, e, d)


def test_options_that_keep_the_program_do_not_flush():
    w, e, d = _pair("c3")
    m0 = _deferring(w, e, d)
    d.set_option("asynchronous", 1)
    d.set_option("asynchronous", 0)
    d.synchronize()
    d.clock()
    d.get_option("derive_closure_fields")
    assert stored(d) == 0 and launches(d) == m0


@pytest.mark.parametrize("field", ["temperature", "internal_energy", "pressure_head"])
def test_flush_on_device_pointer_ends_deferral(field):
    import torch
    w, e, d = _pair("c3")
    m0 = _deferring(w, e, d)
    a = d.device_array(field)
    _flushed_once(d, m0)
    if field == "temperature":      # what the pointer shows is what an eager context downloads
        t = torch.as_tensor(a, device="cuda")
        d.synchronize()
        got = t[:, :w["Nz"]].T.cpu().numpy()
        assert got.tobytes() == np.ascontiguousarray(e.get("temperature")).tobytes()
    e.device_array(field)
    for s in (e, d):
        s.step(w["dt"], 4, finalize=False)
    assert stored(d) == 1 and launches(d) == m0 + 1
    assert d.last_program() == e.last_program()
    _same_state(w, e, d)


def test_flush_on_opening_a_temperature_average():
    w, e, d = _pair("c3")
    m0 = _deferring(w, e, d)
    he, hd = e.open_average("temperature"), d.open_average("temperature")
    _flushed_once(d, m0)
    for s in (e, d):
        s.step(w["dt"], 5, finalize=False)
    assert stored(d) == 1 and launches(d) == m0 + 1
    (ae, we, ne), (ad, wd, nd) = e.average(he), d.average(hd)
    assert ae.tobytes() == ad.tobytes() and (we, ne) == (wd, nd)
    _same_state(w, e, d)
    # an average of a field the step stores anyway does not stand in the way
    for s, h in ((e, he), (d, hd)):
        s.close_average(h)
    he, hd = e.open_average("internal_energy"), d.open_average("internal_energy")
    for s in (e, d):
        s.step(w["dt"], 3, finalize=False)
    assert stored(d) == 0
    assert e.average(he)[0].tobytes() == d.average(hd)[0].tobytes()
    _same_state(w, e, d)


@pytest.mark.parametrize("physics", ["c3", "c4"])
def test_flush_on_restart_write(physics):
    w, e, d = _pair(physics)
    m0 = _deferring(w, e, d)
    ce, cd = (trm.checkpoint(types.SimpleNamespace(state=s)) for s in (e, d))
    _flushed_once(d, m0)
    assert (ce["time"], ce["iteration"], ce["status"]) == (cd["time"], cd["iteration"], cd["status"])
    assert sorted(ce["fields"]) == sorted(cd["fields"]) and "temperature" in cd["fields"]
    for name in ce["fields"]:
        assert ce["fields"][name].tobytes() == cd["fields"][name].tobytes(), name


@pytest.mark.parametrize("physics", ["c3", "c4"])
def test_flush_on_save_state_and_restore(physics):
    w, e, d = _pair(physics)
    m0 = _deferring(w, e, d)
    for s in (e, d):
        s.save_state()
    _flushed_once(d, m0)                 # (the saved copy is current)
    for s in (e, d):
        s.step(w["dt"], 4, finalize=False)
    assert stored(d) == 0
    for s in (e, d):
        s.restore_state()
    assert stored(d) == 1 and launches(d) == m0 + 1      # (dropped, not materialised)
    _same_state(w, e, d)
    for s in (e, d):
        s.step(w["dt"], 4, finalize=True)
    _same_state(w, e, d)


def test_flush_on_upload_of_one_closure_field():
    """an upload of T alone must find the liquid fraction current"""
    w, e, d = _pair("c3")
    m0 = _deferring(w, e, d)
    T = e.get("temperature") + 0.5
    for s in (e, d):
        s.set("temperature", T)
    _flushed_once(d, m0)
    assert e.get("liquid_water_fraction").tobytes() == d.get("liquid_water_fraction").tobytes()
    for s in (e, d):
        s.initialize()
        s.step(w["dt"], 3, finalize=True)
    _same_state(w, e, d)


# ---- 3. drop ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("physics", ["c3", "c4"])
def test_restore_drops_without_a_launch(physics):
    w, e, d = _pair(physics)
    for s in (e, d):
        s.step(w["dt"], 1, finalize=False)
        s.save_state()
    assert launches(d) == 0
    m0 = _deferring(w, e, d)
    assert m0 == 0
    for s in (e, d):
        s.restore_state()
    assert stored(d) == 1 and launches(d) == 0
    _same_state(w, e, d)
    for s in (e, d):
        s.step(w["dt"], 6, finalize=False)
    assert stored(d) == 0
    _same_state(w, e, d)


# ---- 4. no deferral where it is illegal --------------------------------------------------------------------------------------
def _never_deferred(w, d, k=4):
    for _ in range(2):
        d.step(w["dt"], k, finalize=False)
        assert stored(d) == 1
    assert launches(d) == 0


def test_no_deferral_small_grid_auto_rule():
    w = _workload("c3")
    d = _device(w, 1, derive=2)
    _never_deferred(w, d)
    assert d.last_program()["derive"] == "none"


def test_no_deferral_vegetation_coupled():
    lat, lon = W.columns_from_mask("N72")
    sel = np.linspace(0, lat.size - 1, 200).astype(int)
    w = W.make_workload("landveg", lat[sel], lon[sel], 32)
    d = _device(w, 1)
    _never_deferred(w, d)


@pytest.mark.parametrize("field", ["internal_energy", "liquid_water_fraction"])
def test_no_deferral_escaped_pointers(field):
    w = _workload("c3")
    d = _device(w, 1)
    d.device_array(field)
    _never_deferred(w, d)


@pytest.mark.parametrize("field", ["temperature", "liquid_water_fraction"])
def test_no_deferral_open_average(field):
    w = _workload("c3")
    d = _device(w, 1)
    d.open_average(field)
    _never_deferred(w, d)
    assert d.last_program()["derive"] == "T_liq"      # (it derives; it stores as well)


def test_no_deferral_tangents_attached():
    w = _workload("heat")
    e, d = _device(w, 0), _device(w, 1)
    d.open_tangent()
    _never_deferred(w, d)
    assert d.last_program()["derive"] == "T_liq"
    d.close_tangent()
    d.step(w["dt"], 2, finalize=False)
    assert stored(d) == 0
    e.step(w["dt"], 10, finalize=False)
    _same_state(w, e, d)


def test_no_deferral_option_off():
    w = _workload("c3")
    d = _device(w, 0)
    _never_deferred(w, d)
    assert d.last_program()["derive"] == "T_liq"


def test_no_deferral_pipeline_parts():
    w, e, d = _pair("c4", pipeline_parts=1)
    for s in (e, d):
        s.step(w["dt"], 6, finalize=False)
    assert d.last_program() == e.last_program()
    assert stored(d) == 1 and launches(d) == 0
    _same_state(w, e, d)


def test_part_launches_after_deferring_steps():
    """the interleaved LandModel path entered with the arrays stale: materialised in front of its first launch"""
    w, e, d = _pair("c4")
    m0 = _deferring(w, e, d)
    for s in (e, d):
        s.set_option("write_kf_every_step", 1)       # (an option that flushes nothing)
    assert stored(d) == 0
    for s in (e, d):
        s.set_option("pipeline_parts", 1)
        s.step(w["dt"], 4, finalize=False)
    _flushed_once(d, m0)
    _same_state(w, e, d)


# ---- 5. DeviceGroup ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("physics", ["c3", "c4"])
def test_device_group_two_contexts_one_device(physics):
    w = _workload(physics)
    halves = [W.shard_workload(w, 0, NCOL // 2), W.shard_workload(w, NCOL // 2, NCOL)]
    eager = [_device(h, 0) for h in halves]
    group = trm.DeviceGroup([_device(h, 1) for h in halves])
    group.step(w["dt"], 7, finalize=False)
    group.step(w["dt"], 2, finalize=True)
    for s in eager:
        s.step(w["dt"], 7, finalize=False)
        s.step(w["dt"], 2, finalize=True)
    assert [stored(s) for s in group.states] == [0, 0]
    for h, a, b in zip(halves, eager, group.states):
        _same_state(h, a, b)
    assert [launches(s) for s in group.states] == [1, 1]
