"""Time averages accumulated on the device (trm_average_*, AveragedTimeInterval).

Every mean is checked bit for bit against a numpy replay of the documented arithmetic: per launch P = sum_k dt * x_k (x_k the field
after step k, P from 0.0), acc = acc + P, mean = acc / window rounded once to the context precision.  The x_k come from per-step
downloads of a twin context stepped one launch per step (its states are bit-identical to the multi-step program's)."""
import numpy as np
import pytest

import workloads as W
import terrarium_jl_amd as trm

pytestmark = pytest.mark.gpu

SOIL = ("internal_energy", "saturation_water_ice", "temperature", "liquid_water_fraction", "pressure_head")
SURFACE = ("skin_temperature", "ground_heat_flux", "surface_shortwave_up", "surface_longwave_up", "surface_net_radiation",
           "sensible_heat_flux", "latent_heat_flux", "evaporation_ground", "infiltration", "surface_runoff")


def columns(n=4096, name="N72"):
    lat, lon = W.columns_from_mask(name)
    sel = np.linspace(0, lat.size - 1, n).astype(int)
    return lat[sel], lon[sel]


def averaged_fields(w, fused=True):
    names = list(SOIL)
    if w["config"] != "heat" or not fused:
        names += ["surface_excess_water", "water_table"]
    if w["config"] == "land":
        names += list(SURFACE)
    return names


def launches(calls, spl):
    """launch sizes of trm_step calls of `calls` steps with `spl` steps per launch"""
    out = []
    for n in calls:
        while n > 0:
            out.append(min(spl, n))
            n -= out[-1]
    return out


def replay(xs, segments, dt, dtype):
    """(mean, window) of per-step values xs[k] (float arrays) over launches of the given sizes"""
    acc = np.zeros_like(np.asarray(xs[0], dtype=np.float64))
    window, k = 0.0, 0
    for m in segments:
        p = np.zeros_like(acc)
        for _ in range(m):
            p = p + dt * np.asarray(xs[k], dtype=np.float64)
            window += dt
            k += 1
        acc = acc + p
    return (acc / window).astype(dtype), window


def twin_values(d, names, dt, nsteps, heun=False):
    """per-step values of `names` from a context stepped one launch per step"""
    xs = {n: [] for n in names}
    for _ in range(nsteps):
        if heun == "three_call":
            d.heun_predict(dt)
            d.heun_correct(dt, finalize=False)
        else:
            (d.step_heun if heun else d.step)(dt, 1, finalize=False)
        for n in names:
            xs[n].append(d.get(n).copy())
    return xs


def program(d):
    return trm._capi.decode_program(d.get_option("info_last_program"))


def check_means(a, handles, xs, segments, dt, dtype):
    for n, h in handles.items():
        mean, window, steps = a.average(h)
        ref, wref = replay(xs[n], segments, dt, dtype)
        assert steps == sum(segments) and window == wref, n
        assert mean.dtype == np.dtype(dtype) and np.array_equal(mean, ref, equal_nan=True), n


FUSED = [("heat", "default", np.float64, 32), ("richards", "default", np.float64, 32), ("richards", "vg", np.float64, 50),
         ("land", "default", np.float64, 32), ("land", "vg", np.float64, 50), ("richards", "default", np.float32, 32),
         ("land", "default", np.float32, 32)]


@pytest.mark.parametrize("config,hydraulics,dtype,Nz", FUSED)
def test_fused_averages_equal_the_replay_bitwise(config, hydraulics, dtype, Nz):
    """Multi-step program with averages accumulated in the launch (LandModel: surface processes inline)."""
    w = W.make_workload(config, *columns(), Nz, dtype=dtype, hydraulics=hydraulics)
    a, b = W.setup_device(w, steps_per_launch=7), W.setup_device(w, steps_per_launch=1)
    for d in (a, b):
        d.set_option("packed_f32", 0)
    names = averaged_fields(w)
    handles = {n: a.open_average(n) for n in names}
    calls = (57, 1, 12)
    for n in calls:     # (finalize = 0: a finalizing call re-evaluates the LandModel's surface processes, which the twin would not)
        a.step(w["dt"], n, finalize=False)
    p = program(a)
    assert p["family"] == "column_multi" and p.get("averages") == "in_launch"
    assert (p["surface_inline"] if config == "land" else True)
    xs = twin_values(b, names, w["dt"], sum(calls))
    check_means(a, handles, xs, launches(calls, 7), w["dt"], dtype)


def test_fused_averages_with_a_series_and_two_handles_per_field():
    """SERIES: a periodic surface temperature series interpolated in the kernel; two accumulators of one field (scratch partial)."""
    w = W.make_workload("richards", *columns(), 32)
    a, b = W.setup_device(w, steps_per_launch=7), W.setup_device(w, steps_per_launch=1)
    tt = 3600.0 * np.arange(25)
    vals = w["T0"][None, :] + 8.0 * np.sin(2 * np.pi * tt[:, None] / 86400.0 - w["lon"][None, :])
    for d in (a, b):
        d.set_bc_series("temperature", "top", "value", tt, vals, "cyclical")
    h1 = {n: a.open_average(n) for n in ("temperature", "saturation_water_ice", "water_table")}
    a.step(w["dt"], 20, finalize=True)
    h2 = a.open_average("temperature")
    a.step(w["dt"], 30, finalize=True)
    p = program(a)
    assert p["family"] == "column_multi" and p["series"] and p.get("averages") == "in_launch"
    xs = twin_values(b, ["temperature", "saturation_water_ice", "water_table"], w["dt"], 50)
    check_means(a, h1, xs, launches((20, 30), 7), w["dt"], np.float64)
    mean, window, steps = a.average(h2)
    ref, wref = replay(xs["temperature"][20:], launches((30,), 7), w["dt"], np.float64)
    assert steps == 30 and window == wref and np.array_equal(mean, ref)


def generic_case(kind):
    """(workload, options, stepping) of the programs that accumulate through k_accumulate"""
    if kind == "signature_euler":
        return W.make_workload("richards", *columns(), 32), dict(steps_per_launch=1), "euler"
    if kind == "land_surface_in_launch":
        return W.make_workload("land", *columns(), 32), dict(steps_per_launch=1, surface_in_launch=1), "euler"
    if kind == "fused_heun":
        return W.make_workload("richards", *columns(), 32), {}, "heun"
    if kind == "deep_96":
        return W.make_workload("heat", *columns(), 96), {}, "euler"
    if kind == "packed_f32":
        return W.make_workload("richards", *columns(), 32, dtype=np.float32), dict(steps_per_launch=1), "euler"
    if kind == "unfused":
        return W.make_workload("land", *columns(), 32), dict(step_kernel="unfused"), "euler"
    if kind == "three_call_heun":
        return W.make_workload("richards", *columns(), 32), {}, "three_call"
    if kind == "noflow_surface_water":      # the NoFlow program does not carry the 2-D soil fields: per-step path
        return W.make_workload("heat", *columns(), 32), {}, "euler"
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["signature_euler", "land_surface_in_launch", "fused_heun", "deep_96", "packed_f32", "unfused",
                                  "three_call_heun", "noflow_surface_water"])
def test_generic_path_averages_equal_the_replay_bitwise(kind):
    w, opts, stepping = generic_case(kind)
    a, b = W.setup_device(w, steps_per_launch=0), W.setup_device(w, steps_per_launch=1)
    for d in (a, b):
        for k, v in opts.items():
            d.set_option(k, v)
    names = averaged_fields(w, fused=False)
    handles = {n: a.open_average(n) for n in names}
    calls = (9, 1, 4)
    for n in calls:
        if stepping == "euler":
            a.step(w["dt"], n, finalize=False)
        elif stepping == "heun":
            a.step_heun(w["dt"], n, finalize=False)
        else:
            for k in range(n):
                a.heun_predict(w["dt"])
                a.heun_correct(w["dt"], finalize=False)
    assert program(a).get("averages") == "after_launch"
    xs = twin_values(b, names, w["dt"], sum(calls), heun="three_call" if stepping == "three_call" else stepping == "heun")
    check_means(a, handles, xs, [1] * sum(calls), w["dt"], w["dtype"])


@pytest.mark.parametrize("spl", [0, 1])
@pytest.mark.parametrize("config", ["richards", "land"])
def test_open_averages_change_nothing_else(config, spl):
    """Every field, the clock, the status word and the tendencies: array_equal with and without open accumulators."""
    w = W.make_workload(config, *columns(1024), 32)
    a, b = W.setup_device(w, steps_per_launch=spl), W.setup_device(w, steps_per_launch=spl)
    for n in averaged_fields(w):
        a.open_average(n)
    for d in (a, b):
        d.step(w["dt"], 23, finalize=False)
        d.step(w["dt"], 10, finalize=True)
    assert a.clock() == b.clock() and a.status() == b.status()
    names = W.compared_fields(w) + ["tend_internal_energy"] + (["tend_saturation_water_ice", "tend_surface_excess_water"])
    for n in names:
        assert np.array_equal(a.get(n), b.get(n), equal_nan=True), n


def test_handles():
    w = W.make_workload("richards", *columns(512), 32)
    d = W.setup_device(w, steps_per_launch=5)
    h1 = d.open_average("temperature")
    with pytest.raises(trm._capi.TerrariumHipError) as e:
        d.average(h1)
    assert e.value.code == trm._capi.TRM_ESTALE
    d.step(w["dt"], 6)
    h2 = d.open_average("temperature")          # same field, later window start
    d.step(w["dt"], 4)
    m1, w1, n1 = d.average(h1)
    m2, w2, n2 = d.average(h2)
    assert (n1, n2) == (10, 4) and w1 == 10 * w["dt"] and w2 == 4 * w["dt"]
    assert not np.array_equal(m1, m2)
    d.reset_average(h1)
    d.step(w["dt"], 4)
    assert d.average(h1)[2] == 4 and d.average(h2)[2] == 8
    d.reset()                                     # trm_reset: zero, handles kept
    with pytest.raises(trm._capi.TerrariumHipError) as e:
        d.average(h2)
    assert e.value.code == trm._capi.TRM_ESTALE
    d.close_average(h2)
    with pytest.raises(trm._capi.TerrariumHipError) as e:
        d.average(h2)
    assert e.value.code == trm._capi.TRM_EINVAL
    for name in ("tend_internal_energy", "air_temperature", "skin_temperature", "ground_heat_flux"):   # SoilModel: no surface fields
        with pytest.raises(trm._capi.TerrariumHipError) as e:
            d.open_average(name)
        assert e.value.code == trm._capi.TRM_EUNSUPPORTED, name
    d.close()


@pytest.mark.parametrize("host_function", [False, True])
def test_simulation_averaged_writer_matches_a_host_average(tmp_path, host_function):
    """N72 soil_heat_global-style run: periodic surface temperature, dt = 600 s, one day, AveragedTimeInterval(3 h, window = 1 h)
    on temperature with the ring grid, against the host average of an IterationInterval(1) snapshot writer of the same run.
    host_function: the surface temperature is a host function of time (one trm_step per step)."""
    mask = trm.masks.load_land_mask("N72")
    grid = trm.ColumnRingGrid(trm.ExponentialSpacing(N=16), mask)
    lat, lon = trm.masks.masked_latlon(mask)
    T0 = 20.0 - np.abs(40.0 * np.sin(lat))
    f = lambda t: T0 + 10 * np.sin(2 * np.pi * t / 86400.0 - lon)
    value = f if host_function else trm.FieldTimeSeries.from_function(f, 600.0 * np.arange(150))
    bc = trm.PrescribedSurfaceTemperature("Ts", value)
    integ = trm.initialize(trm.SoilModel(grid), trm.ForwardEuler(dt=600.0), boundary_conditions=bc,
                           initializers=dict(temperature=T0[None, :] * np.ones((16, 1)), saturation_water_ice=0.7))
    assert integ._has_time_dependence() == host_function
    sim = trm.Simulation(integ, dt=600.0, stop_time=86400.0)
    out = tmp_path / "mean.npz"
    sim.output_writers["mean"] = trm.SnapshotWriter(["temperature"], trm.AveragedTimeInterval(3 * 3600.0, window=3600.0),
                                                    filename=str(out), ring_grid=grid)
    sim.output_writers["every"] = trm.SnapshotWriter(["temperature"], trm.IterationInterval(1))
    trm.run_simulation(sim)
    f_out = np.load(out)
    ends = [3 * 3600.0 * k for k in range(1, 9)]
    assert list(f_out["time"]) == ends and list(f_out["window_start"]) == [e - 3600.0 for e in ends]
    assert f_out["temperature"].shape == (8, 16) + mask.shape
    every = sim.output_writers["every"]
    snaps = {t: grid.gather(np.asarray(a)) if np.asarray(a).ndim == 3 else np.asarray(a) for t, a in zip(every.times, every.data["temperature"])}
    for k, e in enumerate(ends):
        steps = [t for t in snaps if e - 3600.0 < t <= e + 1e-6]
        assert len(steps) == 6
        host = sum(600.0 * snaps[t] for t in sorted(steps)) / 3600.0
        assert np.allclose(grid.gather(f_out["temperature"][k]), host, rtol=1e-13, atol=0), k


def test_mean_matches_the_oracle():
    """The mean temperature of a few steps against the CPU oracle's trajectory (the tolerance of the parity tests: exact for
    the soil model)."""
    w = W.make_workload("richards", *columns(200), 32)
    d, o = W.setup_device(w, steps_per_launch=0), W.setup_oracle(w)
    h = d.open_average("temperature")
    d.step(w["dt"], 8, finalize=True)
    acc = np.zeros((32, 200))
    for _ in range(8):
        o.run(w["dt"], 1)
        acc = acc + w["dt"] * o.get("temperature")
    mean, window, _ = d.average(h)
    assert np.array_equal(mean, acc / window)


def test_averaged_time_interval_schedule_events():
    s = trm.AveragedTimeInterval(3 * 3600.0, window=3600.0)
    s.first = 0.0
    assert s.next_time(0.0) == 2 * 3600.0 and s.steps_until_next(0.0, 0, 600.0) == 12
    assert s.due(2 * 3600.0) == [("start", 1)] and s.next_time() == 3 * 3600.0
    assert s.due(3 * 3600.0) == [("end", 1)] and s.next_time() == 5 * 3600.0
    with pytest.raises(ValueError):
        trm.AveragedTimeInterval(3600.0, window=7200.0)
