"""Forward-mode tangents of the heat + Richards step behind TRM_OPT_DERIVATIVE_RICHARDS: what the option opens and what stays refused,
the texts with the option at 0, linearity in the two seeds, agreement with the heat-only tangent where no water moves, the closure
tangent against the reference and the reference's analytic slope, and trm.jvp with a saturation seed against the C ABI.  The value-by-value comparison with
the exact Jacobian is test_gpu_tangent_richards_edges.py."""
import ctypes as C

import numpy as np
import pytest

import linearised_heat as LH
import linearised_richards as LR
import richards_cases as RC
import terrarium_jl_amd as trm
from richards_cases import DT, DZ, STEPS
from test_gpu_tangent_richards_edges import TANGENTS, bits, device, tangents

pytestmark = pytest.mark.gpu

CAPI = trm._capi
LD = np.longdouble
HEAT_ONLY = "the heat-only SoilModel (NoFlow) only"
STATE_SEEDS_ONLY = "on a Richards context: state seeds only"


def small(flow="richards", Nz=4, Nh=3):
    p = CAPI.default_params()
    p.flow = CAPI.FLOW[flow]
    d = trm.DeviceState(trm.ColumnGrid(trm.PrescribedSpacing(dz=[DZ] * Nz), Nh), p)
    d.set("temperature", np.linspace(-2.0, 2.0, Nz))
    d.set_bc("temperature", "top", "value", 1.0)
    d.initialize()
    return d


def call(d, name, *args):
    rc = getattr(d._lib, name)(d._ctx, *args)
    return rc, (d._lib.trm_last_error(d._ctx).decode() if rc else "")


def test_the_option_opens_a_richards_context():
    """the test that fails without the feature: trm_tangent_open on a Richards context"""
    d = small()
    assert d.get_option("derivative_richards") == 0
    d.set_option("derivative_richards", 1)
    assert call(d, "trm_tangent_open") == (CAPI.TRM_OK, "")
    buf = np.zeros((4, 3))
    for which in range(5):
        assert call(d, "trm_tangent_download", which, buf.ctypes.data)[0] == CAPI.TRM_OK, which
        assert np.all(buf == 0.0)
    dev, pitch = C.c_void_p(), C.c_int64()
    for which in range(5):
        assert call(d, "trm_tangent_device_ptr", which, C.byref(dev), C.byref(pitch))[0] == CAPI.TRM_OK and dev.value
    # the seeds are dU and dsat; the other three are the closure's
    for which, code in ((0, CAPI.TRM_OK), (3, CAPI.TRM_OK), (1, CAPI.TRM_EINVAL), (2, CAPI.TRM_EINVAL), (4, CAPI.TRM_EINVAL), (5, CAPI.TRM_EINVAL)):
        rc, msg = call(d, "trm_tangent_upload", which, buf.ctypes.data)
        assert rc == code and (not rc or msg == "trm_tangent_upload: bad argument"), (which, rc, msg)
    assert call(d, "trm_tangent_closure")[0] == CAPI.TRM_OK
    assert call(d, "trm_step_tangent", C.c_double(DT), 2)[0] == CAPI.TRM_OK
    prog = d.last_program()
    assert prog["family"] == "column_tangent_richards" and prog["hydraulics"] == "default" and prog["lanes_per_column"] == 32
    assert CAPI.decode_program(16 | 1 << 8 | 2 << 10) == dict(CAPI.decode_program(16 | 1 << 8 | 2 << 10), family="column_tangent_richards",
                                                                 hydraulics="vg_n2", lanes_per_column=64)


def test_with_the_option_at_zero_every_answer_is_todays():
    d = small()
    assert call(d, "trm_tangent_open") == (CAPI.TRM_EUNSUPPORTED, "trm_tangent_open: " + HEAT_ONLY)
    assert call(d, "trm_adjoint_open", 4) == (CAPI.TRM_EUNSUPPORTED, "trm_adjoint_open: " + HEAT_ONLY)
    seed = (C.c_double * 10)()
    assert call(d, "trm_tangent_param_set", seed) == (CAPI.TRM_EUNSUPPORTED, "trm_tangent_param_set: " + HEAT_ONLY)
    # a NoFlow context has three tangent fields, with the option or without it
    for option in (0, 1):
        h = small("noflow")
        h.set_option("derivative_richards", option)
        h.open_tangent()
        buf = np.zeros((4, 3))
        dev, pitch = C.c_void_p(), C.c_int64()
        for which in (3, 4):
            assert call(h, "trm_tangent_upload", which, buf.ctypes.data) == (CAPI.TRM_EINVAL, "trm_tangent_upload: bad argument")
            assert call(h, "trm_tangent_download", which, buf.ctypes.data) == (CAPI.TRM_EINVAL, "trm_tangent_download: bad argument")
            assert call(h, "trm_tangent_device_ptr", which, C.byref(dev), C.byref(pitch)) == (CAPI.TRM_EINVAL, "trm_tangent_device_ptr: bad argument")
        with pytest.raises(trm.TerrariumHipError):
            h.tangent("saturation")


def test_everything_else_still_refuses_a_richards_context():
    d = small()
    d.set_option("derivative_richards", 1)
    d.open_tangent()
    U = CAPI.TRM_EUNSUPPORTED
    buf = np.zeros(16)
    seed = (C.c_double * 10)()
    pos, lev = (C.c_int32 * 1)(1), (C.c_int32 * 1)(0)
    T, TOP = CAPI.BC_VAR["temperature"], CAPI.SIDE["top"]
    for name, args in (("trm_tangent_bc_upload", (T, TOP, buf.ctypes.data)), ("trm_tangent_bc_series_upload", (T, TOP, 5, buf.ctypes.data)),
                       ("trm_tangent_param_set", (seed,)), ("trm_tangent_record_attach", (1, pos, 1, lev)),
                       ("trm_adjoint_open", (4,)), ("trm_adjoint_open_checkpointed", (2, 2)), ("trm_adjoint_param_open", ()),
                       ("trm_step_record", (C.c_double(DT), 1))):
        rc, msg = call(d, name, *args)
        if name == "trm_step_record":      # (no adjoint can be open on such a context: that is what it says)
            assert rc == CAPI.TRM_EINVAL and "no adjoint is open" in msg, (name, rc, msg)
        else:
            assert (rc, msg) == (U, f"{name}: {STATE_SEEDS_ONLY}"), (name, rc, msg)
    # what a step refuses: the generic boundary kinds
    d.set_bc("pressure_head", "bottom", "value", -1.0)
    rc, msg = call(d, "trm_step_tangent", C.c_double(DT), 1)
    assert rc == U and msg.startswith("trm_step_tangent: on a Richards context: the branch-free boundary kinds only"), msg


def test_an_upload_of_the_saturation_makes_the_tangent_stale():
    d = small()
    d.set_option("derivative_richards", 1)
    d.open_tangent()
    d.set_tangent("internal_energy", 1.0)
    d.step_tangent(DT, 1)
    d.set("saturation_water_ice", d.get("saturation_water_ice"))
    buf = np.zeros((4, 3))
    assert call(d, "trm_step_tangent", C.c_double(DT), 1)[0] == CAPI.TRM_ESTALE
    assert call(d, "trm_tangent_closure")[0] == CAPI.TRM_ESTALE
    assert call(d, "trm_tangent_download", 4, buf.ctypes.data)[0] == CAPI.TRM_ESTALE
    assert call(d, "trm_tangent_download", 3, buf.ctypes.data)[0] == CAPI.TRM_OK          # (a seed, like dU)
    d.set_tangent("internal_energy", 1.0)
    d.step_tangent(DT, 1)


@pytest.mark.parametrize("hyd", RC.HYDRAULICS)
def test_linear_in_both_seeds(hyd):
    case = (33, 13, hyd, "infiltration_top")
    seed = RC.inputs(case)[4]
    d = device(case)
    once, twice = tangents(d, seed), tangents(d, 2.0 * seed)
    assert np.array_equal(bits(2.0 * once), bits(twice))
    assert np.all(np.isfinite(once)) and all(np.any(once[x] != 0.0) for x in range(5))
    assert np.all(tangents(d, np.zeros_like(seed)) == 0.0)


def test_without_moving_water_it_is_the_heat_only_tangent():
    """K_sat = 0 and dsat = 0: the saturation stays where it is, and dU, dT, dliq are those of the heat-only tangent under the mirror halo
    policy (the Richards halo cell is the edge cell), within 8 x e_ref of the case"""
    Nz, Nh = 33, 13
    p = RC.params("default", K_sat=0.0)
    U0, sat = RC.mixed_state(Nz, Nh, p, 1)
    bcs = {("temperature", "top"): ("value", np.linspace(-4.0, 4.0, Nh)), ("internal_energy", "bottom"): ("flux", np.full(Nh, 0.05))}
    dU = np.random.default_rng(5).normal(0.0, 1e3, (Nz, Nh))
    seed = np.concatenate([dU, np.zeros((Nz, Nh))])
    wide = LR.run([DZ] * Nz, U0, sat, bcs, p, DT, STEPS, dtype=LD)
    narrow = LR.run([DZ] * Nz, U0, sat, bcs, p, DT, STEPS, dtype=np.float64)
    keep = LR.kept_columns(wide, narrow)
    assert keep.sum() >= Nh - 2
    e_ref, _, Ssum = LH.contraction_error(narrow.jacobian()[..., keep], wide.jacobian()[..., keep], seed[:, keep], RC.AXES)
    assert 0.0 < e_ref < 1e-12

    def run(flow):
        q = RC.params("default", K_sat=0.0)
        q.flow = CAPI.FLOW[flow]
        q.halo_policy = CAPI.HALO["mirror"]
        d = trm.DeviceState(trm.ColumnGrid(trm.PrescribedSpacing(dz=[DZ] * Nz), Nh), q)
        d.set_option("steps_per_launch", 4)
        d.set_option("derivative_richards", 1)
        d.set("saturation_water_ice", sat)
        d.set("internal_energy", U0)
        for (var, side), (kind, value) in bcs.items():
            d.set_bc(var, side, kind, value)
        d.closure()
        d.open_tangent()
        d.set_tangent("internal_energy", dU)
        d.step_tangent(DT, STEPS)
        return d

    rich, heat = run("richards"), run("noflow")
    assert np.array_equal(bits(rich.get("saturation_water_ice")), bits(sat)) and np.all(rich.tangent("saturation") == 0.0)
    for x, name in ((0, "internal_energy"), (2, "temperature"), (3, "liquid_water_fraction")):
        a, b = rich.tangent(name)[:, keep], heat.tangent(name)[:, keep]
        zero = Ssum[x] == 0
        assert np.all(a[zero] == 0.0) and np.all(b[zero] == 0.0)
        err = float(np.max(np.abs(a.astype(LD) - b)[~zero] / Ssum[x][~zero])) if (~zero).any() else 0.0
        print(f"{name}: |Richards - heat-only| / S = {err:.3e} (bound {8.0 * e_ref:.3e})")
        assert err <= 8.0 * e_ref, name


@pytest.mark.parametrize("hyd", RC.HYDRAULICS)
def test_closure_tangent(hyd):
    """trm_tangent_closure on a Richards context: dT, dliq and dpsi of the stored state against the reference's closure tangents; and at
    por = 0.5, sat = 0.5 the reference's analytic answer dpsi / dsat = por / swrc'(psi_m) for both retention curves"""
    case = (33, 13, hyd, "infiltration_top")
    Nz, Nh = case[0], case[1]
    p, U0, sat, bcs, seed = RC.inputs(case)
    d = device(case)
    d.open_tangent()
    d.set_tangent("internal_energy", seed[:Nz])
    d.set_tangent("saturation", seed[Nz:])
    d.tangent_closure()
    dev = np.stack([d.tangent(x) for x in TANGENTS])
    wide = LR.run([DZ] * Nz, U0, sat, bcs, p, DT, 0, dtype=LD)
    narrow = LR.run([DZ] * Nz, U0, sat, bcs, p, DT, 0, dtype=np.float64)
    e_ref, ref, Ssum = LH.contraction_error(narrow.jacobian(), wide.jacobian(), seed, RC.AXES)
    zero = Ssum == 0
    assert np.all(dev[zero] == 0.0)
    err = float(np.max(np.abs(dev.astype(LD) - ref)[~zero] / Ssum[~zero]))
    print(f"{hyd}: closure tangents |dev - ref| / S = {err:.3e}, e_ref = {e_ref:.3e}")
    assert 0.0 < e_ref < 1e-13 and err <= 8.0 * e_ref
    # the analytic slope.  The bound: the slope is a power of r = 0.5 times constants, a dozen roundings in either evaluation, and the
    # generic pow is good to an ulp: 64 eps
    q = RC.params(hyd)
    q.por_mineral = 0.5
    a = trm.DeviceState(trm.ColumnGrid(trm.PrescribedSpacing(dz=[DZ] * 4), 2), q)
    a.set_option("derivative_richards", 1)
    a.set("saturation_water_ice", np.full((4, 2), 0.5))
    a.set("internal_energy", np.full((4, 2), 1e6))
    a.closure()
    a.open_tangent()
    a.set_tangent("saturation", 1.0)
    a.tangent_closure()
    slope = RC.analytic_slope(q, 0.5)
    got = a.tangent("pressure_head")
    print(f"{hyd}: dpsi/dsat = {got[0, 0]!r}, por / swrc' = {float(slope)!r}")
    assert np.all(np.abs(got.astype(LD) - slope) <= 64 * np.finfo(np.float64).eps * abs(slope))


def test_jvp_is_the_c_abi_path():
    def build():
        grid = trm.ColumnGrid(trm.ExponentialSpacing(N=10), num_columns=3)
        soil = trm.SoilEnergyWaterCarbon(hydrology=trm.SoilHydrology(vertical_flow=trm.RichardsEq()))
        # (an unsaturated column: the default initializer saturates every cell, where the head has no slope)
        initializer = trm.SoilInitializer(hydrology=trm.ConstantSaturation(0.5))
        return trm.initialize(trm.SoilModel(grid, soil=soil, initializer=initializer), trm.ForwardEuler(dt=60.0))
    a, b = build(), build()
    rng = np.random.default_rng(3)
    dU, dsat = rng.normal(0.0, 1e3, (10, 3)), rng.normal(0.0, 1e-3, (10, 3))
    tan = trm.jvp(a, {"internal_energy": dU, "saturation": dsat}, 5)
    assert set(tan) == set(TANGENTS) and a.state.get_option("derivative_richards") == 0
    st = b.state
    st.set_option("derivative_richards", 1)
    st.open_tangent()
    st.set_tangent("internal_energy", dU)
    st.set_tangent("saturation", dsat)
    st.step_tangent(60.0, 5)
    for name in TANGENTS:
        assert np.array_equal(bits(tan[name]), bits(st.tangent(name))), name
        assert np.all(np.isfinite(tan[name]))
    assert np.any(tan["saturation"] != 0.0) and np.any(tan["pressure_head"] != 0.0)
    # a plain value seeds the internal energy alone: a zero saturation seed; on a heat-only integrator a saturation seed is refused
    zero = trm.jvp(build(), dU, 5)
    assert set(zero) == set(TANGENTS)
    assert np.array_equal(bits(zero["internal_energy"]), bits(trm.jvp(build(), {"internal_energy": dU, "saturation": 0.0}, 5)["internal_energy"]))
    grid = trm.ColumnGrid(trm.ExponentialSpacing(N=10), num_columns=3)
    heat = trm.initialize(trm.SoilModel(grid, initializer=trm.SoilInitializer()), trm.ForwardEuler(dt=60.0))
    with pytest.raises(ValueError, match="saturation seeds need"):
        trm.jvp(heat, {"internal_energy": 1.0, "saturation": dsat}, 1)
    assert set(trm.jvp(heat, 1.0, 1)) == {"internal_energy", "temperature", "liquid_water_fraction"}
