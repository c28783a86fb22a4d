"""Reverse-mode gradients of the heat + Richards run behind TRM_OPT_DERIVATIVE_RICHARDS_ADJOINT: what the option opens and what stays
refused, the texts with the option at 0, linearity in the five cotangents, invariance under the split into launches and record calls, two
record calls with different dt, the empty tape against the closure tangents, agreement with the heat-only adjoint where no water moves, the
staleness rules, and trm.vjp against the C ABI.  The value-by-value comparison with the exact Jacobian is
test_gpu_adjoint_richards_edges.py."""
import ctypes as C

import numpy as np
import pytest

import linearised_heat as LH
import linearised_richards as LR
import richards_adjoint_cases as RA
import richards_cases as RC
import terrarium_jl_amd as trm
from richards_adjoint_cases import DT, DZ, STEPS
from test_gpu_adjoint_richards_edges import BY_FIELD, adjoint_device, gradients, record, sweep
from test_gpu_tangent_richards import HEAT_ONLY, STATE_SEEDS_ONLY, call, small
from test_gpu_tangent_richards_edges import TANGENTS, bits

pytestmark = pytest.mark.gpu

CAPI = trm._capi
LD = np.longdouble
TAPE_ONLY = "on a Richards context: final-state cotangents on a per-step tape only"
CASE33 = (33, 13, "default", "infiltration_top")


def still_refused():
    """(name, args) of the calls that refuse a Richards context with the option set"""
    buf = np.zeros(16)
    pos, lev = (C.c_int32 * 1)(1), (C.c_int32 * 1)(0)
    dev, n32, n64 = C.c_void_p(), C.c_int32(), C.c_int64()
    return (("trm_adjoint_open_checkpointed", (2, 2)), ("trm_adjoint_bc_open", ()), ("trm_adjoint_param_open", ()),
            ("trm_adjoint_observe", (0, 1, lev, buf.ctypes.data)), ("trm_adjoint_observe_misfit", (1, lev, buf.ctypes.data, None)),
            ("trm_adjoint_observe_record", (1, pos, 1, lev, buf.ctypes.data, None)),
            ("trm_adjoint_observe_record_device", (1, pos, 1, lev, buf.ctypes.data, None)), ("trm_adjoint_record_detach", ()),
            ("trm_adjoint_record_residual_download", (buf.ctypes.data,)), ("trm_adjoint_record_residual_device_ptr", (C.byref(dev),)),
            ("trm_adjoint_record_misfit_download", (buf.ctypes.data,)), ("trm_adjoint_record_info", (C.byref(n32), C.byref(n32), C.byref(n64))))


def wet(saturation=0.8):
    """the 4 x 3 context with an unsaturated column: `small` leaves the saturation at zero, where the Brooks-Corey head is infinite"""
    d = small()
    d.set("saturation_water_ice", saturation)
    d.initialize()
    return d


def test_the_option_opens_a_richards_context():
    """the test that fails without the feature: trm_adjoint_open on a Richards context"""
    d = wet()
    assert d.get_option("derivative_richards_adjoint") == 0 and d.get_option("derivative_richards") == 0
    d.set_option("derivative_richards_adjoint", 1)
    assert call(d, "trm_adjoint_open", 4) == (CAPI.TRM_OK, "")
    buf = np.ones((4, 3))
    for which in range(5):
        assert call(d, "trm_adjoint_download", which, buf.ctypes.data)[0] == CAPI.TRM_OK, which
        assert np.all(buf == 0.0)
        buf[...] = 1.0
    dev, pitch = C.c_void_p(), C.c_int64()
    for which in range(5):
        assert call(d, "trm_adjoint_device_ptr", which, C.byref(dev), C.byref(pitch))[0] == CAPI.TRM_OK and dev.value
        assert call(d, "trm_adjoint_upload", which, buf.ctypes.data)[0] == CAPI.TRM_OK, which
    for name in ("trm_adjoint_upload", "trm_adjoint_download"):
        assert call(d, name, 5, buf.ctypes.data) == (CAPI.TRM_EINVAL, name + ": bad argument")
    assert d.adjoint_tape() == (0, 4)
    assert call(d, "trm_step_record", C.c_double(DT), 3)[0] == CAPI.TRM_OK and d.adjoint_tape() == (3, 4)
    prog = d.last_program()
    assert prog["family"] == "column_adjoint_richards" and prog["hydraulics"] == "default" and prog["lanes_per_column"] == 32
    assert call(d, "trm_adjoint_backward")[0] == CAPI.TRM_OK and d.adjoint_tape() == (0, 4)
    assert d.last_program()["family"] == "column_adjoint_richards"
    assert np.all(np.isfinite(d.cotangent("internal_energy"))) and np.any(d.cotangent("saturation") != 0.0)
    for name in ("temperature", "liquid_water_fraction", "pressure_head"):
        assert np.all(d.cotangent(name) == 0.0), name
    # the tangent calls still need their own option; a tangent and an adjoint may be open at once
    assert call(d, "trm_tangent_open") == (CAPI.TRM_EUNSUPPORTED, "trm_tangent_open: " + HEAT_ONLY)
    d.set_option("derivative_richards", 1)
    assert call(d, "trm_tangent_open")[0] == CAPI.TRM_OK
    assert call(d, "trm_adjoint_close")[0] == CAPI.TRM_OK
    assert call(d, "trm_adjoint_tape", None, None) == (CAPI.TRM_EINVAL, "trm_adjoint_tape: no adjoint is open (trm_adjoint_open)")


@pytest.mark.parametrize("tangent_option", (0, 1))
def test_with_the_option_at_zero_every_answer_is_todays(tangent_option):
    d = small()
    d.set_option("derivative_richards", tangent_option)
    why = STATE_SEEDS_ONLY if tangent_option else HEAT_ONLY
    U = CAPI.TRM_EUNSUPPORTED
    assert call(d, "trm_adjoint_open", 4) == (U, "trm_adjoint_open: " + why)
    assert call(d, "trm_adjoint_open_checkpointed", 2, 2) == (U, "trm_adjoint_open_checkpointed: " + why)
    assert call(d, "trm_adjoint_param_open") == (U, "trm_adjoint_param_open: " + why)
    for name, args in (("trm_step_record", (C.c_double(DT), 1)), ("trm_adjoint_backward", ()), ("trm_adjoint_bc_open", ()), ("trm_adjoint_close", ())):
        rc, msg = call(d, name, *args)
        assert rc == CAPI.TRM_EINVAL and "no adjoint is open" in msg, (name, rc, msg)
    for name, args in still_refused()[3:]:
        rc, msg = call(d, name, *args)
        assert rc == CAPI.TRM_EINVAL and "no adjoint is open" in msg, (name, rc, msg)
    # a NoFlow context has three cotangent fields, with the option or without it
    for option in (0, 1):
        h = small("noflow")
        h.set_option("derivative_richards_adjoint", option)
        h.open_adjoint(2)
        buf = np.zeros((4, 3))
        dev, pitch = C.c_void_p(), C.c_int64()
        for which in (3, 4):
            assert call(h, "trm_adjoint_upload", which, buf.ctypes.data) == (CAPI.TRM_EINVAL, "trm_adjoint_upload: bad argument")
            assert call(h, "trm_adjoint_download", which, buf.ctypes.data) == (CAPI.TRM_EINVAL, "trm_adjoint_download: bad argument")
            assert call(h, "trm_adjoint_device_ptr", which, C.byref(dev), C.byref(pitch)) == (CAPI.TRM_EINVAL, "trm_adjoint_device_ptr: bad argument")
        # ... and the calls a Richards context is refused work there as before
        assert call(h, "trm_adjoint_bc_open")[0] == CAPI.TRM_OK and call(h, "trm_adjoint_param_open")[0] == CAPI.TRM_OK
        assert call(h, "trm_adjoint_open_checkpointed", 2, 2)[0] == CAPI.TRM_OK


@pytest.mark.parametrize("opened", (False, True))
def test_the_other_adjoint_families_still_refuse_a_richards_context(opened):
    d = small()
    d.set_option("derivative_richards_adjoint", 1)
    if opened:
        d.open_adjoint(2)
    for name, args in still_refused():
        assert call(d, name, *args) == (CAPI.TRM_EUNSUPPORTED, f"{name}: {TAPE_ONLY}"), name
    if not opened:      # (refused before anything is allocated: no adjoint came to be open)
        assert call(d, "trm_adjoint_tape", None, None)[0] == CAPI.TRM_EINVAL
    else:
        assert d.adjoint_checkpoints() == (0, 0, 2)
    # what a step refuses: the generic boundary kinds
    if opened:
        d.set_bc("pressure_head", "bottom", "value", -1.0)
        rc, msg = call(d, "trm_step_record", C.c_double(DT), 1)
        assert rc == CAPI.TRM_EUNSUPPORTED and msg.startswith("trm_step_record: on a Richards context: the branch-free boundary kinds only"), msg


@pytest.mark.parametrize("hyd", RC.HYDRAULICS)
def test_linear_in_the_cotangents(hyd):
    case = (33, 13, hyd, "infiltration_top")
    w = RA.cotangents(case)["dense"]
    d = adjoint_device(case)
    once, twice = gradients(d, w), gradients(d, 2.0 * w)
    for a, b in zip(once, twice):
        assert np.array_equal(bits(2.0 * a), bits(b))
        assert np.all(np.isfinite(a)) and np.any(a != 0.0)
    for g in gradients(d, np.zeros_like(w)):
        assert np.all(g == 0.0)


def test_the_split_into_launches_and_calls_changes_no_bit():
    w = RA.cotangents(CASE33)["dense"]
    whole = gradients(adjoint_device(CASE33), w)
    for other in (gradients(adjoint_device(CASE33, steps_per_launch=6), w), gradients(adjoint_device(CASE33), w, ((DT, 3), (DT, 3)))):
        for a, b in zip(whole, other):
            assert np.array_equal(bits(a), bits(b))


def test_two_record_calls_are_pulled_back_with_their_own_dt():
    schedule = ((DT, 3), (DT / 2, 3))
    ref = RA.Reference(CASE33, schedule=list(schedule))
    bound = ref.bound(RA.BROKEN)
    d = adjoint_device(CASE33)
    for label in ("dense", "one-hot saturation 0", "one-hot pressure_head 32"):
        gU, gsat = gradients(d, RA.cotangents(CASE33)[label], schedule)
        err = ref.error(label, gU, gsat)
        print(f"{label}: device = {err:.3e}, e_ref = {ref.parts[label]:.3e}, bound = {bound:.3e}")
        assert err <= bound, label
    # ... and they are not the gradients of six equal steps
    assert not np.array_equal(gradients(d, RA.cotangents(CASE33)["dense"], schedule)[0], gradients(d, RA.cotangents(CASE33)["dense"])[0])


@pytest.mark.parametrize("hyd", RC.HYDRAULICS)
def test_empty_tape_is_the_transpose_of_the_closures(hyd):
    """J_closure from trm_tangent_closure under one-hot seeds; one cotangent field at a time, so that a gradient is one product per cell
    and carries the rounding of one chain of multiplications: rtol 1e-14, the figure of the heat-only test"""
    case = (33, 13, hyd, "infiltration_top")
    Nz, Nh = case[0], case[1]
    d = adjoint_device(case)
    d.set_option("derivative_richards", 1)
    d.open_tangent()
    J = np.zeros((5, Nz, 2 * Nz, Nh))
    for j in range(2 * Nz):
        seed = np.zeros((2 * Nz, Nh))
        seed[j] = 1.0
        d.set_tangent("internal_energy", seed[:Nz])
        d.set_tangent("saturation", seed[Nz:])
        d.tangent_closure()
        J[:, :, j, :] = np.stack([d.tangent(x) for x in TANGENTS])
    assert all(np.any(J[x] != 0.0) for x in range(5))
    rng = np.random.default_rng(23)
    d.open_adjoint(1)
    for x, name in enumerate(BY_FIELD):
        w = np.zeros((5, Nz, Nh))
        w[x] = rng.uniform(0.5, 1.5, (Nz, Nh)) * RA.SCALES[x]
        gU, gsat = sweep(d, w)
        assert d.adjoint_tape() == (0, 1)
        np.testing.assert_allclose(np.concatenate([gU, gsat]), np.einsum(RA.AXES, J, w), rtol=1e-14, atol=0.0, err_msg=name)
        for other in ("temperature", "liquid_water_fraction", "pressure_head"):
            assert np.all(d.cotangent(other) == 0.0)          # folded in
    assert d.last_program()["family"] == "column_adjoint_richards"


def test_without_moving_water_it_is_the_heat_only_gradient():
    """K_sat = 0, wsat = wpsi = 0: gU within the bound of the restatement of this state; whether it is the NoFlow adjoint's bit for bit is
    printed, not asserted"""
    Nz, Nh = 33, 13
    p = RC.params("default", K_sat=0.0)
    U0, sat = RC.mixed_state(Nz, Nh, p, 1)
    bcs = {("temperature", "top"): ("value", np.linspace(-4.0, 4.0, Nh)), ("internal_energy", "bottom"): ("flux", np.full(Nh, 0.05))}
    w = RA.cotangents(CASE33)["dense"].copy()
    w[1] = 0.0
    w[4] = 0.0
    wide = LR.run([DZ] * Nz, U0, sat, bcs, p, DT, STEPS, dtype=LD)
    narrow = LR.run([DZ] * Nz, U0, sat, bcs, p, DT, STEPS, dtype=np.float64)
    keep = LR.kept_columns(wide, narrow)
    assert keep.sum() >= Nh - 2
    e_ref, ref, Ssum = LH.contraction_error(narrow.jacobian()[..., keep], wide.jacobian()[..., keep], w[..., keep], RA.AXES)
    assert 0.0 < e_ref < 1e-12

    def run(flow):
        q = RC.params("default", K_sat=0.0)
        q.flow = CAPI.FLOW[flow]
        q.halo_policy = CAPI.HALO["mirror"]
        d = trm.DeviceState(trm.ColumnGrid(trm.PrescribedSpacing(dz=[DZ] * Nz), Nh), q)
        d.set_option("steps_per_launch", 4)
        d.set_option("derivative_richards_adjoint", 1)
        d.set("saturation_water_ice", sat)
        d.set("internal_energy", U0)
        for (var, side), (kind, value) in bcs.items():
            d.set_bc(var, side, kind, value)
        d.closure()
        d.open_adjoint(STEPS)
        d.step_record(DT, STEPS)
        for name, field in zip(BY_FIELD, w):
            if flow == "richards" or name not in ("saturation", "pressure_head"):
                d.set_cotangent(name, field)
        d.adjoint_backward()
        return d.cotangent("internal_energy")

    rich, heat = run("richards"), run("noflow")
    zero = Ssum[:Nz] == 0
    dev = rich[:, keep]
    assert np.all(dev[zero] == 0.0)
    err = float(np.max(np.abs(dev.astype(LD) - ref[:Nz])[~zero] / Ssum[:Nz][~zero]))
    print(f"gU: |Richards - restatement| / S = {err:.3e} (bound {8.0 * e_ref:.3e}); bit-identical to the NoFlow adjoint's: {np.array_equal(bits(rich), bits(heat))}")
    assert err <= 8.0 * e_ref


def test_staleness_and_the_tape_capacity():
    d = small()
    d.set_option("derivative_richards_adjoint", 1)
    d.set_option("derivative_richards", 1)
    d.open_adjoint(3)
    rc, msg = call(d, "trm_step_record", C.c_double(DT), 4)
    assert rc == CAPI.TRM_EINVAL and "do not fit the tape" in msg and d.adjoint_tape() == (0, 3)
    d.step_record(DT, 2)
    d.set("saturation_water_ice", d.get("saturation_water_ice"))
    assert call(d, "trm_step_record", C.c_double(DT), 1)[0] == CAPI.TRM_ESTALE
    assert call(d, "trm_adjoint_backward")[0] == CAPI.TRM_ESTALE
    d.open_adjoint(3)
    d.open_tangent()
    d.step_record(DT, 1)
    d.set_tangent("internal_energy", 1.0)
    d.step_tangent(DT, 1)
    assert call(d, "trm_step_record", C.c_double(DT), 1)[0] == CAPI.TRM_ESTALE
    assert call(d, "trm_adjoint_backward")[0] == CAPI.TRM_ESTALE
    # a fresh tape works again, and a step_record is a state-changing call for the open tangent
    d.open_adjoint(3)
    d.step_record(DT, 1)
    assert call(d, "trm_step_tangent", C.c_double(DT), 1)[0] == CAPI.TRM_ESTALE
    d.adjoint_backward()


def test_vjp_is_the_c_abi_path():
    def build():
        grid = trm.ColumnGrid(trm.ExponentialSpacing(N=10), num_columns=3)
        soil = trm.SoilEnergyWaterCarbon(hydrology=trm.SoilHydrology(vertical_flow=trm.RichardsEq()))
        initializer = trm.SoilInitializer(hydrology=trm.ConstantSaturation(0.5))
        return trm.initialize(trm.SoilModel(grid, soil=soil, initializer=initializer), trm.ForwardEuler(dt=60.0))
    a, b = build(), build()
    rng = np.random.default_rng(3)
    w = {name: rng.normal(size=(10, 3)) * scale for name, scale in zip(BY_FIELD, RA.SCALES)}
    g = trm.vjp(a, 5, temperature=w["temperature"], internal_energy={k: v for k, v in w.items() if k != "temperature"})
    assert set(g) == {"internal_energy", "saturation"} and a.state.get_option("derivative_richards_adjoint") == 0
    st = b.state
    st.set_option("derivative_richards_adjoint", 1)
    st.open_adjoint(5)
    st.step_record(60.0, 5)
    for name in BY_FIELD:
        st.set_cotangent(name, w[name])
    st.adjoint_backward()
    for name in g:
        assert np.array_equal(bits(g[name]), bits(st.cotangent(name))), name
        assert np.all(np.isfinite(g[name])) and np.any(g[name] != 0.0)
    # the transpose of jvp there: <w, J v> = <J^T w, v>
    v = {"internal_energy": rng.normal(0.0, 1e3, (10, 3)), "saturation": rng.normal(0.0, 1e-3, (10, 3))}
    tan = trm.jvp(build(), v, 5)
    left = sum(float(np.sum(w[name].astype(LD) * tan[name])) for name in BY_FIELD)
    right = sum(float(np.sum(g[name].astype(LD) * v[name])) for name in g)
    scale = sum(float(np.sum(np.abs(w[name] * tan[name]))) for name in BY_FIELD)
    assert abs(left - right) <= 1e-9 * scale, (left, right, scale)
    # a plain value is the cotangent of the internal energy alone
    plain = trm.vjp(build(), 5, internal_energy=w["internal_energy"])
    assert set(plain) == {"internal_energy", "saturation"}
    for kwargs in (dict(checkpoint_every=2), dict(wrt_boundary=True), dict(wrt_params=True)):
        with pytest.raises(ValueError, match="on an integrator with RichardsEq"):
            trm.vjp(build(), 5, internal_energy=1.0, **kwargs)
    grid = trm.ColumnGrid(trm.ExponentialSpacing(N=10), num_columns=3)
    heat = trm.initialize(trm.SoilModel(grid, initializer=trm.SoilInitializer()), trm.ForwardEuler(dt=60.0))
    for name in ("saturation", "pressure_head"):
        with pytest.raises(ValueError, match="need an integrator with RichardsEq"):
            trm.vjp(heat, 1, internal_energy={name: 1.0})
    assert trm.vjp(heat, 1, internal_energy=1.0).shape == (10, 3)
