"""Hydraulic-parameter gradients of the heat + Richards adjoint behind TRM_OPT_DERIVATIVE_RICHARDS_PARAMS: what the option opens together
with TRM_OPT_DERIVATIVE_RICHARDS_ADJOINT and what stays refused, the texts with either option at 0, the id rules on both kinds of context,
linearity in the cotangents, invariance under the split into launches and record calls, the accumulators of a second sweep, the empty tape
against the analytic slopes of the retention curve, K_sat = 0, and trm.hydraulic_parameter_gradient against the C ABI.  The value-by-value
comparison with the exact Jacobian is test_gpu_adjoint_richards_params_edges.py."""
import ctypes as C

import numpy as np
import pytest

import linearised_richards_params as LP
import richards_cases as RC
import terrarium_jl_amd as trm
from linearised_richards_params import DT
from test_gpu_adjoint_richards import TAPE_ONLY, still_refused, wet
from test_gpu_adjoint_richards_edges import BY_FIELD, record, sweep
from test_gpu_adjoint_richards_params_edges import PARAMS, param_sweep, params_device
from test_gpu_tangent_richards import HEAT_ONLY, call, small
from test_gpu_tangent_richards_edges import bits

pytestmark = pytest.mark.gpu

CAPI = trm._capi
LD = np.longdouble
CASE33 = (33, 13, "default", "infiltration_top")
IDS = CAPI.HYDRAULIC_PARAMS
NOT_OPEN = "no parameter gradients are open (trm_adjoint_param_open)"


def test_both_options_open_the_parameter_gradients():
    """the test that fails without the feature: trm_adjoint_param_open on a Richards context"""
    d = wet()
    assert d.get_option("derivative_richards_params") == 0
    d.set_option("derivative_richards_adjoint", 1)
    d.set_option("derivative_richards_params", 1)
    assert d.get_option("derivative_richards_params") == 1
    assert call(d, "trm_adjoint_param_open") == (CAPI.TRM_EINVAL, "trm_adjoint_param_open: no adjoint is open (trm_adjoint_open)")
    d.open_adjoint(4)
    buf = np.ones(3)
    assert call(d, "trm_adjoint_param_download", IDS["K_sat"], buf.ctypes.data) == (CAPI.TRM_EINVAL, "trm_adjoint_param_download: " + NOT_OPEN)
    assert call(d, "trm_adjoint_param_open") == (CAPI.TRM_OK, "")
    dev = C.c_void_p()
    first = None
    for at, which in enumerate(IDS.values()):
        assert call(d, "trm_adjoint_param_download", which, buf.ctypes.data)[0] == CAPI.TRM_OK and np.all(buf == 0.0), which
        buf[...] = 1.0
        assert call(d, "trm_adjoint_param_device_ptr", which, C.byref(dev))[0] == CAPI.TRM_OK and dev.value
        first = dev.value if first is None else first
        assert dev.value == first + at * 3 * 8      # [TRM_HYDRAULIC_PARAM_COUNT][num_columns] doubles
    # it does not imply trm_adjoint_bc_open, and nothing else opens with it
    for name, args in still_refused():
        if name != "trm_adjoint_param_open":
            assert call(d, name, *args) == (CAPI.TRM_EUNSUPPORTED, f"{name}: {TAPE_ONLY}"), name
    d.step_record(DT, 3)
    assert "hydraulic_parameter_gradient" not in d.last_program()       # (the record is the one it always was)
    # (not a uniform cotangent: the column's water content does not depend on K_sat)
    d.set_cotangent("saturation", np.random.default_rng(5).normal(size=(4, 3)))
    d.adjoint_backward()
    prog = d.last_program()
    assert prog["family"] == "column_adjoint_richards" and prog["hydraulic_parameter_gradient"] is True and prog["hydraulics"] == "default"
    grads = {name: d.param_gradient(name) for name in PARAMS}
    assert all(np.all(np.isfinite(g)) for g in grads.values()) and np.any(grads["K_sat"] != 0.0)
    for name in LP.unread("default"):
        assert np.all(grads[name] == 0.0), name
    # trm_adjoint_close frees them: a new adjoint starts without
    d.close_adjoint()
    d.open_adjoint(2)
    assert call(d, "trm_adjoint_param_download", IDS["K_sat"], buf.ctypes.data) == (CAPI.TRM_EINVAL, "trm_adjoint_param_download: " + NOT_OPEN)


@pytest.mark.parametrize("adjoint_option, params_option", ((1, 0), (0, 1), (0, 0)))
def test_with_either_option_at_zero_every_answer_is_todays(adjoint_option, params_option):
    d = wet()
    d.set_option("derivative_richards_adjoint", adjoint_option)
    d.set_option("derivative_richards_params", params_option)
    buf, dev = np.zeros(3), C.c_void_p()
    U = CAPI.TRM_EUNSUPPORTED
    if not adjoint_option:
        assert call(d, "trm_adjoint_open", 4) == (U, "trm_adjoint_open: " + HEAT_ONLY)
        assert call(d, "trm_adjoint_param_open") == (U, "trm_adjoint_param_open: " + HEAT_ONLY)
        for name, arg in (("trm_adjoint_param_download", buf.ctypes.data), ("trm_adjoint_param_device_ptr", C.byref(dev))):
            rc, msg = call(d, name, IDS["K_sat"], arg)
            assert rc == CAPI.TRM_EINVAL and "no adjoint is open" in msg, (name, msg)
        return
    for opened in (False, True):
        if opened:
            d.open_adjoint(4)
        for name, args in still_refused():
            assert call(d, name, *args) == (U, f"{name}: {TAPE_ONLY}"), name
    for which in (0, IDS["K_sat"]):
        assert call(d, "trm_adjoint_param_download", which, buf.ctypes.data) == (CAPI.TRM_EINVAL, "trm_adjoint_param_download: " + NOT_OPEN)
        assert call(d, "trm_adjoint_param_device_ptr", which, C.byref(dev)) == (CAPI.TRM_EINVAL, "trm_adjoint_param_device_ptr: " + NOT_OPEN)
    d.step_record(DT, 2)
    d.set_cotangent("saturation", 1.0)
    d.adjoint_backward()
    assert "hydraulic_parameter_gradient" not in d.last_program()


def test_the_id_rules_on_both_kinds_of_context():
    d = wet()
    d.set_option("derivative_richards_adjoint", 1)
    d.set_option("derivative_richards_params", 1)
    d.open_adjoint(2)
    d.open_param_gradient()
    buf, dev = np.zeros(3), C.c_void_p()
    calls = (("trm_adjoint_param_download", buf.ctypes.data), ("trm_adjoint_param_device_ptr", C.byref(dev)))
    for name, arg in calls:
        for which in list(range(len(CAPI.THERMAL_PARAMS))) + [-1, 17, 26]:
            rc, msg = call(d, name, which, arg)
            assert rc == CAPI.TRM_EINVAL and msg.startswith(name + ": bad argument"), (name, which, msg)
        rc, msg = call(d, name, IDS["K_sat"], None)
        assert rc == CAPI.TRM_EINVAL and msg.startswith(name + ": bad argument"), (name, msg)
        for which in IDS.values():
            assert call(d, name, which, arg)[0] == CAPI.TRM_OK, (name, which)
    with pytest.raises(CAPI.TerrariumHipError, match="bad argument"):
        d.param_gradient("k_water")         # (the thermal names are the thermal ids)
    # a NoFlow context: the thermal ids as ever, the hydraulic ids a bad argument -- with the options or without
    for option in (0, 1):
        h = small("noflow")
        h.set_option("derivative_richards_adjoint", option)
        h.set_option("derivative_richards_params", option)
        h.open_adjoint(2)
        h.open_param_gradient()
        for name, arg in calls:
            for which in IDS.values():
                rc, msg = call(h, name, which, arg)
                assert rc == CAPI.TRM_EINVAL and msg.startswith(name + ": bad argument"), (name, which, msg)
            for which in range(len(CAPI.THERMAL_PARAMS)):
                assert call(h, name, which, arg)[0] == CAPI.TRM_OK, (name, which)
        assert call(h, "trm_adjoint_bc_open")[0] == CAPI.TRM_OK


@pytest.mark.parametrize("hyd", RC.HYDRAULICS)
def test_linear_in_the_cotangents(hyd):
    case = (33, 13, hyd, "infiltration_top")
    w = LP.cotangents(case)["dense"]
    d = params_device(case)
    (_, once), (_, twice) = param_sweep(d, w), param_sweep(d, 2.0 * w)
    for name in PARAMS:
        assert np.array_equal(bits(2.0 * once[name]), bits(twice[name])), name
        assert np.all(np.isfinite(once[name])), name
        assert np.any(once[name] != 0.0) == (name not in LP.unread(hyd)), name
    state, zeros = param_sweep(d, np.zeros_like(w))
    for g in list(state) + list(zeros.values()):
        assert np.all(g == 0.0)


def test_the_split_into_launches_and_calls_changes_no_bit():
    w = LP.cotangents(CASE33)["dense"]
    whole = param_sweep(params_device(CASE33), w)[1]
    others = (param_sweep(params_device(CASE33, steps_per_launch=6), w)[1], param_sweep(params_device(CASE33), w, ((DT, 3), (DT, 3)))[1])
    for other in others:
        for name in PARAMS:
            assert np.array_equal(bits(whole[name]), bits(other[name])), name
    assert np.any(whole["K_sat"] != 0.0)


def test_a_second_sweep_starts_from_zeroed_accumulators():
    w = LP.cotangents(CASE33)["dense"]
    d = params_device(CASE33)
    first = param_sweep(d, w)[1]
    # (record opens the adjoint anew: trm_adjoint_open keeps the accumulators, zeroed -- no trm_adjoint_param_open in between)
    record(d)
    assert all(np.all(d.param_gradient(name) == 0.0) for name in PARAMS)
    sweep(d, w)
    assert d.last_program()["hydraulic_parameter_gradient"] is True
    for name in PARAMS:
        assert np.array_equal(bits(first[name]), bits(d.param_gradient(name))), name


def analytic_slopes(p, sat):
    """{name: dpsi_m/dp} of the retention curve at theta = sat por, in extended precision"""
    por, res, theta = LD(RC.porosity(p)), LD(p.theta_res), LD(sat) * LD(RC.porosity(p))
    span = por - res
    r = (theta - res) / span
    dr = (r - 1) / span
    out = {name: np.zeros_like(r) for name in PARAMS}
    if p.swrc == CAPI.SWRC["van_genuchten"]:
        n, alpha = LD(p.vg_n), LD(p.vg_alpha)
        a, b = -n / (n - 1), 1 / n
        u = r ** a
        g = (u - 1) ** b
        out["theta_res"] = -1 / alpha * b * g / (u - 1) * a * u / r * dr
        out["vg_alpha"] = g / alpha ** 2
        du = u * np.log(r) / (n - 1) ** 2
        out["vg_n"] = -1 / alpha * g * (-np.log(u - 1) / n ** 2 + b * du / (u - 1))
    else:
        lam, psi_s = LD(p.bc_lambda), LD(p.bc_psi_s)
        ra = r ** (-1 / lam)
        out["theta_res"] = -psi_s * (-1 / lam) * ra / r * dr
        out["bc_psi_s"] = -ra
        out["bc_lambda"] = -psi_s * ra * np.log(r) / lam ** 2
    return out


@pytest.mark.parametrize("hyd", RC.HYDRAULICS)
def test_empty_tape_gives_the_slopes_of_the_retention_curve(hyd):
    """no taped step: the gradient is the fold's wpsi dpsi/dp at the stored saturation, one product per column under a one-hot wpsi"""
    case = (33, 13, hyd, "infiltration_top")
    Nz, Nh = case[0], case[1]
    d = params_device(case)
    d.restore_state()
    d.open_adjoint(1)
    d.open_param_gradient()
    sat = d.get("saturation_water_ice")
    for level in (0, 17, Nz - 1):
        w = np.zeros((5, Nz, Nh))
        w[BY_FIELD.index("pressure_head"), level] = 1.0
        sweep(d, w)
        assert d.adjoint_tape() == (0, 1) and d.last_program()["hydraulic_parameter_gradient"] is True
        expected = analytic_slopes(RC.inputs(case)[0], sat[level])
        for name in PARAMS:
            got = d.param_gradient(name)
            if np.all(expected[name] == 0):
                assert np.all(got == 0.0), name
            else:
                np.testing.assert_allclose(got, expected[name].astype(np.float64), rtol=1e-13, atol=0.0, err_msg=f"{name} at level {level}")
                assert np.all(got != 0.0), name


def test_k_sat_zero_has_a_finite_gradient():
    """dKc/dK_sat = water / por whatever K_sat is: at K_sat = 0 no water moves, and dL/dK_sat is finite and the restatement's, within
    8 x e_ref of the restatement of this very run (13 columns)"""
    case = CASE33
    p = RC.params("default", K_sat=0.0)
    _, U0, sat, bcs, _ = RC.inputs(case)
    # (no branch mask: with K_sat = 0 every conductivity is 0 and every face minimum a tie, in float64 and in extended precision alike;
    #  the restatement takes the second operand there, as Base.min, and so does the sweep)
    ref = LP.Reference(case, inputs=(p, U0, sat, bcs), mask=False)
    assert ref.keep.all() and 0.0 < ref.e_ref < 1e-11
    d = trm.DeviceState(trm.ColumnGrid(trm.PrescribedSpacing(dz=[LP.DZ] * case[0]), case[1]), p)
    d.set_option("steps_per_launch", LP.SPL)
    d.set_option("derivative_richards_adjoint", 1)
    d.set_option("derivative_richards_params", 1)
    d.set("saturation_water_ice", sat)
    d.set("internal_energy", U0)
    for (var, side), (kind, value) in bcs.items():
        d.set_bc(var, side, kind, value)
    d.closure()
    d.save_state()
    for label in ("dense", "one-hot saturation 0", "one-hot internal_energy 32"):
        _, grads = param_sweep(d, LP.cotangents(case)[label])
        assert np.all(np.isfinite(grads["K_sat"]))
        err = ref.error(label, grads)
        print(f"{label}: device = {err:.3e}, e_ref = {ref.parts[label]:.3e}, bound = {8.0 * ref.e_ref:.3e}")
        assert err <= 8.0 * ref.e_ref, label
    assert np.any(ref.expected["dense"][1][PARAMS.index("K_sat")] > 0) and np.any(grads["K_sat"] != 0.0)


def test_hydraulic_parameter_gradient_is_the_c_abi_path():
    def build():
        grid = trm.ColumnGrid(trm.ExponentialSpacing(N=10), num_columns=3)
        soil = trm.SoilEnergyWaterCarbon(hydrology=trm.SoilHydrology(vertical_flow=trm.RichardsEq()))
        initializer = trm.SoilInitializer(hydrology=trm.ConstantSaturation(0.5))
        return trm.initialize(trm.SoilModel(grid, soil=soil, initializer=initializer), trm.ForwardEuler(dt=60.0))
    a, b = build(), build()
    rng = np.random.default_rng(3)
    w = {name: rng.normal(size=(10, 3)) * scale for name, scale in zip(BY_FIELD, (1e-6, 1.0, 1e-1, 1.0, 1e-2))}
    state, grads = trm.hydraulic_parameter_gradient(a, 5, w)
    assert set(state) == {"internal_energy", "saturation"} and tuple(grads) == PARAMS
    assert a.state.get_option("derivative_richards_adjoint") == 0 and a.state.get_option("derivative_richards_params") == 0
    st = b.state
    st.set_option("derivative_richards_adjoint", 1)
    st.set_option("derivative_richards_params", 1)
    st.open_adjoint(5)
    st.step_record(60.0, 5)
    for name in BY_FIELD:
        st.set_cotangent(name, w[name])
    st.open_param_gradient()
    st.adjoint_backward()
    for name in state:
        assert np.array_equal(bits(state[name]), bits(st.cotangent(name))), name
    for name in PARAMS:
        assert grads[name].shape == (3,) and np.array_equal(bits(grads[name]), bits(st.param_gradient(name))), name
    assert np.any(grads["K_sat"] != 0.0) and np.all(grads["vg_n"] == 0.0)
    # the state gradients are vjp's, and vjp keeps refusing wrt_params there
    plain = trm.vjp(build(), 5, internal_energy=w)
    for name in state:
        assert np.array_equal(bits(state[name]), bits(plain[name])), name
    with pytest.raises(ValueError, match="on an integrator with RichardsEq"):
        trm.vjp(build(), 5, internal_energy=1.0, wrt_params=True)
    with pytest.raises(KeyError, match="hydraulic_conductivity"):
        trm.hydraulic_parameter_gradient(build(), 1, {"hydraulic_conductivity": 1.0})
    grid = trm.ColumnGrid(trm.ExponentialSpacing(N=10), num_columns=3)
    heat = trm.initialize(trm.SoilModel(grid, initializer=trm.SoilInitializer()), trm.ForwardEuler(dt=60.0))
    with pytest.raises(ValueError, match="needs an integrator with RichardsEq"):
        trm.hydraulic_parameter_gradient(heat, 1, {"internal_energy": 1.0})
