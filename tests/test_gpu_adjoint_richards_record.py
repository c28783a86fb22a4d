"""Soil-moisture records on the heat + Richards adjoint behind TRM_OPT_DERIVATIVE_RICHARDS_RECORD (together with
TRM_OPT_DERIVATIVE_RICHARDS_ADJOINT): a record of saturations attached once and read inside the backward launches, with or without the
hydraulic-parameter gradients.

Against the reference of tests/richards_record.py on every case: gU, gsat, the seven parameter gradients and the per-column misfit, each
within its derived bound on the kept columns, exact zeros where S is zero.  Without a tolerance, bit for bit: null records, doubled
weights, the host's resummation of the residuals, the split into launches and record calls, the parameter gradient open or not, two
rounds on one attachment, the detach, the device-pointer attach, the primal against a trm_step twin, TRM_INFO_LAST_PROGRAM.  The adjoint
identity against trm_step_tangent stopped at the record's positions.  The gates with either option at 0, what stays refused, a NoFlow
context, and trm.soil_moisture_gradient against the C path.

Largest device error to bound ratio measured per part over the 52 cases: see DESIGN 4.8 "Richards records"."""
import ctypes as C

import numpy as np
import pytest

import linearised_richards as LR
import richards_adjoint_cases as RA
import richards_cases as RC
import richards_record as RR
import terrarium_jl_amd as trm
from richards_record import DT, STEPS
from test_gpu_adjoint_richards import TAPE_ONLY, still_refused, wet
from test_gpu_adjoint_richards_edges import BY_FIELD, adjoint_device, record, sweep
from test_gpu_tangent_richards import call, small
from test_gpu_tangent_richards_edges import STATE, TANGENTS, bits, stepped_twin

pytestmark = pytest.mark.gpu

CAPI = trm._capi
LD = np.longdouble
PARAMS = tuple(CAPI.HYDRAULIC_PARAMS)
RECORD_CALLS = ("trm_adjoint_observe_record", "trm_adjoint_observe_record_device", "trm_adjoint_record_detach", "trm_adjoint_record_residual_download",
                "trm_adjoint_record_residual_device_ptr", "trm_adjoint_record_misfit_download", "trm_adjoint_record_info")
CASE33 = ("edges", (33, 13, "default", "infiltration_top"))
SOME = [CASE33, ("edges", (32, 13, "generic", "T_top+flux_bottom")), ("dense", (3, 13, "default", "repair")), ("ends", (2, 13, "vg_n2", "infiltration_top"))]


def record_device(case, steps_per_launch=RR.SPL, params=True):
    d = adjoint_device(case, steps_per_launch=steps_per_launch)
    d.set_option("derivative_richards_record", 1)
    d.set_option("derivative_richards_params", 1 if params else 0)
    return d


def attach(d, rec, device_arrays=False):
    if not device_arrays:
        return d.attach_record(rec["positions"], rec["levels"], rec["observed"], rec["weight"])
    import torch
    on = torch.device("cuda", int(d.grid.device))
    observed, weight = (torch.as_tensor(np.ascontiguousarray(rec[key], dtype=np.float64), device=on) for key in ("observed", "weight"))
    torch.cuda.synchronize(on)
    return d.attach_record(rec["positions"], rec["levels"], observed, weight)


def arm_and_sweep(d, w, params, rec):
    """the taped run pulled back under the final cotangent w [5][Nz][Nh]: {state [2 Nz][Nh], params [7][Nh], misfit, residuals}"""
    if params:
        d.open_param_gradient()
    gU, gsat = sweep(d, w)
    out = dict(state=np.concatenate([gU, gsat]))
    if params:
        out["params"] = np.stack([d.param_gradient(name) for name in PARAMS])
    if rec is not None:
        out["misfit"], out["residuals"] = d.record_misfit(), d.record_residuals()
    return out


def record_sweep(d, rec, w, schedule=((DT, STEPS),), params=True):
    """the saved state taped under the schedule on a fresh tape, `rec` (None: no record) attached to it, pulled back"""
    record(d, schedule)
    if rec is not None:
        attach(d, rec)
    return arm_and_sweep(d, w, params, rec)


def same(a, b, what):
    assert a.keys() == b.keys(), what
    for key in a:
        assert np.array_equal(bits(a[key]), bits(b[key])), (what, key)


# ---- 1. against the reference ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rcase", RR.CASES, ids=RR.record_id)
def test_gradients_and_misfit_match_the_reference(rcase):
    ref = RR.reference(rcase)
    case, rec = rcase[1], ref.record
    bounds = {part: RR.bound(rcase, part) for part in RR.PARTS}
    d = record_device(case)
    figures = {}
    for variant in RR.VARIANTS:
        record(d)
        if variant == "record":      # the primal is trm_step's, whatever the record
            state, status, clock = stepped_twin(case)
            for name in STATE:
                assert np.array_equal(bits(d.get(name)), state[name]), (RR.record_id(rcase), name)
            assert d.status() == status and d.clock() == clock
        attach(d, rec)
        assert d.record_info()[:2] == (len(rec["positions"]), len(rec["levels"]))
        got = arm_and_sweep(d, RR.final_cotangent(case, variant), True, rec)
        prog = d.last_program()
        assert prog["family"] == "column_adjoint_richards" and prog["hydraulic_parameter_gradient"] is True, (RR.record_id(rcase), prog)
        assert prog["hydraulics"] == case[2] and prog["lanes_per_column"] == (32 if case[0] <= 32 else 64), (RR.record_id(rcase), prog)
        for part, key in zip(RR.PARTS, ("state", "params", "misfit")):
            figures[(part, variant)] = ref.error(part, variant, got[key])
    print(f"{RR.record_id(rcase)}: kept {int(ref.keep.sum())}/{ref.keep.size}")
    for (part, variant), err in figures.items():
        print(f"    {part} ({variant}): device = {err:.3e}, e_ref = {ref.parts[(part, variant)]:.3e}, bound = {bounds[part]:.3e}, ratio = {err / bounds[part]:.3f}")
    over = {key: err for key, err in figures.items() if not err <= bounds[key[0]]}
    assert not over, (RR.record_id(rcase), bounds, over)


# ---- 2. without a tolerance ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rcase", SOME, ids=RR.record_id)
def test_null_records_doubling_and_resummation_bit_for_bit(rcase):
    ref = RR.reference(rcase)
    case, rec = rcase[1], ref.record
    final, zero = RR.final_cotangent(case, "record+final"), RR.final_cotangent(case, "record")
    d = record_device(case)
    plain = record_sweep(d, None, final)
    # a record of NaNs, or of weights 0, gives the sweep without a record
    for null in (dict(rec, observed=np.full_like(rec["observed"], np.nan)), dict(rec, weight=np.zeros_like(rec["weight"]))):
        got = record_sweep(d, null, final)
        assert np.all(got["misfit"] == 0.0) and np.all(bits(got["residuals"]) == 0)            # (+0.0 for a gap)
        same({key: got[key] for key in plain}, plain, (RR.record_id(rcase), "a null record"))
    # one gap among the samples: its residual is +0.0, the others are the full record's
    full = record_sweep(d, rec, final)
    assert np.any(full["state"] != plain["state"]) and np.any(full["params"] != plain["params"]) and np.all(full["misfit"] > 0.0)
    holed = dict(rec, observed=rec["observed"].copy())
    holed["observed"][-1, 0, 0] = np.nan
    got = record_sweep(d, holed, final)
    assert bits(got["residuals"])[-1, 0, 0] == 0 and np.array_equal(bits(got["residuals"]).ravel()[:-rec["observed"][-1].size], bits(full["residuals"]).ravel()[:-rec["observed"][-1].size])
    assert got["misfit"][0] < full["misfit"][0] and np.array_equal(bits(got["misfit"][1:]), bits(full["misfit"][1:]))
    # doubled weights double the misfit and, with zero final cotangents, every gradient
    once, twice = record_sweep(d, rec, zero), record_sweep(d, dict(rec, weight=2.0 * rec["weight"]), zero)
    for key in ("state", "params", "misfit"):
        assert np.array_equal(bits(2.0 * once[key]), bits(twice[key])), (RR.record_id(rcase), key)
    assert np.array_equal(bits(once["residuals"]), bits(twice["residuals"])) and np.any(once["state"] != 0.0)
    # the host's resummation of the downloaded residuals is the misfit: positions ascending, levels in list order, one term at a time
    s = np.zeros(case[1])
    for r, w in zip(full["residuals"], rec["weight"]):
        for j in range(r.shape[0]):
            s = s + 0.5 * w[j] * r[j] * r[j]
    assert np.array_equal(bits(s), bits(full["misfit"]))
    # the residuals are sat_p - sat_obs of the taped saturations
    d.restore_state()
    first = d.get("saturation_water_ice")[rec["levels"]] - rec["observed"][0]
    assert rec["positions"][0] == 0 and np.array_equal(bits(first), bits(full["residuals"][0]))


@pytest.mark.parametrize("rcase", SOME, ids=RR.record_id)
def test_the_split_into_launches_and_calls_changes_no_bit(rcase):
    ref = RR.reference(rcase)
    case, rec = rcase[1], ref.record
    final = RR.final_cotangent(case, "record+final")
    whole = record_sweep(record_device(case), rec, final)
    same(record_sweep(record_device(case, steps_per_launch=6), rec, final), whole, "steps_per_launch 6")
    same(record_sweep(record_device(case), rec, final, ((DT, 3), (DT, 3))), whole, "two step_record calls of 3")
    same(record_sweep(record_device(case, steps_per_launch=1), rec, final), whole, "steps_per_launch 1")
    # gU and gsat with the parameter gradient open are those without it, and so are the residuals and the misfit
    without = record_sweep(record_device(case, params=False), rec, final, params=False)
    same(without, {key: whole[key] for key in without}, "without the parameter gradient")


def test_two_dts_agree_with_the_schedule_restatement():
    rcase = CASE33
    ref = RR.reference(rcase)
    case, rec = rcase[1], ref.record
    schedule = ((DT, 3), (DT / 2, 3))
    expected, Ssum, e_ref, keep = RR.schedule_reference(rcase, rec, schedule)
    bound = RR.FACTOR * max(e_ref, RA.Reference(case, schedule=list(schedule)).e_ref)
    assert 0.0 < bound <= RA.BROKEN
    got = record_sweep(record_device(case), rec, RR.final_cotangent(case, "record"), schedule)
    err = float(np.max(np.abs(got["state"][:, keep].astype(LD) - expected)[Ssum > 0] / Ssum[Ssum > 0]))
    print(f"two dts: device = {err:.3e}, e_ref = {e_ref:.3e}, bound = {bound:.3e}")
    assert keep.all() and err <= bound
    assert np.any(got["state"] != record_sweep(record_device(case), rec, RR.final_cotangent(case, "record"))["state"])


@pytest.mark.parametrize("rcase", SOME[:2], ids=RR.record_id)
def test_record_persists_over_sweeps_and_detaches(rcase):
    ref = RR.reference(rcase)
    case, rec = rcase[1], ref.record
    final = RR.final_cotangent(case, "record+final")
    d = record_device(case)
    plain = record_sweep(d, None, final)
    plain_program = d.last_program()
    d.restore_state()
    d.open_adjoint(STEPS)
    attach(d, rec)
    info = d.record_info()
    for fn in (d.record_misfit, d.record_residuals):                         # (no sweep has run with this record)
        with pytest.raises(CAPI.TerrariumHipError, match="no sweep has run with this record"):
            fn()
    rounds = []
    for _ in range(2):                                                       # two rounds of restore / record / sweep on one attachment
        d.restore_state()
        d.step_record(DT, STEPS)
        rounds.append(arm_and_sweep(d, final, True, rec))
        assert d.last_program() == plain_program                             # that of the record-free launch
    same(rounds[1], rounds[0], "the second round")
    assert d.record_info()[:2] == info[:2] and d.record_info()[2] > info[2]  # (the position table went up with the first sweep)
    assert np.any(rounds[0]["state"] != plain["state"])
    # a record longer than the tape is refused before anything is launched, and the tape stays usable
    d.restore_state()
    d.step_record(DT, STEPS - 1)
    assert call(d, "trm_adjoint_backward") == (CAPI.TRM_EINVAL, f"trm_adjoint_backward: the attached record is longer than the tape: position {STEPS} of {STEPS - 1} taped steps")
    d.step_record(DT, 1)
    same(arm_and_sweep(d, final, True, rec), rounds[0], "after the refusal")
    # detached: today's sweep
    d.detach_record()
    assert d.record_info() == (0, 0, 0)
    with pytest.raises(CAPI.TerrariumHipError, match="no record is attached"):
        d.record_misfit()
    d.restore_state()
    d.step_record(DT, STEPS)
    same(arm_and_sweep(d, final, True, None), plain, "after the detach")
    # the device-pointer attach against the host attach
    attach(d, rec, device_arrays=True)
    d.restore_state()
    d.step_record(DT, STEPS)
    same(arm_and_sweep(d, final, True, rec), rounds[0], "device arrays")
    assert d.record_info()[2] < info[2]                                      # (the arrays stay the caller's)
    d.close_adjoint()


# ---- 3. the adjoint identity on the device -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rcase", SOME, ids=RR.record_id)
def test_adjoint_identity_against_the_tangent_stopped_at_the_positions(rcase):
    ref = RR.reference(rcase)
    case, rec = rcase[1], ref.record
    Nz, keep, levels = case[0], ref.keep, rec["levels"]
    v = RC.inputs(case)[4]
    d = record_device(case)
    d.set_option("derivative_richards", 1)
    for variant in RR.VARIANTS:
        final = RR.final_cotangent(case, variant)
        got = record_sweep(d, rec, final)
        d.restore_state()
        d.open_tangent()
        d.set_tangent("internal_energy", v[:Nz])
        d.set_tangent("saturation", v[Nz:])
        lhs = np.zeros(case[1], dtype=LD)
        at = 0
        for k, s in enumerate(rec["positions"]):
            if s > at:
                d.step_tangent(DT, s - at)
                at = s
            dsat = d.tangent("saturation")
            lhs += np.einsum("ic,ic->c", (rec["weight"][k] * got["residuals"][k]).astype(LD), dsat[levels].astype(LD))
        t = np.stack([d.tangent(x) for x in TANGENTS])
        d.close_tangent()
        finite = np.isfinite(t) | (final != 0)                                # (a head at zero saturation: its cotangent is zero)
        lhs += np.einsum("xic,xic->c", final.astype(LD), np.where(finite, t, 0.0).astype(LD))
        rhs = np.einsum("jc,jc->c", got["state"].astype(LD), v.astype(LD))
        expected, Ssum = ref.identity[variant]
        assert np.all(Ssum > 0)
        err = float(np.max(np.abs(lhs[keep] - rhs[keep]) / Ssum))
        both = float(max(np.max(np.abs(lhs[keep] - expected) / Ssum), np.max(np.abs(rhs[keep] - expected) / Ssum)))
        bound = RR.bound(rcase, "state")
        print(f"{RR.record_id(rcase)} ({variant}): identity / S = {err:.3e}, against the reference {both:.3e}, bound {bound:.3e}")
        assert err <= bound and both <= bound, (RR.record_id(rcase), variant, err, both, bound)


# ---- 4. the gates ----------------------------------------------------------------------------------------------------------------------
def test_both_options_open_the_record_calls():
    """the test that fails without the feature: trm_adjoint_observe_record on a Richards context"""
    d = wet()
    assert d.get_option("derivative_richards_record") == 0
    d.set_option("derivative_richards_adjoint", 1)
    d.set_option("derivative_richards_record", 1)
    assert d.get_option("derivative_richards_record") == 1
    calls = dict(still_refused())
    # without an open adjoint the seven calls answer as on a heat-only context
    for name in RECORD_CALLS:
        rc, msg = call(d, name, *calls[name])
        assert rc == CAPI.TRM_EINVAL and "no adjoint is open (trm_adjoint_open)" in msg, (name, msg)
    d.open_adjoint(4)
    # the per-position calls, the checkpointed opener and trm_adjoint_bc_open stay refused (trm_adjoint_param_open: another option's)
    for name, args in still_refused():
        if name not in RECORD_CALLS:
            assert call(d, name, *args) == (CAPI.TRM_EUNSUPPORTED, f"{name}: {TAPE_ONLY}"), name
    assert d.record_info() == (0, 0, 0)
    d.attach_record([0, 2], [1, 3], np.full((2, 2, 3), 0.7), None)
    assert d.record_info()[:2] == (2, 2)
    rc, msg = call(d, "trm_adjoint_observe_record", *calls["trm_adjoint_observe_record"])
    assert rc == CAPI.TRM_EINVAL and "a record is attached already" in msg
    d.step_record(DT, 3)
    d.adjoint_backward()
    prog = d.last_program()
    assert prog["family"] == "column_adjoint_richards" and "hydraulic_parameter_gradient" not in prog
    assert d.record_residuals().shape == (2, 2, 3) and np.all(d.record_misfit() > 0.0) and np.any(d.cotangent("saturation") != 0.0)
    # the attach validation is the heat-only path's
    d.detach_record()
    for positions, levels, text in (([2, 2], [0], "the positions are taped-step counts >= 0, strictly increasing"), ([0], [4], "the levels are rows 0 ... 3"), ([0], [2, 1], "strictly increasing")):
        with pytest.raises(CAPI.TerrariumHipError, match=text):
            d.attach_record(positions, levels, np.zeros((len(positions), len(levels), 3)))
    with pytest.raises(CAPI.TerrariumHipError, match="a weight is negative or NaN"):
        d.attach_record([0], [0], np.zeros((1, 1, 3)), -1.0)


@pytest.mark.parametrize("adjoint_option, record_option", ((1, 0), (0, 1), (0, 0)))
def test_with_either_option_at_zero_every_answer_is_todays(adjoint_option, record_option):
    d = wet()
    d.set_option("derivative_richards_adjoint", adjoint_option)
    d.set_option("derivative_richards_record", record_option)
    calls = dict(still_refused())
    if not adjoint_option:
        assert call(d, "trm_adjoint_open", 4)[0] == CAPI.TRM_EUNSUPPORTED
        twin = wet()                                                         # (a context that has never heard of the option)
        for name in RECORD_CALLS:
            assert call(d, name, *calls[name]) == call(twin, name, *calls[name]), name
        return
    for opened in (False, True):
        if opened:
            d.open_adjoint(4)
        for name, args in still_refused():
            assert call(d, name, *args) == (CAPI.TRM_EUNSUPPORTED, f"{name}: {TAPE_ONLY}"), name


@pytest.mark.parametrize("option", (0, 1))
def test_a_noflow_context_behaves_as_before(option):
    h = small("noflow")
    h.set_option("derivative_richards_adjoint", option)
    h.set_option("derivative_richards_record", option)
    h.open_adjoint(3)
    h.attach_record([0, 2], [0, 3], np.full((2, 2, 3), 1.0), None)           # a temperature record, as ever
    h.step_record(DT, 2)
    h.adjoint_backward()
    assert h.last_program()["family"] == "column_adjoint" and np.all(np.isfinite(h.record_misfit()))
    misfit = h.record_misfit()
    twin = small("noflow")
    twin.open_adjoint(3)
    twin.attach_record([0, 2], [0, 3], np.full((2, 2, 3), 1.0), None)
    twin.step_record(DT, 2)
    twin.adjoint_backward()
    assert np.array_equal(bits(misfit), bits(twin.record_misfit())) and np.array_equal(bits(h.cotangent("internal_energy")), bits(twin.cotangent("internal_energy")))
    assert call(h, "trm_adjoint_bc_open")[0] == CAPI.TRM_OK


# ---- 5. the Python driver ----------------------------------------------------------------------------------------------------------------
def test_soil_moisture_gradient_is_the_c_abi_path():
    def build():
        grid = trm.ColumnGrid(trm.ExponentialSpacing(N=10), num_columns=3)
        soil = trm.SoilEnergyWaterCarbon(hydrology=trm.SoilHydrology(vertical_flow=trm.RichardsEq()))
        initializer = trm.SoilInitializer(hydrology=trm.ConstantSaturation(0.5))
        return trm.initialize(trm.SoilModel(grid, soil=soil, initializer=initializer), trm.ForwardEuler(dt=60.0))
    rng = np.random.default_rng(11)
    steps, levels = [0, 2, 5], [1, 4, 9]
    values = 0.5 + rng.uniform(-0.05, 0.05, (3, 3, 3))
    values[1, 2, 0] = np.nan
    weight = rng.uniform(0.5, 2.0, values.shape)
    rec = trm.SoilMoistureRecord(steps, levels, values, weight)
    w = {name: rng.normal(size=(10, 3)) * scale for name, scale in zip(BY_FIELD, (1e-6, 1.0, 1e-1, 1.0, 1e-2))}
    a = build()
    misfit, state, grads = trm.soil_moisture_gradient(a, rec, steps=6, cotangents=w, wrt_params=True)
    assert misfit.shape == (3,) and set(state) == {"internal_energy", "saturation"} and tuple(grads) == PARAMS
    for option in ("derivative_richards_adjoint", "derivative_richards_record", "derivative_richards_params"):
        assert a.state.get_option(option) == 0, option
    st = build().state
    for option in ("derivative_richards_adjoint", "derivative_richards_record", "derivative_richards_params"):
        st.set_option(option, 1)
    st.open_adjoint(6)
    st.attach_record(steps, levels, values, weight)
    st.step_record(60.0, 6)
    for name in BY_FIELD:
        st.set_cotangent(name, w[name])
    st.open_param_gradient()
    st.adjoint_backward()
    assert np.array_equal(bits(misfit), bits(st.record_misfit())) and np.all(misfit > 0.0)
    for name in state:
        assert np.array_equal(bits(state[name]), bits(st.cotangent(name))), name
    for name in PARAMS:
        assert grads[name].shape == (3,) and np.array_equal(bits(grads[name]), bits(st.param_gradient(name))), name
    assert st.record_residuals()[1, 2, 0] == 0.0 and np.any(grads["K_sat"] != 0.0)
    # the defaults: to the last observation, zero final cotangents, no parameters -- two items
    b = build()
    out = trm.soil_moisture_gradient(b, rec)
    assert len(out) == 2
    st = build().state
    st.set_option("derivative_richards_adjoint", 1)
    st.set_option("derivative_richards_record", 1)
    st.open_adjoint(5)
    st.attach_record(steps, levels, values, weight)
    st.step_record(60.0, 5)
    st.adjoint_backward()
    assert np.array_equal(bits(out[0]), bits(st.record_misfit())) and np.array_equal(bits(out[1]["saturation"]), bits(st.cotangent("saturation")))
    # vjp and hydraulic_parameter_gradient keep their behaviour: the record-free sweep
    plain = trm.vjp(build(), 6, internal_energy=w)
    none = trm.soil_moisture_gradient(build(), trm.SoilMoistureRecord(steps, levels, np.full_like(values, np.nan)), steps=6, cotangents=w)
    for name in plain:
        assert np.array_equal(bits(plain[name]), bits(none[1][name])), name
    assert np.all(none[0] == 0.0)
    # the ValueErrors
    with pytest.raises(ValueError, match="strictly increasing"):
        trm.soil_moisture_gradient(build(), trm.SoilMoistureRecord([0, 2, 2], levels, values))
    with pytest.raises(ValueError, match="observations behind the last step"):
        trm.soil_moisture_gradient(build(), rec, steps=4)
    with pytest.raises(KeyError, match="hydraulic_conductivity"):
        trm.soil_moisture_gradient(build(), rec, cotangents={"hydraulic_conductivity": 1.0})
    grid = trm.ColumnGrid(trm.ExponentialSpacing(N=10), num_columns=3)
    heat = trm.initialize(trm.SoilModel(grid, initializer=trm.SoilInitializer()), trm.ForwardEuler(dt=60.0))
    with pytest.raises(ValueError, match="needs an integrator with RichardsEq"):
        trm.soil_moisture_gradient(heat, rec)
