"""Tangent records on the device (trm_tangent_record_attach): positions and levels attached to the open tangent once, the temperature and
its tangent stored inside the tangent launches, value by value against the exact Jacobian of tests/linearised_heat.py.

The cases and the reference are tangent_record.py's: the records of adjoint_record.py (positions 0, 3, 5, 6 of a run of 6 steps in
launches of 4 and 2, so that 3 and 5 fall inside launches; a dense record; the two ends alone) with the seeds of the case on the state,
the boundary values, the thermal parameters and the nodes of a series.  Per case every T and dT sample lies within 8 x e_ref of its
contraction.  Beside it what needs no tolerance -- with one step per launch every sample is the bits of trm_step_tangent(dt, 1) repeated
and a download, the state and the three tangents are those of the run without a record, doubled seeds, NaN at unreached positions, a
rewind, the counter across calls and a change of dt -- the refusals on a live context, the adjoint identity against the attached
adjoint record for every family of seeds, and the Python interface with the Gauss-Newton example."""
import numpy as np
import pytest

import tangent_record as TR
import terrarium_jl_amd as trm
from boundary_derivatives import LD, PAIRS
from parameter_derivatives import PARAMS
from test_gpu_adjoint_observations import code_of, obs_device
from test_gpu_adjoint_record import SOME, sweep
from test_gpu_derivative_edges import DT, SERIES_PAIR, STEPS, device, report
from test_gpu_tangent import STATE, TANGENTS, bits

pytestmark = pytest.mark.gpu
EINVAL = trm._capi.TRM_EINVAL


def one_step_device(case):
    d = device(case, steps_per_launch=1)
    if case[5]:
        d.set_option("derivative_series_params", 1)
    return d


def seed(d, case, key, v, scale=1.0):
    """the saved state under a fresh tangent (which zeroes every seed and drops a record) with the seeds `v` of the family `key`"""
    d.restore_state()
    d.open_tangent()
    d.set_tangent("internal_energy", v * scale if key == "state" else 0.0)
    if key == "boundary":
        for pair, values in zip(PAIRS, v):
            d.set_bc_tangent(*pair, values * scale)
    if key == "params":
        d.set_param_tangent(dict(zip(PARAMS, v * scale)))
    if key == "series":
        d.set_bc_series_tangent(*SERIES_PAIR[case[2]], v * scale)


def samples(d):
    return d.tangent_record("temperature"), d.tangent_record("tangent")


def recorded(d, case, rcase, key, v, scale=1.0, pieces=((DT, STEPS),)):
    """(T, dT) of the saved state run in `pieces` with the record of the case attached"""
    seed(d, case, key, v, scale)
    d.attach_tangent_record(TR.positions_of(rcase), TR.levels_of(rcase))
    for dt, n in pieces:
        d.step_tangent(dt, n)
    prog = d.last_program()
    assert prog["family"] == "column_tangent" and prog["lanes_per_column"] == (32 if case[0] <= 32 else 64), (TR.record_id(rcase), prog)
    assert prog["parameter_seeds"] == (key == "params")
    return samples(d)


def left_behind(d):
    return {name: bits(d.get(name)) for name in STATE}, {x: bits(d.tangent(x)) for x in TANGENTS}, d.status(), d.clock(), d.last_program()


# ---- 1. the exact Jacobian -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rcase", TR.CASES, ids=TR.record_id)
def test_samples_match_the_exact_jacobian(rcase):
    ref = TR.reference(rcase)
    case, vectors = rcase[1], ref.inputs[5]
    d = obs_device(case)
    figures = {}
    for key in TR.seed_keys(case):
        T, dT = recorded(d, case, rcase, key, vectors[key])
        assert not np.any(np.isnan(T)) and not np.any(np.isnan(dT)), (TR.record_id(rcase), key)
        assert d.tangent_record_info()[:3] == (len(TR.positions_of(rcase)), len(TR.levels_of(rcase)), STEPS)
        figures[f"dT {key}"] = ref.error(f"dT {key}", dT)
        figures[f"temperature [{key}]"] = ref.error("temperature", T)
        d.close_tangent()
    report(ref, figures)


# ---- 2. what needs no tolerance --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rcase", SOME, ids=TR.record_id)
def test_one_step_launches_give_the_bits_of_step_tangent_and_a_download(rcase):
    ref = TR.reference(rcase)
    case, vectors = rcase[1], ref.inputs[5]
    positions, levels = TR.positions_of(rcase), TR.levels_of(rcase)
    d1, d4 = one_step_device(case), obs_device(case)
    for key in TR.seed_keys(case):
        T, dT = recorded(d1, case, rcase, key, vectors[key])
        # by hand: trm_step_tangent(dt, 1) repeated p times, then the downloads
        seed(d1, case, key, vectors[key])
        d1.tangent_closure()
        at = 0
        for k, p in enumerate(positions):
            for _ in range(p - at):
                d1.step_tangent(DT, 1)
            at = p
            assert np.array_equal(bits(T[k]), bits(d1.get("temperature")[levels])), (TR.record_id(rcase), key, "T at position", p)
            assert np.array_equal(bits(dT[k]), bits(d1.tangent("temperature")[levels])), (TR.record_id(rcase), key, "dT at position", p)
        d1.close_tangent()
        # launches of 4 and 2: a figure, no assertion
        T4, dT4 = recorded(d4, case, rcase, key, vectors[key])
        d4.close_tangent()
        print(f"ONE-VS-FOUR-STEP-LAUNCHES {TR.record_id(rcase)} [{key}]: T bit-identical = {np.array_equal(bits(T4), bits(T))}, "
              f"dT bit-identical = {np.array_equal(bits(dT4), bits(dT))}")


@pytest.mark.parametrize("rcase", SOME, ids=TR.record_id)
def test_state_and_tangents_are_those_of_the_run_without_a_record(rcase):
    ref = TR.reference(rcase)
    case, vectors = rcase[1], ref.inputs[5]
    d = obs_device(case)
    for key in TR.seed_keys(case):
        seed(d, case, key, vectors[key])
        d.step_tangent(DT, STEPS)
        plain = left_behind(d)
        T, dT = recorded(d, case, rcase, key, vectors[key])
        with_record = left_behind(d)
        for mine, theirs in zip(with_record[:2], plain[:2]):
            for name in theirs:
                assert np.array_equal(mine[name], theirs[name]), (TR.record_id(rcase), key, name)
        assert with_record[2:] == plain[2:], (TR.record_id(rcase), key, with_record[2:], plain[2:])
        # the last position is the end of the run: its samples are the stored fields
        assert np.array_equal(bits(T[-1]), with_record[0]["temperature"][TR.levels_of(rcase)])
        assert np.array_equal(bits(dT[-1]), with_record[1]["temperature"][TR.levels_of(rcase)])
        # seeds doubled: the samples of dT doubled, those of T unchanged, bit for bit
        T2, dT2 = recorded(d, case, rcase, key, vectors[key], scale=2.0)
        assert np.array_equal(bits(dT2), bits(2.0 * dT)) and np.array_equal(bits(T2), bits(T)), (TR.record_id(rcase), key)
        assert key != "state" or np.any(dT != 0.0)       # (boundary seeds may not reach the levels of a deep column in six steps)
        d.close_tangent()


@pytest.mark.parametrize("rcase", SOME, ids=TR.record_id)
def test_unreached_positions_rewind_and_the_counter(rcase):
    ref = TR.reference(rcase)
    case, dU = rcase[1], ref.inputs[5]["state"]
    positions, levels = TR.positions_of(rcase), TR.levels_of(rcase)
    d = obs_device(case)
    T, dT = recorded(d, case, rcase, "state", dU)
    # two calls: the counter runs on, positions behind it read NaN until a step reaches them
    part_T, part_dT = recorded(d, case, rcase, "state", dU, pieces=((DT, 4),))
    reached = np.array([p <= 4 for p in positions])
    assert d.tangent_record_info()[2] == 4
    for a, whole in ((part_T, T), (part_dT, dT)):
        assert np.all(np.isnan(a[~reached])) and np.array_equal(bits(a[reached]), bits(whole[reached])), TR.record_id(rcase)
    d.step_tangent(DT, 2)
    assert d.tangent_record_info()[2] == STEPS
    # (the launches were 4 and 2 either way)
    assert np.array_equal(bits(d.tangent_record("temperature")), bits(T)) and np.array_equal(bits(d.tangent_record("tangent")), bits(dT))
    # steps behind the last position sample nothing, and the counter counts them
    state = left_behind(d)
    d.step_tangent(DT, 3)
    assert d.tangent_record_info()[2] == STEPS + 3 and d.last_program() == state[4]
    assert np.array_equal(bits(d.tangent_record("temperature")), bits(T)) and np.array_equal(bits(d.tangent_record("tangent")), bits(dT))
    # a rewind and a second run on the same attachment: NaN, then the bits of the first run
    d.rewind_tangent_record()
    assert d.tangent_record_info()[:3] == (len(positions), len(levels), 0)
    assert np.all(np.isnan(d.tangent_record("temperature"))) and np.all(np.isnan(d.tangent_record("tangent")))
    d.restore_state()
    d.set_tangent("internal_energy", dU)
    d.step_tangent(DT, STEPS)
    assert np.array_equal(bits(d.tangent_record("temperature")), bits(T)) and np.array_equal(bits(d.tangent_record("tangent")), bits(dT))
    d.close_tangent()
    # a change of dt inside the run: positions on both sides of the change and at it, against the same calls without a record
    if not case[5] and 3 in positions:
        pieces = ((DT, 3), (2.0 * DT, 3))
        T_two, dT_two = recorded(d, case, rcase, "state", dU, pieces=pieces)
        assert d.tangent_record_info()[2] == STEPS and not np.any(np.isnan(T_two)) and np.any(T_two[-1] != T[-1])
        seed(d, case, "state", dU)
        for (dt, n), p in zip(pieces, (3, STEPS)):
            d.step_tangent(dt, n)
            k = positions.index(p)
            assert np.array_equal(bits(T_two[k]), bits(d.get("temperature")[levels])) and np.array_equal(bits(dT_two[k]), bits(d.tangent("temperature")[levels]))
        d.close_tangent()


# ---- 3. detach and refusals on a live context ---------------------------------------------------------------------------------------------
def test_detach_and_refusals_on_a_live_context():
    rcase = next(rc for rc in SOME if rc[0] == "AO" and rc[1][0] == 33 and rc[1][5] is None)
    case = rcase[1]
    positions, levels = list(TR.positions_of(rcase)), TR.levels_of(rcase)
    dU = TR.reference(rcase).inputs[5]["state"]
    d = obs_device(case)
    L = trm._capi.lib()
    # without an open tangent: the words of the other tangent calls
    for call in (lambda: d.attach_tangent_record(positions, levels), d.rewind_tangent_record, d.detach_tangent_record, d.tangent_record_info,
                 lambda: d.tangent_record("temperature")):
        code, msg = code_of(call)
        assert code == EINVAL and "no tangent is open (trm_tangent_open)" in msg, msg
    d.restore_state()
    d.open_tangent()
    assert d.tangent_record_info() == (0, 0, 0, 0)
    for call in (d.rewind_tangent_record, d.detach_tangent_record):
        code, msg = code_of(call)
        assert code == EINVAL and "no record is attached (trm_tangent_record_attach)" in msg, msg
    # bad lists attach nothing
    for bad, why in ((lambda: d.attach_tangent_record([], levels), "bad argument"), (lambda: d.attach_tangent_record(positions, []), "bad argument"),
                     (lambda: d.attach_tangent_record([-1, 2], levels), "strictly increasing"), (lambda: d.attach_tangent_record([0, 3, 3], levels), "strictly increasing"),
                     (lambda: d.attach_tangent_record([3, 0], levels), "the positions are tangent-step counts >= 0, strictly increasing"),
                     (lambda: d.attach_tangent_record([0], [case[0]]), f"the levels are rows 0 ... {case[0] - 1} of the host layout"),
                     (lambda: d.attach_tangent_record([0], [-1]), "the levels are rows"), (lambda: d.attach_tangent_record([0], [1, 0]), "strictly increasing")):
        code, msg = code_of(bad)
        assert code == EINVAL and why in msg, msg
    idx = np.zeros(1, dtype=np.int32)
    assert L.trm_tangent_record_attach(d._ctx, 1, None, 1, idx.ctypes.data) == EINVAL and L.trm_tangent_record_attach(d._ctx, 1, idx.ctypes.data, 1, None) == EINVAL
    assert d.tangent_record_info() == (0, 0, 0, 0)
    # attached: the shape, the bytes, one record at a time, `which` and NULL pointers
    d.attach_tangent_record(positions, levels)
    cells = len(positions) * len(levels) * case[1]
    assert d.tangent_record_info() == (len(positions), len(levels), 0, 2 * cells * 8 + (case[0] + positions[-1] + 1) * 4)
    assert np.all(np.isnan(d.tangent_record("temperature"))) and np.all(np.isnan(d.tangent_record("tangent")))
    code, msg = code_of(lambda: d.attach_tangent_record(positions, levels))
    assert code == EINVAL and "a record is attached already (trm_tangent_record_detach)" in msg, msg
    import ctypes
    a, dev = np.zeros(cells), ctypes.c_void_p()
    for which in (-1, 2):
        assert L.trm_tangent_record_download(d._ctx, which, a.ctypes.data) == EINVAL
        assert L.trm_tangent_record_device_ptr(d._ctx, which, ctypes.byref(dev)) == EINVAL
    assert L.trm_tangent_record_download(d._ctx, 0, None) == EINVAL and L.trm_tangent_record_device_ptr(d._ctx, 0, None) == EINVAL
    with pytest.raises(KeyError):
        d.tangent_record("liquid_water_fraction")
    # two device arrays of their own
    ptrs = []
    for which in (0, 1):
        assert L.trm_tangent_record_device_ptr(d._ctx, which, ctypes.byref(dev)) == 0 and dev.value
        ptrs.append(dev.value)
    assert abs(ptrs[0] - ptrs[1]) >= cells * 8
    d.set_tangent("internal_energy", dU)
    d.step_tangent(DT, STEPS)
    T, dT = samples(d)
    assert not np.any(np.isnan(T)) and np.any(dT != 0.0)
    # detached: the run without a record, and nothing to read
    d.detach_tangent_record()
    assert d.tangent_record_info() == (0, 0, 0, 0)
    assert code_of(lambda: d.tangent_record("tangent"))[0] == EINVAL and code_of(d.detach_tangent_record)[0] == EINVAL
    # trm_tangent_open and trm_tangent_close drop the record as well
    d.attach_tangent_record(positions, levels)
    d.open_tangent()
    assert d.tangent_record_info() == (0, 0, 0, 0)
    d.attach_tangent_record(positions, levels)
    d.close_tangent()
    d.open_tangent()
    assert d.tangent_record_info() == (0, 0, 0, 0)
    d.close_tangent()
    # the model kinds the tangent refuses keep refusing in their words, and have no tangent to attach to
    from test_gpu_derivative_refusals import context
    for kind, why in (("f32", "fp64 contexts only"), ("richards", "the heat-only SoilModel (NoFlow) only")):
        other = context(kind)
        code, msg = code_of(other.open_tangent)
        assert code == trm._capi.TRM_EUNSUPPORTED and why in msg, msg
        code, msg = code_of(lambda: other.attach_tangent_record([0], [0]))
        assert code == trm._capi.TRM_EUNSUPPORTED and "trm_tangent_record_attach" in msg and why in msg, msg
        other.close()


# ---- 4. the adjoint identity against the attached adjoint record ---------------------------------------------------------------------------
@pytest.mark.parametrize("rcase", [rc for rc in TR.CASES if rc[0] != "AO" or rc[1][4] == 26.0], ids=TR.record_id)
def test_adjoint_identity_against_the_attached_adjoint_record(rcase):
    """per column sum_k sum_i w r (J_k v)_i from the tangent record against <gradient of the misfit, v> from one sweep with the record
    attached to the adjoint (zero final cotangents), for every family of seeds; both within the bound of the reference's contraction"""
    ref = TR.reference(rcase)
    case, rec, vectors = rcase[1], ref.record, ref.inputs[5]
    d = obs_device(case)
    zero = np.zeros_like(vectors["cotangents"])
    grads, _, _ = sweep(d, case, rec, zero, None, ride="params")
    figures = {}
    for key in TR.seed_keys(case):
        v = vectors[key]
        T, dT = recorded(d, case, rcase, key, v)
        d.close_tangent()
        lhs = np.einsum("kic,kic->c", (rec["weight"] * (T - rec["observed"])).astype(LD), dT.astype(LD))
        g = grads[key].astype(LD)
        rhs = np.einsum("qc,q->c", g, v.astype(LD)) if v.ndim == 1 else np.einsum("jc,jc->c", g, v.astype(LD))
        figures[f"identity {key} [tangent record]"] = ref.error(f"identity {key}", lhs)
        figures[f"identity {key} [adjoint record]"] = ref.error(f"identity {key}", rhs)
        Ssum = ref.expected[f"identity {key}"][1]
        print(f"    {key}: lhs - rhs = {float(np.max(np.abs(lhs - rhs)[ref.keep][Ssum > 0] / Ssum[Ssum > 0], initial=0.0)):.3e} S")
    report(ref, figures)


# ---- 5. the Python interface ---------------------------------------------------------------------------------------------------------------
def column(Nz=33, Nh=13):
    grid = trm.ColumnGrid(trm.ExponentialSpacing(N=Nz), num_columns=Nh)
    model = trm.SoilModel(grid, initializer=trm.SoilInitializer())
    bcs = trm.merge_boundary_conditions(trm.PrescribedSurfaceTemperature("T_ub", 1.0))
    return trm.initialize(model, trm.ForwardEuler(), boundary_conditions=bcs)


def test_record_jvp_of_an_integrator_is_the_calls_by_hand():
    Nz, Nh = 33, 13
    dt = trm.ForwardEuler().dt
    positions, levels = [0, 3, 5, 6], [0, 31, 32]
    rng = np.random.default_rng(6)
    dU = rng.normal(0.0, 1e3, (Nz, Nh))
    seeds = dict(k_mineral=1.0, c_water=-2.0e5)
    integ = column()
    T, dT = trm.record_jvp(integ, positions, levels, d_internal_energy=dU, d_boundary={("temperature", "top"): 0.5}, d_params=seeds)
    assert T.shape == dT.shape == (4, 3, Nh) and np.all(np.isfinite(T)) and np.all(np.isfinite(dT)) and np.any(dT[0] != 0.0)
    assert trm.iteration(integ) == 6 and not getattr(integ.state, "_tangent_open", False)
    st = column().state
    st.open_tangent()
    st.set_tangent("internal_energy", dU)
    st.set_bc_tangent("temperature", "top", 0.5)
    st.set_param_tangent(seeds)
    st.attach_tangent_record(positions, levels)
    st.step_tangent(dt, 6)
    assert np.array_equal(bits(st.tangent_record("temperature")), bits(T)) and np.array_equal(bits(st.tangent_record("tangent")), bits(dT))
    # ... and the final samples are jvp's tangent
    final = trm.jvp(column(), dU, 6, d_boundary={("temperature", "top"): 0.5}, d_params=seeds)
    assert np.array_equal(bits(final["temperature"][levels]), bits(dT[-1]))
    st.close_tangent()
    # zero seeds: the record the model itself produces, steps behind the last position allowed, an open tangent stays open
    integ = column()
    integ.state.open_tangent()
    T0, dT0 = trm.record_jvp(integ, positions, levels, steps=8)
    assert np.array_equal(bits(T0), bits(T)) and not dT0.any() and trm.iteration(integ) == 8
    assert integ.state._tangent_open and integ.state.tangent_record_info()[:2] == (0, 0)
    integ.state.close_tangent()


@pytest.mark.parametrize("rcase", [rc for rc in SOME if rc[1][5] is None and rc[0] != "ends" and rc[1][2] == "flux_top+T_bottom"], ids=TR.record_id)
def test_normal_equations_b_is_the_gradient_of_record_gradient(rcase):
    """b of trm.record_normal_equations (ten tangent runs) against the parameter gradients of trm.record_gradient (one sweep), both
    contracted with the parameter seeds of the case: within the bound of the reference's "identity params" """
    ref = TR.reference(rcase)
    case, rec, v = rcase[1], ref.record, ref.inputs[5]["params"]
    d = obs_device(case)
    d.restore_state()
    integ = trm.ModelIntegrator(None, trm.ForwardEuler(dt=DT), d, {}, {}, {})
    record = trm.TemperatureRecord(rec["positions"], rec["levels"], rec["observed"], rec["weight"])
    before, clock = {name: bits(d.get(name)) for name in trm.restart_fields(integ)}, d.clock()
    misfit, b, A = trm.record_normal_equations(integ, record, PARAMS)
    # (left where it was: the restart set and the clock, what trm.restore brings back)
    assert all(np.array_equal(bits(d.get(name)), before[name]) for name in before) and d.clock() == clock
    assert b.shape == (10, case[1]) and A.shape == (10, 10, case[1]) and np.all(misfit > 0)
    L, _, pg = trm.record_gradient(integ, record, wrt_params=True)
    g = np.stack([pg[name] for name in PARAMS])
    figures = {"identity params [normal equations]": ref.error("identity params", np.einsum("qc,q->c", b.astype(LD), v.astype(LD))),
               "identity params [record_gradient]": ref.error("identity params", np.einsum("qc,q->c", g.astype(LD), v.astype(LD)))}
    print(f"    misfit: normal equations against record_gradient, largest relative difference {float(np.max(np.abs(misfit - L) / L)):.3e}")
    report(ref, figures)


def test_the_gauss_newton_example_calibrates():
    import importlib.util
    import os

    def load(name):
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", name + ".py")
        spec = importlib.util.spec_from_file_location(name, path)
        module = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(module)
        return module

    ex, dense = load("borehole_calibration_gauss_newton"), load("borehole_calibration_dense")
    # its synthetic record is the 240-call record of the sibling example, bit for bit
    record, U0 = ex.synthetic_record()
    positions, levels, values, U0_dense = dense.synthetic_record()
    assert record.steps == positions and list(record.levels) == list(levels)
    assert np.array_equal(bits(record.values), bits(values)) and np.array_equal(bits(U0), bits(U0_dense))
    history = ex.main(iterations=6)
    misfits = [L for L, _, _ in history]
    accepted = [k for k, (_, _, ok) in enumerate(history) if ok and k > 0]
    assert len(accepted) >= 1, history
    assert all(misfits[k] < misfits[k - 1] for k in accepted) and all(misfits[k] == misfits[k - 1] for k in range(1, len(history)) if k not in accepted)
    assert misfits[-1] < misfits[0]
    # beside gradient descent on the same problem: figures, no assertion

    def error(params):
        return max(abs(float(np.log(params[name] / ex.TRUTH[name]))) for name in ex.NAMES)

    descent = dense.main(12)
    print(f"GAUSS-NEWTON-VS-DESCENT: Levenberg-Marquardt, {len(history) - 1} iterates of 2 tangent runs: misfit {misfits[-1]:.6e}, "
          f"largest |log(p / truth)| {error(history[-1][1]):.3e}; descent, 12 iterates of 1 sweep: misfit {descent[-1][0]:.6e}, "
          f"largest |log(p / truth)| {error(descent[-1][1]):.3e}; initial misfit {misfits[0]:.6e}")
