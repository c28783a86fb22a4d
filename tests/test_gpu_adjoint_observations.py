"""Adjoint observations on the device: gradients of a loss that reads the run at taped positions (trm_adjoint_observe,
trm_adjoint_observe_misfit), value by value against the exact Jacobian of tests/linearised_heat.py.

The cases, the record and the reference are adjoint_observations.py's: Nz in 2, 3, 32, 33, 64 x 13 columns and 64 x 1, observed on the
levels 0 and Nz - 1 plus 31 and 32, at the positions 0, 3, 5 and 6 of a run of 6 steps in launches of up to 4 -- before any step, inside
what would be one launch, one step before the end, and at the end together with final cotangents.  On the checkpointed tape (K = 4)
position 3 falls inside a segment and 5 closes one early.  Per case, for the linear and the misfit kind and on both tapes, dL/dU_0,
the boundary gradients, the node gradients of a series and the ten parameter gradients lie within 8 x e_ref of the case and of the
contraction itself (e_ref computed on the CPU, a bound above 1e-12 refused, exact 0.0 where every reference product is zero), and so
does the misfit per column.  Beside it what needs no tolerance: zero cotangents change no bit, a factor 2 scales every bit, a NaN
sample is a weight 0, the checkpointed tape gives the per-step tape's dL/dU_0; the adjoint identity against trm_step_tangent called
in the same pieces; the primal of the interleaved record calls is trm_step's; the bookkeeping of the observation list and of the slot
a mid-segment observation takes; trm.misfit_gradient against the calls by hand, and examples/borehole_calibration.py."""
import importlib.util
import os

import numpy as np
import pytest

import adjoint_observations as AO
import terrarium_jl_amd as trm
from boundary_derivatives import LD, PAIRS
from parameter_derivatives import PARAMS
from test_gpu_derivative_edges import DT, FACTOR, SERIES_PAIR, STEPS, assert_primal, case_id, device, report, stepped_twin
from test_gpu_tangent import STATE, TANGENTS, bits

pytestmark = pytest.mark.gpu
K, POSITIONS = AO.K, AO.POSITIONS
EINVAL, ESTALE = trm._capi.TRM_EINVAL, trm._capi.TRM_ESTALE
# a representative of every lane layout for the tests that need no reference: both halves of the 32- and 64-lane layouts, a series
SOME = [c for c in AO.CASES if (c[0], c[1]) in ((3, 13), (33, 13), (64, 1)) and c[4] == 26.0 and c[2] in (AO.SERIES_SET, "flux_top+T_bottom")]


def obs_device(case):
    d = device(case)
    if case[5]:
        d.set_option("derivative_series_params", 1)
    return d


def slots(checkpoint_every):
    return STEPS if checkpoint_every is None else 3           # K = 4: the stretches 0-3, 3-5, 5-6


def register(d, kind, rec, k, scale=1.0, zero=False):
    levels = rec["levels"]
    f = 0.0 if zero else scale
    if kind == "linear":
        w = rec["linear"][k] * f
        d.observe(levels, internal_energy=w[0], temperature=w[1], liquid_water_fraction=w[2])
    else:
        d.observe_misfit(levels, rec["observed"][k], rec["weight"][k] * f)


def sweep(d, case, kind, rec, final, checkpoint_every=None, ride="params", scale=1.0, zero=False, observe=True, dts=None, on_recorded=None):
    """{input: gradient} and the misfit per column of the saved state: records the run on a fresh tape in the pieces between the
    observed positions, registers the record's observations of `kind` on the way, pulls everything back in one sweep.  ride: "state"
    (dL/dU_0 alone), "boundary", "params" (with the boundary values; with a series: the nodes, the other pairs, the parameters)"""
    d.restore_state()
    d.open_adjoint(slots(checkpoint_every) if dts is None else STEPS, checkpoint_every)
    if ride == "boundary":
        d.open_bc_gradient()
    if ride == "params":
        d.open_param_gradient()
    at = 0
    for k, s in enumerate(POSITIONS):
        if s > at:
            d.step_record(DT if dts is None else dts[k], s - at)
            at = s
        if observe:
            register(d, kind, rec, k, scale, zero)
    if on_recorded:
        on_recorded(d)
    for x, wx in zip(TANGENTS, final):
        d.set_cotangent(x, wx * scale)
    loss = d.misfit()
    d.adjoint_backward()
    prog = d.last_program()
    assert prog["family"] == "column_adjoint" and prog["backward"] and prog["checkpointed"] == (checkpoint_every is not None), (case_id(case), prog)
    assert prog["parameter_gradient"] == (ride == "params") and prog["lanes_per_column"] == (32 if case[0] <= 32 else 64), (case_id(case), prog)
    assert d.adjoint_observations() == (0, 0) and not d.misfit().any()          # a sweep that succeeded drops them
    out = {"state": d.cotangent("internal_energy")}
    if ride in ("boundary", "params"):
        boundary = np.zeros((len(PAIRS), case[1]))                              # (a seriesed pair has no per-column gradient: its row stays 0)
        for pair in PAIRS:
            if not (case[5] and pair == SERIES_PAIR[case[2]]):
                boundary[PAIRS.index(pair)] = d.bc_gradient(*pair)
        out["boundary"] = boundary
    if ride == "params":
        out["params"] = np.stack([d.param_gradient(name) for name in PARAMS])
    if case[5]:
        out["series"] = d.bc_series_gradient(*SERIES_PAIR[case[2]])
    d.close_adjoint()
    return out, loss


def report_each(ref, figures):
    """report of test_gpu_derivative_edges.py (every figure within the bound of the case), and every figure within FACTOR x e_ref of
    its own contraction as well: the parts of a case differ by two orders (the misfit carries the rounding of T - T_obs)"""
    report(ref, figures)
    over = {label: (err, ref.parts[label.split(" [")[0]]) for label, err in figures.items() if not err <= FACTOR * ref.parts[label.split(" [")[0]]}
    assert not over, (case_id(ref.case), "beyond FACTOR x e_ref of the contraction itself", over)


def same_bits(a, b, what):
    for key in a:
        assert np.array_equal(bits(a[key]), bits(b[key])), (what, key)


# ---- 1. the exact Jacobian -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", AO.CASES, ids=case_id)
def test_gradients_and_loss_match_the_exact_jacobian(case):
    ref = AO.reference(case)
    rec, final = ref.record, ref.inputs[5]["cotangents"]
    d = obs_device(case)
    rides = ("params",) if case[5] else ("state", "boundary", "params")
    figures = {}
    for kind in AO.KINDS:
        for ride in rides:
            per_step, loss = sweep(d, case, kind, rec, final, ride=ride)
            checkpointed, loss_ckpt = sweep(d, case, kind, rec, final, checkpoint_every=K, ride=ride)
            # 2d. the checkpointed tape gives the per-step tape's dL/dU_0, and the misfit does not depend on the tape
            assert np.array_equal(bits(checkpointed["state"]), bits(per_step["state"])), (case_id(case), kind, ride, "checkpointed against per-step")
            assert np.array_equal(bits(loss_ckpt), bits(loss))
            for tape, grads in (("per-step", per_step), ("checkpointed", checkpointed)):
                for key, g in grads.items():
                    figures[f"{kind} gradient {key} [{ride}, {tape}]"] = ref.error(f"{kind} gradient {key}", g)
            if kind == "misfit":
                figures[f"misfit loss [{ride}]"] = ref.error("misfit loss", loss)
            else:
                assert not loss.any()
        if case[4] == 26.0:
            assert np.any(per_step["params"][PARAMS.index("k_organic")] != 0.0) and np.any(per_step["params"][PARAMS.index("c_organic")] != 0.0)
    report_each(ref, figures)


# ---- 2. equivalences that need no tolerance -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SOME, ids=case_id)
@pytest.mark.parametrize("checkpoint_every", (None, K), ids=("per-step", "checkpointed"))
def test_equivalences_bit_for_bit(case, checkpoint_every):
    ref = AO.reference(case)
    rec, final = ref.record, ref.inputs[5]["cotangents"]
    d = obs_device(case)
    for kind in AO.KINDS:
        what = (case_id(case), kind)
        # observations whose cotangents are all zero: the bits of the sweep without them
        plain, _ = sweep(d, case, kind, rec, final, checkpoint_every, observe=False)
        zeroed, loss = sweep(d, case, kind, rec, final, checkpoint_every, zero=True)
        same_bits(zeroed, plain, what + ("zero cotangents",))
        assert not loss.any()
        # every cotangent and weight times 2: every gradient, and the misfit, times 2
        once, loss1 = sweep(d, case, kind, rec, final, checkpoint_every)
        twice, loss2 = sweep(d, case, kind, rec, final, checkpoint_every, scale=2.0)
        same_bits(twice, {key: 2.0 * g for key, g in once.items()}, what + ("scaled by 2",))
        assert np.array_equal(bits(loss2), bits(2.0 * loss1))
        assert any(np.any(once[key] != plain[key]) for key in once), what + ("the observations change the gradient",)
    # a NaN sample: the gradient and the misfit of the same record with that sample's weight 0; no weights: the weights 1
    Nh = case[1]
    gap = {key: [a.copy() for a in v] if key != "levels" else v for key, v in rec.items()}
    holed = {key: [a.copy() for a in v] if key != "levels" else v for key, v in rec.items()}
    for k, (j, c) in enumerate([(0, 0), (-1, Nh - 1), (0, Nh // 2), (-1, 0)]):
        gap["observed"][k][j, c] = np.nan
        holed["weight"][k][j, c] = 0.0
    with_gap, loss_gap = sweep(d, case, "misfit", gap, final, checkpoint_every)
    with_zero, loss_zero = sweep(d, case, "misfit", holed, final, checkpoint_every)
    same_bits(with_gap, with_zero, (case_id(case), "a NaN sample against its weight 0"))
    assert np.array_equal(bits(loss_gap), bits(loss_zero)) and np.all(np.isfinite(loss_gap))
    full, loss_full = sweep(d, case, "misfit", rec, final, checkpoint_every)
    assert np.any(loss_gap != loss_full)          # (the gradient may not move: a sample in phase change has the slope 0)
    ones = dict(rec, weight=[np.ones_like(w) for w in rec["weight"]])
    explicit, loss_explicit = sweep(d, case, "misfit", ones, final, checkpoint_every)
    d.restore_state()
    d.open_adjoint(slots(checkpoint_every), checkpoint_every)
    d.open_param_gradient()
    at = 0
    for k, s in enumerate(POSITIONS):
        if s > at:
            d.step_record(DT, s - at)
            at = s
        d.observe_misfit(rec["levels"], rec["observed"][k])
    for x, wx in zip(TANGENTS, final):
        d.set_cotangent(x, wx)
    assert np.array_equal(bits(d.misfit()), bits(loss_explicit))
    d.adjoint_backward()
    assert np.array_equal(bits(d.cotangent("internal_energy")), bits(explicit["state"]))
    d.close_adjoint()


@pytest.mark.parametrize("case", [c for c in SOME if c[5] is None], ids=case_id)
def test_checkpointed_tape_with_a_change_of_dt_gives_the_per_step_bits(case):
    ref = AO.reference(case)
    rec, final = ref.record, ref.inputs[5]["cotangents"]
    d = obs_device(case)
    dts = (DT, DT, 0.5 * DT, 0.5 * DT)                        # (the call that reaches position 5 runs under another dt)
    for kind in AO.KINDS:
        per_step, loss = sweep(d, case, kind, rec, final, dts=dts)
        checkpointed, loss_ckpt = sweep(d, case, kind, rec, final, checkpoint_every=K, dts=dts)
        assert np.array_equal(bits(checkpointed["state"]), bits(per_step["state"])), (case_id(case), kind)
        assert np.array_equal(bits(loss_ckpt), bits(loss))
        reference_dt, _ = sweep(d, case, kind, rec, final)
        assert np.any(per_step["state"] != reference_dt["state"])


# ---- 3. the adjoint identity on the device --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", AO.CASES, ids=case_id)
def test_adjoint_identity_against_the_tangent_in_the_same_pieces(case):
    ref = AO.reference(case)
    rec, final, dU = ref.record, ref.inputs[5]["cotangents"], ref.inputs[5]["state"]
    levels = rec["levels"]
    d = obs_device(case)
    d.restore_state()
    d.open_tangent()
    d.set_tangent("internal_energy", dU)
    d.tangent_closure()
    lhs = np.zeros(case[1], dtype=LD)
    at = 0
    for k, s in enumerate(POSITIONS):
        if s > at:
            d.step_tangent(DT, s - at)
            at = s
        t = np.stack([d.tangent(x) for x in TANGENTS])
        lhs += np.einsum("xic,xic->c", rec["linear"][k].astype(LD), t[:, levels].astype(LD))
    lhs += np.einsum("xic,xic->c", final.astype(LD), t.astype(LD))
    d.close_tangent()
    for checkpoint_every in (None, K):
        g, _ = sweep(d, case, "linear", rec, final, checkpoint_every, ride="state")
        rhs = np.einsum("jc,jc->c", g["state"].astype(LD), dU.astype(LD))
        expected, Ssum = ref.identity
        keep = ref.keep
        assert np.all(Ssum > 0)
        err = float(np.max(np.abs(lhs[keep] - rhs[keep]) / Ssum))
        both = float(max(np.max(np.abs(lhs[keep] - expected) / Ssum), np.max(np.abs(rhs[keep] - expected) / Ssum)))
        print(f"{case_id(case)}: identity {err:.3e}, against the reference {both:.3e}, bound {ref.bound():.3e}")
        assert err <= ref.bound() and both <= ref.bound(), (case_id(case), checkpoint_every, err, both, ref.bound())


# ---- 4. the primal is untouched --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SOME, ids=case_id)
@pytest.mark.parametrize("checkpoint_every", (None, K), ids=("per-step", "checkpointed"))
def test_primal_of_the_interleaved_record_calls_is_trm_step(case, checkpoint_every):
    ref = AO.reference(case)
    twin = stepped_twin(case)
    d = obs_device(case)
    for kind in AO.KINDS:
        sweep(d, case, kind, ref.record, ref.inputs[5]["cotangents"], checkpoint_every, on_recorded=lambda dev: assert_primal(dev, twin, case, "column_adjoint"))
        # the sweep and its injections leave the state, the status word and the clock where the record left them
        state, status, clock = twin
        for name in STATE:
            assert np.array_equal(bits(d.get(name)), state[name]), (case_id(case), kind, name)
        assert d.status() == status and d.clock() == clock


# ---- 5. bookkeeping --------------------------------------------------------------------------------------------------------------------
def code_of(call):
    with pytest.raises(trm.TerrariumHipError) as e:
        call()
    return e.value.code, str(e.value)


def test_observation_list_counts_bytes_and_lifetime():
    case = next(c for c in SOME if c[0] == 33 and c[5] is None)
    Nz, Nh = case[0], case[1]
    rec = AO.reference(case).record
    levels = rec["levels"]
    nl = len(levels)
    d = obs_device(case)
    # without an open adjoint: the wording of the other adjoint calls
    for call in (lambda: d.observe(levels, temperature=1.0), lambda: d.observe_misfit(levels, 0.0), d.misfit, d.adjoint_observations):
        code, msg = code_of(call)
        assert code == EINVAL and "no adjoint is open (trm_adjoint_open)" in msg, msg
    d.open_adjoint(STEPS)
    assert d.adjoint_observations() == (0, 0) and not d.misfit().any()
    d.observe(levels, temperature=rec["linear"][0][1])
    assert d.adjoint_observations() == (1, nl * Nh * 8 + nl * 4)
    d.observe(levels[:1], internal_energy=1.0, liquid_water_fraction=2.0)     # two observations of one level
    assert d.adjoint_observations() == (3, (nl + 2) * Nh * 8 + (nl + 2) * 4)
    d.step_record(DT, 2)
    d.observe_misfit(levels, rec["observed"][1])                               # no weights: one array
    d.observe_misfit(levels, rec["observed"][1], rec["weight"][1])             # two
    assert d.adjoint_observations() == (5, (4 * nl + 2) * Nh * 8 + (3 * nl + 2) * 4)
    assert np.all(d.misfit() > 0)
    assert d.adjoint_tape() == (2, STEPS)
    # bad arguments register nothing
    bad = [lambda: d.observe([], temperature=1.0), lambda: d.observe([0, 0], temperature=1.0), lambda: d.observe([1, 0], temperature=1.0),
           lambda: d.observe([-1], temperature=1.0), lambda: d.observe([Nz], temperature=1.0), lambda: d.observe_misfit([0], 1.0, -1.0),
           lambda: d.observe_misfit([0], 1.0, np.nan)]
    for call in bad:
        assert code_of(call)[0] == EINVAL
    L = trm._capi.lib()
    lv = np.zeros(1, dtype=np.int32)
    a = np.zeros(Nh)
    assert L.trm_adjoint_observe(d._ctx, 3, 1, lv.ctypes.data, a.ctypes.data) == EINVAL
    assert L.trm_adjoint_observe(d._ctx, 0, 1, None, a.ctypes.data) == EINVAL and L.trm_adjoint_observe(d._ctx, 0, 1, lv.ctypes.data, None) == EINVAL
    assert L.trm_adjoint_observe_misfit(d._ctx, 1, lv.ctypes.data, None, None) == EINVAL
    assert d.adjoint_observations()[0] == 5
    # opening again starts a fresh tape: no observations, no misfit
    d.open_adjoint(STEPS)
    assert d.adjoint_observations() == (0, 0) and not d.misfit().any()
    # a foreign step makes the tape stale: nothing is registered on it
    d.step_record(DT, 1)
    d.observe(levels, temperature=1.0)
    d.step(DT, 1)
    for call in (lambda: d.observe(levels, temperature=1.0), lambda: d.observe_misfit(levels, 0.0)):
        code, msg = code_of(call)
        assert code == ESTALE, msg
    assert d.adjoint_observations()[0] == 1
    assert code_of(d.adjoint_backward)[0] == ESTALE
    d.close_adjoint()
    d.open_adjoint(STEPS)
    assert d.adjoint_observations() == (0, 0)
    d.close_adjoint()


def test_a_mid_segment_observation_takes_a_checkpoint_slot():
    case = next(c for c in SOME if c[0] == 3 and c[5] is None)
    levels = AO.observed_levels(case[0])
    d = obs_device(case)
    # without observations the 6 steps take two slots of K = 4 ...
    d.restore_state()
    d.open_adjoint(2, K)
    d.step_record(DT, 3)
    d.step_record(DT, 2)
    d.step_record(DT, 1)
    assert d.adjoint_checkpoints() == (K, 2, 2)
    # ... an observation at 3 closes the segment of 3 steps, one at 5 the segment of 2: the last step needs a third slot
    d.restore_state()
    d.open_adjoint(2, K)
    d.step_record(DT, 3)
    d.observe(levels, temperature=1.0)
    d.observe(levels, internal_energy=1.0)                     # (a second one at the same position closes nothing more)
    assert d.adjoint_checkpoints() == (K, 1, 2)
    d.step_record(DT, 2)
    assert d.adjoint_checkpoints() == (K, 2, 2)
    d.observe_misfit(levels, 0.0)
    state, rest = {name: bits(d.get(name)) for name in STATE}, (d.status(), d.clock(), d.adjoint_tape())
    code, msg = code_of(lambda: d.step_record(DT, 1))
    assert code == EINVAL and "1 steps need 1 checkpoints (2 of 2 slots taken)" in msg, msg
    # nothing is stepped
    assert all(np.array_equal(bits(d.get(name)), state[name]) for name in STATE) and (d.status(), d.clock(), d.adjoint_tape()) == rest
    assert rest[2] == (5, 2 * K) and d.adjoint_observations()[0] == 3
    # the tape is still good: the sweep pulls the three observations back from position 5 = n
    d.adjoint_backward()
    assert d.adjoint_observations() == (0, 0) and d.adjoint_checkpoints() == (K, 0, 2)
    assert np.any(d.cotangent("internal_energy") != 0.0)
    d.close_adjoint()


def test_misfit_gradient_of_an_integrator_is_the_sweep_by_hand():
    """trm.misfit_gradient: the tape it sizes, the split of step_record at the record's steps, L and the tail of vjp"""
    Nz, Nh = 33, 13

    def column():
        grid = trm.ColumnGrid(trm.ExponentialSpacing(N=Nz), num_columns=Nh)
        model = trm.SoilModel(grid, initializer=trm.SoilInitializer())
        bcs = trm.merge_boundary_conditions(trm.PrescribedSurfaceTemperature("T_ub", 1.0))
        return trm.initialize(model, trm.ForwardEuler(), boundary_conditions=bcs)

    dt = trm.ForwardEuler().dt
    levels = AO.observed_levels(Nz)
    rng = np.random.default_rng(5)
    values = rng.normal(0.0, 2.0, (3, len(levels), Nh))
    values[1, 0, 2] = np.nan
    record = trm.TemperatureRecord([0, 3, 5], levels, values, weight=rng.uniform(0.5, 2.0, values.shape))
    out = {}
    for every in (None, K):
        integ = column()
        out[every] = trm.misfit_gradient(integ, record, steps=6, checkpoint_every=every, wrt_boundary=True, wrt_params=True)
        L, g, boundary, params = out[every]
        assert L.shape == (Nh,) and np.all(L > 0) and g.shape == (Nz, Nh) and np.any(g != 0.0)
        assert set(params) == set(PARAMS) and ("temperature", "top") in boundary
        assert trm.iteration(integ) == 6 and not getattr(integ.state, "_adjoint_open", False)
    assert np.array_equal(bits(out[K][0]), bits(out[None][0])) and np.array_equal(bits(out[K][1]), bits(out[None][1]))
    # by hand on the state
    st = column().state
    st.open_adjoint(6)
    st.observe_misfit(levels, values[0], record.weight[0])
    st.step_record(dt, 3)
    st.observe_misfit(levels, values[1], record.weight[1])
    st.step_record(dt, 2)
    st.observe_misfit(levels, values[2], record.weight[2])
    st.step_record(dt, 1)
    L = st.misfit()
    st.adjoint_backward()
    assert np.array_equal(bits(L), bits(out[None][0])) and np.array_equal(bits(st.cotangent("internal_energy")), bits(out[None][1]))
    st.close_adjoint()


def test_the_example_calibrates():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "borehole_calibration.py")
    spec = importlib.util.spec_from_file_location("borehole_calibration", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    history = ex.main(iterations=6)
    misfits = [L for L, _ in history]
    assert len(history) == 7 and all(b <= a for a, b in zip(misfits, misfits[1:])) and misfits[-1] < 0.1 * misfits[0], misfits
    first, last = history[0][1], history[-1][1]
    for name, truth in ex.TRUTH.items():                       # both parameters end closer to the truth than the guess was
        assert abs(np.log(last[name] / truth)) < abs(np.log(first[name] / truth)), (name, first, last)
