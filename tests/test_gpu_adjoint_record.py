"""Attached temperature records on the device (trm_adjoint_observe_record): a record given once, kept across sweeps and read inside the
backward launches, value by value against the exact Jacobian of tests/linearised_heat.py.

The cases, the records and the reference are adjoint_record.py's: the 48 cases of adjoint_observations.py with their record at the
positions 0, 3, 5 and 6 of a run of 6 steps (3 and 5 inside the launch of the steps 2 ... 5, inside the segments of K = 4), a dense
record -- every position 0 ... 6 on every level -- on (3, 13), (33, 13) and (64, 1), and the two ends alone on (2, 13).  Per case and
on both tapes dL/dU_0, the boundary gradients, the node gradients of a series, the ten parameter gradients and the misfit per column lie
within 8 x e_ref of the case and of the contraction itself.  Beside it the capability (no position takes a slot: 6 steps in 2 slots, a
sample at every one of 24 steps in 3), what needs no tolerance (null records, a NaN against a weight 0, doubling, the host's
resummation of the residuals, both tapes, persistence over sweeps, the zero-copy attach, the primal), the adjoint identity against
trm_step_tangent stopped at the positions, and the refusals on a live context."""
import numpy as np
import pytest

import adjoint_observations as AO
import adjoint_record as AR
import terrarium_jl_amd as trm
from boundary_derivatives import LD, PAIRS
from parameter_derivatives import PARAMS
from test_gpu_derivative_edges import DT, FACTOR, SERIES_PAIR, STEPS, assert_primal, case_id, report, stepped_twin
from test_gpu_adjoint_observations import code_of, obs_device, same_bits
from test_gpu_tangent import STATE, TANGENTS, bits

pytestmark = pytest.mark.gpu
K = AO.K
EINVAL = trm._capi.TRM_EINVAL
# a representative of every lane layout for the tests that need no reference's bound: both halves of the 32- and 64-lane layouts, a series
SOME = [rc for rc in AR.CASES if rc[1] in [c for c in AO.CASES if (c[0], c[1]) in ((3, 13), (33, 13), (64, 1)) and c[4] == 26.0 and c[2] in (AO.SERIES_SET, "flux_top+T_bottom")]]
TAPES = pytest.mark.parametrize("checkpoint_every", (None, K), ids=("per-step", "checkpointed"))


def slots(checkpoint_every, steps=STEPS):
    return steps if checkpoint_every is None else -(-steps // checkpoint_every)


def attach(d, rec, weight="given", device_arrays=False, keep=None):
    w = rec["weight"] if weight == "given" else weight
    if device_arrays:
        import torch
        dev = torch.device("cuda", int(d.grid.device))
        obs_t = torch.as_tensor(np.ascontiguousarray(rec["observed"]), device=dev)
        w_t = None if w is None else torch.as_tensor(np.array(np.broadcast_to(w, rec["observed"].shape)), device=dev)
        torch.cuda.synchronize(dev)
        d.attach_record(rec["positions"], rec["levels"], obs_t, w_t)
    else:
        d.attach_record(rec["positions"], rec["levels"], rec["observed"], w)


def gradients(d, case, ride):
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
    return out


def record_and_sweep(d, case, final, checkpoint_every, ride, pieces, scale=1.0, with_record=True):
    """one round on the open tape: U_0 back, the run recorded in `pieces` [(dt, steps)], the final cotangents, one sweep"""
    d.restore_state()
    for dt, n in pieces:
        d.step_record(dt, n)
    for x, wx in zip(TANGENTS, final):
        d.set_cotangent(x, wx * scale)
    d.adjoint_backward()
    prog = d.last_program()
    assert prog["family"] == "column_adjoint" and prog["backward"] and prog["checkpointed"] == (checkpoint_every is not None), (case_id(case), prog)
    assert prog["parameter_gradient"] == (ride == "params") and prog["lanes_per_column"] == (32 if case[0] <= 32 else 64), (case_id(case), prog)
    out = gradients(d, case, ride)
    if with_record:
        assert d.adjoint_observations() == (0, 0)
        return out, d.record_misfit(), d.record_residuals()
    return out, None, None


def sweep(d, case, rec, final, checkpoint_every=None, ride="params", pieces=((DT, STEPS),), scale=1.0, weight="given", device_arrays=False):
    """{input: gradient}, the misfit per column and the residuals of the saved state with `rec` attached (None: no record) on a fresh tape"""
    d.restore_state()
    d.open_adjoint(slots(checkpoint_every) if len(pieces) == 1 else (STEPS if checkpoint_every is None else len(pieces)), checkpoint_every)
    if ride == "boundary":
        d.open_bc_gradient()
    if ride == "params":
        d.open_param_gradient()
    if rec is not None:
        attach(d, rec, weight, device_arrays)
    out = record_and_sweep(d, case, final, checkpoint_every, ride, pieces, scale, rec is not None)
    d.close_adjoint()
    return out


def report_each(ref, figures):
    """report of test_gpu_derivative_edges.py (every figure within the bound of the case), and every figure within FACTOR x e_ref of
    its own contraction as well"""
    report(ref, figures)
    over = {label: (err, ref.parts[label.split(" [")[0]]) for label, err in figures.items() if not err <= FACTOR * ref.parts[label.split(" [")[0]]}
    assert not over, (AR.record_id(ref.rcase), "beyond FACTOR x e_ref of the contraction itself", over)


# ---- 1. the exact Jacobian -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rcase", AR.CASES, ids=AR.record_id)
def test_gradients_and_misfit_match_the_exact_jacobian(rcase):
    ref = AR.reference(rcase)
    case = rcase[1]
    rec, final = ref.record, ref.inputs[5]["cotangents"]
    d = obs_device(case)
    rides = ("params",) if case[5] else ("state", "boundary", "params")
    figures = {}
    for ride in rides:
        for tape, every in (("per-step", None), ("checkpointed", K)):
            grads, misfit, _ = sweep(d, case, rec, final, every, ride)
            for key, g in grads.items():
                figures[f"misfit gradient {key} [{ride}, {tape}]"] = ref.error(f"misfit gradient {key}", g)
            figures[f"misfit loss [{ride}, {tape}]"] = ref.error("misfit loss", misfit)
    assert np.any(grads["params"][PARAMS.index("k_organic")] != 0.0) or case[4] != 26.0
    report_each(ref, figures)


# ---- 2. the capability -----------------------------------------------------------------------------------------------------------------
def test_no_position_takes_a_checkpoint_slot():
    rcase = next(rc for rc in SOME if rc[0] == "AO" and rc[1][0] == 33 and rc[1][5] is None)
    case, rec = rcase[1], AR.reference(rcase).record
    d = obs_device(case)
    # K = 4 and 6 steps: 2 slots with the record attached, whatever the pieces ...
    for pieces in ((6,), (3, 2, 1)):
        d.restore_state()
        d.open_adjoint(2, K)
        attach(d, rec)
        for n in pieces:
            d.step_record(DT, n)
        assert d.adjoint_checkpoints() == (K, 2, 2) and d.adjoint_tape() == (6, 2 * K) and d.adjoint_observations() == (0, 0)
        d.adjoint_backward()
        assert d.adjoint_checkpoints() == (K, 0, 2) and d.record_info()[:2] == (4, len(rec["levels"]))
        d.close_adjoint()
    # ... the per-position path takes 3
    d.restore_state()
    d.open_adjoint(3, K)
    at = 0
    for k, s in enumerate(rec["positions"]):
        if s > at:
            d.step_record(DT, s - at)
            at = s
        d.observe_misfit(rec["levels"], rec["observed"][k], rec["weight"][k])
    assert d.adjoint_checkpoints() == (K, 3, 3)
    d.close_adjoint()


def test_a_sample_at_every_step_fits_the_checkpointed_tape():
    case = next(rc for rc in SOME if rc[0] == "dense" and rc[1][0] == 33 and rc[1][5] is None)[1]
    Nz, Nh = case[0], case[1]
    steps, every, cap = 24, 8, 3
    rng = np.random.default_rng(24)
    levels = list(range(Nz))
    observed = rng.normal(0.0, 2.0, (steps + 1, Nz, Nh))
    d = obs_device(case)
    d.restore_state()
    d.open_adjoint(cap, every)
    d.attach_record(list(range(steps + 1)), levels, observed)
    d.step_record(DT, steps)
    assert d.adjoint_checkpoints() == (every, cap, cap) and d.adjoint_observations() == (0, 0)
    d.adjoint_backward()
    r = d.record_residuals()
    assert r.shape == observed.shape and np.all(np.isfinite(r)) and np.all(d.record_misfit() > 0) and np.any(d.cotangent("internal_energy") != 0.0)
    assert d.record_info() == (steps + 1, Nz, 2 * observed.size * 8 + Nh * 8 + (Nz + steps + 1) * 4)
    d.close_adjoint()
    # the same run through observe_misfit: a slot per sample, refused by trm_step_record for lack of slots
    d.restore_state()
    d.open_adjoint(cap, every)
    taken = 0
    with pytest.raises(trm.TerrariumHipError) as e:
        for s in range(steps):
            d.observe_misfit(levels, observed[s])
            d.step_record(DT, 1)
            taken += 1
    assert e.value.code == EINVAL and "1 steps need 1 checkpoints (3 of 3 slots taken)" in str(e.value) and taken == cap
    d.close_adjoint()


# ---- 3. what needs no tolerance --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rcase", SOME, ids=AR.record_id)
@TAPES
def test_null_records_gaps_and_doubling_bit_for_bit(rcase, checkpoint_every):
    ref = AR.reference(rcase)
    case, rec, final = rcase[1], ref.record, ref.inputs[5]["cotangents"]
    d = obs_device(case)
    what = (AR.record_id(rcase),)
    # (a) a record of gaps alone, or of weights 0 alone: the bits of the sweep without a record, residuals +0.0
    plain, _, _ = sweep(d, case, None, final, checkpoint_every)
    full, misfit_full, r_full = sweep(d, case, rec, final, checkpoint_every)
    assert any(np.any(full[key] != plain[key]) for key in full), what + ("the record changes the gradient",)
    for null in (dict(rec, observed=np.full_like(rec["observed"], np.nan)), dict(rec, weight=np.zeros_like(rec["weight"]))):
        got, misfit, r = sweep(d, case, null, final, checkpoint_every)
        same_bits(got, plain, what + ("a null record",))
        assert not misfit.any() and np.array_equal(bits(r), bits(np.zeros_like(r)))
    # (b) a NaN sample is that sample's weight 0
    gap, holed = dict(rec, observed=rec["observed"].copy()), dict(rec, weight=rec["weight"].copy())
    Nh = case[1]
    for k, (j, c) in zip((0, 1, len(rec["positions"]) - 1), [(0, 0), (-1, Nh - 1), (-1, Nh // 2)]):
        gap["observed"][k, j, c] = np.nan
        holed["weight"][k, j, c] = 0.0
    with_gap, misfit_gap, r_gap = sweep(d, case, gap, final, checkpoint_every)
    with_zero, misfit_zero, r_zero = sweep(d, case, holed, final, checkpoint_every)
    same_bits(with_gap, with_zero, what + ("a NaN sample against its weight 0",))
    assert np.array_equal(bits(misfit_gap), bits(misfit_zero)) and np.array_equal(bits(r_gap), bits(r_zero)) and np.all(np.isfinite(misfit_gap))
    assert np.any(misfit_gap != misfit_full) and r_gap[0, 0, 0] == 0.0 and not np.signbit(r_gap[0, 0, 0])
    # (c) zero final cotangents: twice the weights, twice every gradient bit and the misfit
    zero = np.zeros_like(final)
    once, misfit1, r1 = sweep(d, case, rec, zero, checkpoint_every)
    twice, misfit2, r2 = sweep(d, case, dict(rec, weight=2.0 * rec["weight"]), zero, checkpoint_every)
    same_bits(twice, {key: 2.0 * g for key, g in once.items()}, what + ("weights times 2",))
    assert np.array_equal(bits(misfit2), bits(2.0 * misfit1)) and np.array_equal(bits(r2), bits(r1)) and np.any(once["state"] != 0.0)
    # no weights: the weights 1
    ones, misfit_ones, _ = sweep(d, case, dict(rec, weight=np.ones_like(rec["weight"])), final, checkpoint_every)
    none, misfit_none, _ = sweep(d, case, rec, final, checkpoint_every, weight=None)
    same_bits(none, ones, what + ("no weights",))
    assert np.array_equal(bits(misfit_none), bits(misfit_ones))
    # (d) the misfit is the host's sequential float64 sum over the residuals: positions ascending, levels in list order
    s = np.zeros(Nh)
    for k in range(r_full.shape[0]):
        for j in range(r_full.shape[1]):
            s = s + 0.5 * rec["weight"][k, j] * r_full[k, j] * r_full[k, j]
    assert np.array_equal(bits(misfit_full), bits(s))


@pytest.mark.parametrize("rcase", SOME, ids=AR.record_id)
def test_both_tapes_give_the_same_bits(rcase):
    ref = AR.reference(rcase)
    case, rec, final = rcase[1], ref.record, ref.inputs[5]["cotangents"]
    d = obs_device(case)
    # (e) also across a change of dt inside the run: positions on both sides of the change and at it
    assert 3 in rec["positions"] or rcase[0] != "AO"
    runs = [((DT, STEPS),)] + ([] if case[5] else [((DT, 3), (2.0 * DT, 3))])
    for pieces in runs:
        per_step, misfit, r = sweep(d, case, rec, final, None, pieces=pieces)
        checkpointed, misfit_ckpt, r_ckpt = sweep(d, case, rec, final, K, pieces=pieces)
        assert np.array_equal(bits(checkpointed["state"]), bits(per_step["state"])), (AR.record_id(rcase), pieces)
        assert np.array_equal(bits(r_ckpt), bits(r)) and np.array_equal(bits(misfit_ckpt), bits(misfit))
    one_dt, _, _ = sweep(d, case, rec, final, None)
    assert case[5] or np.any(per_step["state"] != one_dt["state"])


@pytest.mark.parametrize("rcase", SOME, ids=AR.record_id)
@TAPES
def test_record_persists_over_sweeps_and_detaches(rcase, checkpoint_every):
    ref = AR.reference(rcase)
    case, rec, final = rcase[1], ref.record, ref.inputs[5]["cotangents"]
    d = obs_device(case)
    pieces = ((DT, STEPS),)
    plain, _, _ = sweep(d, case, None, final, checkpoint_every)
    twin = stepped_twin(case)
    # (f) two rounds of upload-U_0 / record / sweep on one attachment
    d.restore_state()
    d.open_adjoint(slots(checkpoint_every), checkpoint_every)
    d.open_param_gradient()
    attach(d, rec)
    info = d.record_info()
    for code, msg in (code_of(d.record_misfit), code_of(d.record_residuals)):              # (no sweep has run with this record)
        assert code == EINVAL and "no sweep has run with this record" in msg, msg
    d.restore_state()
    d.step_record(DT, STEPS)
    assert_primal(d, twin, case, "column_adjoint")                                          # (g) the primal is trm_step's
    d.adjoint_backward()                                                                    # (zero final cotangents: a sweep of its own)
    first = record_and_sweep(d, case, final, checkpoint_every, "params", pieces)
    second = record_and_sweep(d, case, final, checkpoint_every, "params", pieces)
    same_bits(second[0], first[0], (AR.record_id(rcase), "the second round"))
    assert np.array_equal(bits(second[1]), bits(first[1])) and np.array_equal(bits(second[2]), bits(first[2]))
    assert d.record_info()[:2] == info[:2] == (len(rec["positions"]), len(rec["levels"])) and d.record_info()[2] > info[2]
    assert np.any(first[0]["state"] != plain["state"])
    # detached: the sweep without a record
    d.detach_record()
    assert d.record_info() == (0, 0, 0)
    assert code_of(d.record_misfit)[0] == EINVAL and code_of(d.detach_record)[0] == EINVAL
    after, _, _ = record_and_sweep(d, case, final, checkpoint_every, "params", pieces, with_record=False)
    same_bits(after, plain, (AR.record_id(rcase), "after the detach"))
    # the device-pointer attach: the host attach's bits
    attach(d, rec, device_arrays=True)
    zero_copy = record_and_sweep(d, case, final, checkpoint_every, "params", pieces)
    same_bits(zero_copy[0], first[0], (AR.record_id(rcase), "device arrays"))
    assert np.array_equal(bits(zero_copy[1]), bits(first[1])) and np.array_equal(bits(zero_copy[2]), bits(first[2]))
    assert d.record_info()[2] < info[2]                                                    # (the arrays stay the caller's)
    d.close_adjoint()


# ---- 4. the adjoint identity on the device ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rcase", [rc for rc in AR.CASES if rc[0] != "AO" or rc[1][4] == 26.0], ids=AR.record_id)
def test_adjoint_identity_against_the_tangent_stopped_at_the_positions(rcase):
    ref = AR.reference(rcase)
    case, rec = rcase[1], ref.record
    final, dU = ref.inputs[5]["cotangents"], ref.inputs[5]["state"]
    levels = rec["levels"]
    d = obs_device(case)
    for checkpoint_every in (None, K):
        g, _, r = sweep(d, case, rec, final, checkpoint_every, ride="state")
        d.restore_state()
        d.open_tangent()
        d.set_tangent("internal_energy", dU)
        d.tangent_closure()
        lhs = np.zeros(case[1], dtype=LD)
        at = 0
        for k, s in enumerate(rec["positions"]):
            if s > at:
                d.step_tangent(DT, s - at)
                at = s
            dT = d.tangent("temperature")
            lhs += np.einsum("ic,ic->c", (rec["weight"][k] * r[k]).astype(LD), dT[levels].astype(LD))
        t = np.stack([d.tangent(x) for x in TANGENTS])
        lhs += np.einsum("xic,xic->c", final.astype(LD), t.astype(LD))
        d.close_tangent()
        rhs = np.einsum("jc,jc->c", g["state"].astype(LD), dU.astype(LD))
        expected, Ssum = ref.identity
        keep = ref.keep
        assert np.all(Ssum > 0)
        err = float(np.max(np.abs(lhs[keep] - rhs[keep]) / Ssum))
        both = float(max(np.max(np.abs(lhs[keep] - expected) / Ssum), np.max(np.abs(rhs[keep] - expected) / Ssum)))
        print(f"{AR.record_id(rcase)}: identity {err:.3e}, against the reference {both:.3e}, bound {ref.bound():.3e}")
        assert err <= ref.bound() and both <= ref.bound(), (AR.record_id(rcase), checkpoint_every, err, both, ref.bound())


# ---- 5. refusals on a live context -----------------------------------------------------------------------------------------------------
def test_refusals_on_a_live_context():
    rcase = next(rc for rc in SOME if rc[0] == "AO" and rc[1][0] == 33 and rc[1][5] is None)
    case, rec = rcase[1], AR.reference(rcase).record
    levels = rec["levels"]
    d = obs_device(case)
    # without an open adjoint: the words of the other adjoint calls
    for call in (lambda: attach(d, rec), d.detach_record, d.record_misfit, d.record_info):
        code, msg = code_of(call)
        assert code == EINVAL and "no adjoint is open (trm_adjoint_open)" in msg, msg
    d.restore_state()
    d.open_adjoint(STEPS)
    assert d.record_info() == (0, 0, 0)
    # bad arguments attach nothing
    obs, w = rec["observed"], rec["weight"]
    bad = [lambda: d.attach_record([], levels, 0.0), lambda: d.attach_record([0, 3], [], 0.0), lambda: d.attach_record([-1, 2], levels, 0.0),
           lambda: d.attach_record([0, 3, 3], levels, 0.0), lambda: d.attach_record([3, 0], levels, 0.0), lambda: d.attach_record([0], [case[0]], 0.0),
           lambda: d.attach_record([0], [1, 0], 0.0), lambda: d.attach_record([0], levels, 0.0, -1.0), lambda: d.attach_record([0], levels, 0.0, np.nan)]
    for call in bad:
        assert code_of(call)[0] == EINVAL
    assert d.record_info() == (0, 0, 0)
    # the two paths do not mix, either way
    d.observe(levels, temperature=1.0)
    code, msg = code_of(lambda: attach(d, rec))
    assert code == EINVAL and "the two paths do not mix" in msg, msg
    d.open_adjoint(STEPS)
    attach(d, rec)
    for call in (lambda: d.observe(levels, temperature=1.0), lambda: d.observe_misfit(levels, 0.0)):
        code, msg = code_of(call)
        assert code == EINVAL and "a temperature record is attached" in msg and "the two paths do not mix" in msg, msg
    code, msg = code_of(lambda: attach(d, rec))
    assert code == EINVAL and "a record is attached already" in msg, msg
    assert d.adjoint_observations() == (0, 0) and d.record_info()[:2] == (len(rec["positions"]), len(levels))
    # a record longer than the tape: refused before anything is launched, the tape survives, the sweep after more steps succeeds
    d.step_record(DT, 4)
    state = {name: bits(d.get(name)) for name in STATE}
    lam = d.cotangent("internal_energy")
    code, msg = code_of(d.adjoint_backward)
    assert code == EINVAL and "the attached record is longer than the tape: position 6 of 4 taped steps" in msg, msg
    assert d.adjoint_tape() == (4, STEPS) and all(np.array_equal(bits(d.get(name)), state[name]) for name in STATE)
    assert np.array_equal(bits(d.cotangent("internal_energy")), bits(lam))
    assert code_of(d.record_misfit)[0] == EINVAL
    d.step_record(DT, 2)
    d.adjoint_backward()
    assert d.adjoint_tape() == (0, STEPS) and np.all(d.record_misfit() > 0) and np.any(d.cotangent("internal_energy") != 0.0)
    # attaching with steps on the tape: positions count from the tape's start
    d.detach_record()
    d.restore_state()
    d.step_record(DT, 3)
    attach(d, rec)
    d.step_record(DT, 3)
    d.adjoint_backward()
    late = d.record_residuals()
    d.open_adjoint(STEPS)                                          # (a new tape drops the record)
    assert d.record_info() == (0, 0, 0)
    attach(d, rec)
    d.restore_state()
    d.step_record(DT, STEPS)
    d.adjoint_backward()
    assert np.array_equal(bits(d.record_residuals()), bits(late))
    d.close_adjoint()
    # the model kinds the adjoint refuses keep refusing in their words, and have no adjoint to attach to
    from test_gpu_derivative_refusals import context
    for kind, why in (("f32", "fp64 contexts only"), ("richards", "the heat-only SoilModel (NoFlow) only")):
        other = context(kind)
        code, msg = code_of(lambda: other.open_adjoint(2))
        assert code == trm._capi.TRM_EUNSUPPORTED and why in msg, msg
        code, msg = code_of(lambda: other.attach_record([0], [0], 0.0))
        assert code == EINVAL and "no adjoint is open (trm_adjoint_open)" in msg, msg
        other.close()


# ---- 6. the Python interface -----------------------------------------------------------------------------------------------------------
def test_record_gradient_of_an_integrator_is_the_sweep_by_hand():
    """trm.record_gradient: one attach, one step_record, one sweep on a tape of ceil(steps / K) slots; what misfit_gradient returns"""
    Nz, Nh = 33, 13

    def column():
        grid = trm.ColumnGrid(trm.ExponentialSpacing(N=Nz), num_columns=Nh)
        model = trm.SoilModel(grid, initializer=trm.SoilInitializer())
        bcs = trm.merge_boundary_conditions(trm.PrescribedSurfaceTemperature("T_ub", 1.0))
        return trm.initialize(model, trm.ForwardEuler(), boundary_conditions=bcs)

    dt = trm.ForwardEuler().dt
    levels = AO.observed_levels(Nz)
    rng = np.random.default_rng(5)
    values = rng.normal(0.0, 2.0, (7, len(levels), Nh))
    values[1, 0, 2] = np.nan
    record = trm.TemperatureRecord(list(range(7)), levels, values, weight=rng.uniform(0.5, 2.0, values.shape))
    out = {}
    for every in (None, K):
        integ = column()
        out[every] = trm.record_gradient(integ, record, steps=6, checkpoint_every=every, wrt_boundary=True, wrt_params=True)
        L, g, boundary, params = out[every]
        assert L.shape == (Nh,) and np.all(L > 0) and g.shape == (Nz, Nh) and np.any(g != 0.0)
        assert set(params) == set(PARAMS) and ("temperature", "top") in boundary
        assert trm.iteration(integ) == 6 and not getattr(integ.state, "_adjoint_open", False)
    assert np.array_equal(bits(out[K][0]), bits(out[None][0])) and np.array_equal(bits(out[K][1]), bits(out[None][1]))
    # by hand on the state: the dense record on two slots of K = 4
    st = column().state
    st.open_adjoint(2, K)
    st.attach_record(record.steps, levels, values, record.weight)
    st.step_record(dt, 6)
    assert st.adjoint_checkpoints() == (K, 2, 2)
    st.adjoint_backward()
    assert np.array_equal(bits(st.record_misfit()), bits(out[K][0])) and np.array_equal(bits(st.cotangent("internal_energy")), bits(out[K][1]))
    st.close_adjoint()
    # one sample per position
    with pytest.raises(ValueError):
        trm.record_gradient(column(), trm.TemperatureRecord([0, 3, 3], levels, values[:3]), steps=6)


def test_the_dense_example_calibrates_on_fifteen_slots():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "borehole_calibration_dense.py")
    spec = importlib.util.spec_from_file_location("borehole_calibration_dense", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    history = ex.main(iterations=6)
    misfits = [L for L, _, _ in history]
    assert len(history) == 7 and all(b <= a for a, b in zip(misfits, misfits[1:])) and misfits[-1] < 0.1 * misfits[0], misfits
    assert all(used == 15 for _, _, used in history)            # 240 samples, 240 / 16 slots
    first, last = history[0][1], history[-1][1]
    for name, truth in ex.TRUTH.items():
        assert abs(np.log(last[name] / truth)) < abs(np.log(first[name] / truth)), (name, first, last)


# ---- the attached path beside the per-position path: a figure, no assertion ----------------------------------------------------------
@pytest.mark.parametrize("case", AO.CASES, ids=case_id)
def test_report_the_difference_to_the_per_position_path(case):
    from test_gpu_adjoint_observations import sweep as per_position_sweep
    ref = AR.reference(("AO", case))
    final = ref.inputs[5]["cotangents"]
    d = obs_device(case)
    theirs, _ = per_position_sweep(d, case, "misfit", dict(ref.record, observed=list(ref.record["observed"]), weight=list(ref.record["weight"])), final, ride="state")
    mine, _, _ = sweep(d, case, ref.record, final, None, ride="state")
    same = np.array_equal(bits(mine["state"]), bits(theirs["state"]))
    _, Ssum = ref.expected["misfit gradient state"]
    diff = np.abs(mine["state"].astype(LD) - theirs["state"].astype(LD))[..., ref.keep]
    worst = float(np.max(np.where(Ssum > 0, diff / np.where(Ssum > 0, Ssum, 1), 0)) / ref.e_ref)
    print(f"ATTACHED-VS-PER-POSITION {case_id(case)}: dL/dU_0 bit-identical = {same}, largest difference {worst:.3e} e_ref")
