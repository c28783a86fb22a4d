"""The checkpointed adjoint tape (trm_adjoint_open_checkpointed, trm.vjp(..., checkpoint_every=K)).

The record keeps the internal energy before every K-th step alone; the backward launch of a segment forms the states in between again
by re-running the recorded steps, and applies the per-step tape's transposed step to them.  The recomputed states are the recorded
ones bit for bit and the transposed step is one function, so every comparison here is bit for bit with the per-step tape: no
tolerance appears in this file.  The per-step adjoint's own tests (test_gpu_adjoint) carry the comparison with the tangent program
and the oracle."""
import numpy as np
import pytest

import workloads as W
import terrarium_jl_amd as trm
from test_gpu_tangent import CAPI, DT, STATE, TANGENTS, bits, boundary_sets, code_of, device, load_example, mixed_state, params, small
from test_gpu_adjoint import cotangents, pull_back

pytestmark = pytest.mark.gpu

COLUMNS = 48
CASES = [(Nz, bcset, halo) for Nz in (10, 32, 50) for bcset in ("T_top+flux_bottom", "gradient_top+flux_bottom")
         for halo in ("reference_zero", "mirror")]
MAX_K = CAPI.ADJOINT_MAX_INTERVAL


def case_device(Nz, bcset, halo, Nh=COLUMNS, steps_per_launch=0, seed=29):
    p = params(halo)
    U, sat = mixed_state(Nz, Nh, p, seed=seed)
    return device(Nz, Nh, p, U, sat, boundary_sets(Nh)[bcset], steps_per_launch=steps_per_launch)


def pull_back_checkpointed(d, calls, w, K, slots=None):
    """pull_back of test_gpu_adjoint on a checkpointed tape of interval K; `slots` defaults to what one segment per K steps of each call needs"""
    d.restore_state()
    d.open_adjoint(slots or max(1, sum(-(-n // K) for _, n in calls)), checkpoint_every=K)
    for dt, n in calls:
        d.step_record(dt, n)
    for name in TANGENTS:
        d.set_cotangent(name, w.get(name, 0.0))
    d.adjoint_backward()
    return d.cotangent("internal_energy")


# ---- 1. the recorded primal: bit for bit what trm_step computes -------------------------------------------------------------------
@pytest.mark.parametrize("Nz,bcset,halo", CASES)
def test_checkpointed_record_is_trm_step_bit_for_bit(Nz, bcset, halo):
    K, n = 4, 11
    a = case_device(Nz, bcset, halo, steps_per_launch=5)     # launches of steps 0-4, 5-9 and 10; checkpoints at 0, 4 and 8: the launches
    b = case_device(Nz, bcset, halo)                         # straddle segment boundaries and the last one stores nothing
    a.open_adjoint(3, checkpoint_every=K)
    a.step_record(DT, n)
    b.step(DT, n, finalize=True)
    for name in STATE:
        assert np.array_equal(bits(a.get(name)), bits(b.get(name))), name
    assert a.status() == b.status() and a.clock() == b.clock()
    assert a.adjoint_checkpoints() == (K, 3, 3) and a.adjoint_tape() == (n, 3 * K)
    prog = a.last_program()
    assert prog["family"] == "column_adjoint" and prog["checkpointed"] and not prog["backward"]
    assert prog["lanes_per_column"] == (32 if Nz <= 32 else 64)
    assert prog["generic_boundaries"] == bool(b.get_option("info_generic_boundary_kernels")) == bcset.startswith("gradient")


# ---- 2. the gradient: bit for bit the per-step tape's ---------------------------------------------------------------------------------
SHAPES = [(4, 11, 5), (16, 17, 0), (32, 40, 0), (1, 6, 0), (4, 0, 0)]     # (K, n, steps_per_launch): segments 4 4 3 | 16 1 | 32 8 | 1 x 6 | none


@pytest.fixture(scope="module")
def per_step_gradients():
    """{(case, n, steps_per_launch): g of the per-step tape}, computed once per key"""
    cache = {}

    def get(Nz, bcset, halo, n, spl):
        key = (Nz, bcset, halo, n, spl)
        if key not in cache:
            d = case_device(Nz, bcset, halo, steps_per_launch=spl)
            d.save_state()
            g = pull_back(d, [(DT, n)], cotangents(Nz, COLUMNS, 61))
            prog = d.last_program()
            assert prog["family"] == "column_adjoint" and prog["backward"] and not prog["checkpointed"]
            g.setflags(write=False)
            cache[key] = g
        return cache[key]
    return get


@pytest.mark.parametrize("K,n,spl", SHAPES)
@pytest.mark.parametrize("Nz,bcset,halo", CASES)
def test_checkpointed_gradient_is_the_per_step_tapes_bit_for_bit(Nz, bcset, halo, K, n, spl, per_step_gradients):
    g_ref = per_step_gradients(Nz, bcset, halo, n, spl)
    d = case_device(Nz, bcset, halo, steps_per_launch=spl)
    d.save_state()
    g = pull_back_checkpointed(d, [(DT, n)], cotangents(Nz, COLUMNS, 61), K)
    prog = d.last_program()
    assert prog["family"] == "column_adjoint" and prog["backward"] and prog["checkpointed"]
    assert prog["lanes_per_column"] == (32 if Nz <= 32 else 64) and prog["generic_boundaries"] == bcset.startswith("gradient")
    assert np.any(g_ref != 0.0) and np.all(np.isfinite(g_ref))
    assert np.array_equal(bits(g), bits(g_ref))
    assert d.adjoint_checkpoints()[1] == 0 and d.adjoint_tape()[0] == 0
    assert np.all(d.cotangent("temperature") == 0.0) and np.all(d.cotangent("liquid_water_fraction") == 0.0)      # folded in


@pytest.mark.parametrize("Nz,bcset", [(32, "T_top+flux_bottom"), (50, "gradient_top+flux_bottom")])
def test_clamped_tail_lanes(Nz, bcset):
    """13 columns: the one workgroup and its last wave carry clamped tail lanes, which recompute and store nothing"""
    Nh, K, n = 13, 4, 11
    d = case_device(Nz, bcset, "reference_zero", Nh=Nh, steps_per_launch=5)
    d.save_state()
    w = cotangents(Nz, Nh, 67)
    g_ref = pull_back(d, [(DT, n)], w)
    g = pull_back_checkpointed(d, [(DT, n)], w, K)
    assert np.any(g_ref != 0.0) and np.array_equal(bits(g), bits(g_ref))


# ---- 3. dt changes: every segment has one dt -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("bcset", ["T_top+flux_bottom", "gradient_top+flux_bottom"])
def test_a_change_of_dt_opens_a_segment(bcset):
    Nz, K, cap = 32, 4, 6
    calls = [(DT, 3), (0.5 * DT, 6), (DT, 2)]                      # segments 3 | 4, 2 | 2
    d = case_device(Nz, bcset, "reference_zero", steps_per_launch=3)
    d.save_state()
    w = cotangents(Nz, COLUMNS, 71)
    g_ref = pull_back(d, calls, w)
    d.restore_state()
    d.open_adjoint(cap, checkpoint_every=K)
    for dt, n in calls:
        d.step_record(dt, n)
    assert d.adjoint_checkpoints() == (K, 4, cap) and d.adjoint_tape() == (11, cap * K)
    for name in TANGENTS:
        d.set_cotangent(name, w[name])
    d.adjoint_backward()
    assert np.any(g_ref != 0.0) and np.array_equal(bits(d.cotangent("internal_energy")), bits(g_ref))
    assert d.adjoint_checkpoints() == (K, 0, cap)


# ---- 4. capacity ------------------------------------------------------------------------------------------------------------------------
def test_recording_past_the_checkpoint_capacity_is_refused_and_changes_nothing():
    E, I = CAPI.TRM_EINVAL, CAPI.TRM_OK
    d = small()
    d.open_adjoint(3, checkpoint_every=16)
    for n in (20, 20, 8):                                          # 48 steps: segments 16 16 16, the calls end inside segments
        assert code_of(d.step_record, DT, n) == I
    assert d.adjoint_checkpoints() == (16, 3, 3) and d.adjoint_tape() == (48, 48)
    before = {name: d.get(name) for name in STATE}
    clock, status = d.clock(), d.status()
    assert code_of(d.step_record, DT, 1) == E
    assert d.adjoint_checkpoints() == (16, 3, 3) and d.adjoint_tape() == (48, 48)
    for name in STATE:
        assert np.array_equal(bits(d.get(name)), bits(before[name])), name
    assert d.clock() == clock and d.status() == status
    assert code_of(d.step_record, DT, 0) == I
    assert code_of(d.adjoint_backward) == I
    assert d.adjoint_checkpoints() == (16, 0, 3) and d.adjoint_tape() == (0, 48)
    # a call that needs more slots than are left steps nothing, even where its first steps would fit
    d.open_adjoint(2, checkpoint_every=4)
    assert code_of(d.step_record, DT, 6) == I
    clock = d.clock()
    assert code_of(d.step_record, DT, 3) == E                      # 2 fit the open segment, the third needs a slot
    assert d.clock() == clock and d.adjoint_tape() == (6, 8)
    assert code_of(d.step_record, DT, 2) == I
    assert code_of(d.step_record, 0.5 * DT, 1) == E                # another dt: a new segment
    assert code_of(d.adjoint_backward) == I


# ---- 5. refusals, staleness, the two modes -----------------------------------------------------------------------------------------
def test_refusals():
    U, E, I = CAPI.TRM_EUNSUPPORTED, CAPI.TRM_EINVAL, CAPI.TRM_OK
    d = small()
    assert code_of(d.open_adjoint, 4, 0) == E
    assert code_of(d.open_adjoint, 4, -1) == E
    assert code_of(d.open_adjoint, 4, MAX_K + 1) == E
    assert code_of(d.open_adjoint, 0, 16) == E
    assert code_of(d.adjoint_checkpoints) == E                     # none of them opened anything
    assert code_of(d.open_adjoint, 4, MAX_K) == I
    assert d.adjoint_checkpoints() == (MAX_K, 0, 4)
    assert code_of(small(dtype=np.float32).open_adjoint, 4, 16) == U
    rich = params()
    rich.flow = CAPI.FLOW["richards"]
    assert code_of(small(p=rich).open_adjoint, 4, 16) == U


@pytest.mark.parametrize("change", ["step", "set_bc"])
def test_state_changes_make_the_checkpointed_tape_stale(change):
    S, I = CAPI.TRM_ESTALE, CAPI.TRM_OK
    d = small()
    d.open_adjoint(8, checkpoint_every=4)
    d.step_record(DT, 2)
    {"step": lambda: d.step(DT, 1), "set_bc": lambda: d.set_bc("temperature", "top", "value", 2.0)}[change]()
    clock = d.clock()
    assert code_of(d.adjoint_backward) == S
    assert code_of(d.step_record, DT, 1) == S
    assert d.adjoint_tape() == (2, 32) and d.adjoint_checkpoints() == (4, 1, 8) and d.clock() == clock
    d.open_adjoint(8, checkpoint_every=4)                           # a fresh tape
    assert d.adjoint_checkpoints() == (4, 0, 8)
    assert code_of(d.step_record, DT, 1) == I
    assert code_of(d.adjoint_backward) == I


def test_changes_before_the_first_taped_step_do_not_make_the_tape_stale():
    I = CAPI.TRM_OK
    d = small()
    d.open_adjoint(4, checkpoint_every=4)
    d.step(DT, 1)
    d.set_bc("temperature", "top", "value", 2.0)
    assert code_of(d.step_record, DT, 2) == I
    assert code_of(d.adjoint_backward) == I
    d.step(DT, 1)                                                  # the sweep has emptied the tape
    assert code_of(d.step_record, DT, 1) == I
    assert code_of(d.adjoint_backward) == I


def test_reopening_in_the_other_mode_replaces_the_tape():
    Nz, n = 10, 6
    d = case_device(Nz, "T_top+flux_bottom", "reference_zero")
    d.save_state()
    w = cotangents(Nz, COLUMNS, 73)
    g_ref = pull_back(d, [(DT, n)], w)                             # per-step ...
    assert d.adjoint_checkpoints() == (0, 0, n)
    d.restore_state()
    d.open_adjoint(2, checkpoint_every=4)                          # ... then checkpointed, with steps left on the tape it replaces ...
    assert d.adjoint_checkpoints() == (4, 0, 2) and d.adjoint_tape() == (0, 8)
    d.step_record(DT, 3)
    d.open_adjoint(n)                                              # ... and per-step again
    assert d.adjoint_checkpoints() == (0, 0, n) and d.adjoint_tape() == (0, n)
    assert np.array_equal(bits(pull_back_checkpointed(d, [(DT, n)], w, 4)), bits(g_ref))
    assert np.array_equal(bits(pull_back(d, [(DT, n)], w)), bits(g_ref))
    assert not d.last_program()["checkpointed"]
    d.close_adjoint()
    assert code_of(d.adjoint_checkpoints) == CAPI.TRM_EINVAL


# ---- 6. at size ---------------------------------------------------------------------------------------------------------------------
def test_checkpointed_gradient_at_size():
    lat, lon = W.columns_from_mask("N145")
    Nz, n, K = 32, 40, 16
    w = W.make_workload("heat", lat, lon, Nz)
    d = W.setup_device(w, steps_per_launch=0)
    d.closure()
    Nh = d.grid.Nh
    assert Nh == 56951
    d.save_state()
    cot = cotangents(Nz, Nh, 47)
    calls = [(w["dt"], n)]
    g_ref = pull_back(d, calls, cot)
    d.restore_state()
    d.open_adjoint(3, checkpoint_every=K)                          # 44 MB of tape against 584 MB
    d.step_record(w["dt"], n)
    assert d.adjoint_checkpoints() == (K, 3, 3)
    for name in TANGENTS:
        d.set_cotangent(name, cot[name])
    d.adjoint_backward()
    g = d.cotangent("internal_energy")
    assert d.last_program()["checkpointed"] and d.last_program()["lanes_per_column"] == 32
    assert np.all(np.isfinite(g_ref)) and np.any(g_ref != 0.0)
    assert np.array_equal(bits(g), bits(g_ref))


# ---- 7. Python ------------------------------------------------------------------------------------------------------------------------
def test_vjp_with_checkpoints_equals_vjp():
    def build():
        grid = trm.ColumnGrid(trm.ExponentialSpacing(N=20), num_columns=3)
        model = trm.SoilModel(grid, initializer=trm.SoilInitializer(energy=trm.QuasiThermalSteadyState(T0=-1.0)))
        bcs = trm.merge_boundary_conditions(trm.PrescribedSurfaceTemperature("T_ub", 1.0))
        return trm.initialize(model, trm.ForwardEuler(), boundary_conditions=bcs)
    a, b, c = build(), build(), build()
    g_ref = trm.vjp(a, 40, temperature=1.0)
    g = trm.vjp(b, 40, temperature=1.0, checkpoint_every=16)
    trm.run(c, steps=40)
    assert np.any(g_ref != 0.0) and np.array_equal(bits(g), bits(g_ref))
    for name in STATE:
        assert np.array_equal(bits(b.state.get(name)), bits(c.state.get(name))), name
    assert b.state.clock() == c.state.clock()
    # an adjoint the caller has opened is reused or replaced, and stays open
    b.state.open_adjoint(5)
    a.state.open_adjoint(5)
    g_ref = trm.vjp(a, 7, temperature=1.0)
    g = trm.vjp(b, 7, temperature=1.0, checkpoint_every=4)
    assert a.state.adjoint_checkpoints() == (0, 0, 7) and b.state.adjoint_checkpoints() == (4, 0, 2)
    assert np.array_equal(bits(g), bits(g_ref))


def test_example_gradient_with_checkpoints_equals_the_examples_gradient():
    ex = load_example()
    g_ref = ex.gradient(200)
    g = ex.gradient(200, checkpoint_every=16)
    assert g.shape == g_ref.shape and np.any(g_ref != 0.0)
    assert np.array_equal(bits(g), bits(g_ref))
