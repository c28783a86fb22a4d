"""Derivatives with respect to boundary values of the heat-only run: seeds on trm_step_tangent (trm_tangent_bc_upload), gradients from
trm_adjoint_backward (trm_adjoint_bc_*), trm.jvp(d_boundary=...) and trm.vjp(wrt_boundary=True).

What holds exactly is checked exactly: the primal and g = dL/dU_0 are bit for bit what they are without, zero seeds change nothing,
scaling by two scales bit for bit, a pair whose kind reads no value gives exact zeros, the reach of a cotangent, and the independence
of the boundary gradients of how the tape is cut into launches and segments.  The gradients are then checked as the transpose of the
seeded tangent program (extended-precision contraction of its one-hot Jacobians) and both against central differences of the oracle.

The transpose tolerance is 8 x err_tan, err_tan measured when the module runs (the fixture `yardstick`) on the seeded tangent program
alone: one launch with a dense dU and dense seeds on every active pair against the extended-precision contraction of that program's
one-hot Jacobians, boundary columns included, over TRANSPOSE_BC_CASES.  Nothing of the adjoint enters the bound.  Each test prints
the figures it measures before it asserts."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import workloads as W
import terrarium_jl_amd as trm
import boundary_derivatives as B
from boundary_derivatives import HALOS, LD, PAIRS, active_pairs
from test_gpu_adjoint import TRANSPOSE_CASES, TRANSPOSE_COLUMNS, TRANSPOSE_STEPS, cotangents, normalised_error
from test_gpu_tangent import (CAPI, DT, ROOT, STATE, TANGENTS, assert_close_by_column, bits, boundary_sets, code_of, device, mixed_state, params,
                              small)

pytestmark = pytest.mark.gpu

SETS = list(boundary_sets(2))
SIZES = (10, 32, 50)        # fewer than 32 lanes a column, exactly 32, the 64-lane layout
NH = 301                    # an odd tail: half of the last wave of the 32-lane layout is clamped
# the cases of test_gpu_adjoint.py, a Flux on top, a Gradient at the bottom (generic halos), and the zero Gradient the primal skips
TRANSPOSE_BC_CASES = TRANSPOSE_CASES + [(32, "flux_top+T_bottom", "reference_zero"), (50, "gradient_bottom+T_top", "mirror"),
                                        (10, "zero_gradient_bottom+T_top", "reference_zero")]


def record_and_sweep(d, calls, w, capacity=None, checkpoint_every=None, bc=True):
    """(g, {pair: boundary gradient}) of the saved state: restores it, records `calls` on a fresh tape, pulls `w` back"""
    d.restore_state()
    steps = sum(n for _, n in calls)
    if checkpoint_every is None:
        d.open_adjoint(capacity or max(1, steps))
    else:
        d.open_adjoint(capacity or max(1, steps), checkpoint_every)      # (a slot per step is enough for any interval and split)
    if bc:
        d.open_bc_gradient()
    for dt, n in calls:
        d.step_record(dt, n)
    for name in TANGENTS:
        d.set_cotangent(name, w.get(name, 0.0))
    d.adjoint_backward()
    return d.cotangent("internal_energy"), ({pair: d.bc_gradient(*pair) for pair in PAIRS} if bc else {})


def seeded_tangent(d, calls, dU, seeds):
    """{X: tangent of X} of the saved state under the seed dU and the boundary seeds {pair: values}; every other pair's seed is zero"""
    d.restore_state()
    d.set_tangent("internal_energy", dU)
    for pair in PAIRS:
        d.set_bc_tangent(*pair, seeds.get(pair, 0.0))
    for dt, n in calls:
        d.step_tangent(dt, n)
    assert d.last_program()["boundary_seeds"]
    return {x: d.tangent(x) for x in TANGENTS}


def case_device(Nz, bcset, halo, Nh=NH, seed=7, steps_per_launch=0):
    p = params(halo)
    U, sat = mixed_state(Nz, Nh, p, seed=seed)
    bcs = boundary_sets(Nh)[bcset]
    d = device(Nz, Nh, p, U, sat, bcs, steps_per_launch=steps_per_launch)
    d.save_state()
    return d, bcs


def assert_same_gradients(a, b, what):
    for pair in PAIRS:
        assert np.array_equal(bits(a[pair]), bits(b[pair])), (what, pair)


# ---- 1. the primal and the initial-state gradient are what they were ---------------------------------------------------------------
@pytest.mark.parametrize("halo", HALOS)
@pytest.mark.parametrize("bcset", SETS)
@pytest.mark.parametrize("Nz", SIZES)
def test_primal_and_initial_state_gradient_are_unchanged(Nz, bcset, halo):
    n = 7
    p = params(halo)
    U, sat = mixed_state(Nz, NH, p)
    bcs = boundary_sets(NH)[bcset]
    w = cotangents(Nz, NH, 2)
    a = device(Nz, NH, p, U, sat, bcs, steps_per_launch=3)      # 7 steps: launches of 3, 3 and 1
    b = device(Nz, NH, p, U, sat, bcs, steps_per_launch=3)      # the twin without boundary gradients
    c = device(Nz, NH, p, U, sat, bcs)                          # trm_step, the library's own choice of program
    for d in (a, b):
        d.open_adjoint(n)
    a.open_bc_gradient()
    for d in (a, b):
        d.step_record(DT, n)
    c.step(DT, n, finalize=True)
    for name in STATE:
        assert np.array_equal(bits(a.get(name)), bits(b.get(name))) and np.array_equal(bits(a.get(name)), bits(c.get(name))), name
    for d in (a, b):
        for name in TANGENTS:
            d.set_cotangent(name, w[name])
        d.adjoint_backward()
    pa, pb = a.last_program(), b.last_program()
    assert pa["family"] == "column_adjoint" and pa["backward"] and pa["boundary_gradient"] and not pb["boundary_gradient"]
    assert {k: v for k, v in pa.items() if k != "boundary_gradient"} == {k: v for k, v in pb.items() if k != "boundary_gradient"}
    assert np.array_equal(bits(a.cotangent("internal_energy")), bits(b.cotangent("internal_energy")))
    for pair in PAIRS:
        g = a.bc_gradient(*pair)
        assert np.all(np.isfinite(g)) and np.any(g != 0.0) == (pair in active_pairs(bcs)), pair
    # the tangent: the state under seeds is trm_step's, and zero seeds give the unseeded tangents
    dU = np.random.default_rng(1).normal(0.0, 1e3, (Nz, NH))
    t, u = device(Nz, NH, p, U, sat, bcs, steps_per_launch=3), device(Nz, NH, p, U, sat, bcs, steps_per_launch=3)
    for d in (t, u):
        d.open_tangent()
        d.set_tangent("internal_energy", dU)
    rng = np.random.default_rng(3)
    for pair in PAIRS:
        t.set_bc_tangent(*pair, rng.normal(0.0, 1.0, NH))
    t.step_tangent(DT, n)
    u.step_tangent(DT, n)
    pt, pu = t.last_program(), u.last_program()
    assert pt["family"] == "column_tangent" and pt["boundary_seeds"] and not pu["boundary_seeds"]
    assert {k: v for k, v in pt.items() if k != "boundary_seeds"} == {k: v for k, v in pu.items() if k != "boundary_seeds"}
    for name in STATE:
        assert np.array_equal(bits(t.get(name)), bits(c.get(name))), name
    assert t.status() == c.status() and t.clock() == c.clock()
    unseeded = {x: u.tangent(x) for x in TANGENTS}
    changed = any(not np.array_equal(t.tangent(x), unseeded[x]) for x in TANGENTS)
    assert changed == bool(active_pairs(bcs))                   # (the seeds of a pair that reads no value do nothing)
    z = device(Nz, NH, p, U, sat, bcs, steps_per_launch=3)
    z.open_tangent()
    z.set_tangent("internal_energy", dU)
    for pair in PAIRS:
        z.set_bc_tangent(*pair, 0.0)
    z.step_tangent(DT, n)
    assert z.last_program()["boundary_seeds"]
    for x in TANGENTS:
        assert np.array_equal(z.tangent(x), unseeded[x]), x


# ---- 2. what holds exactly ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("halo", HALOS)
@pytest.mark.parametrize("bcset", SETS)
@pytest.mark.parametrize("Nz", SIZES)
def test_scaling_and_zeros_are_exact(Nz, bcset, halo):
    n = 5
    d, bcs = case_device(Nz, bcset, halo, seed=11, steps_per_launch=2)
    calls = [(DT, n)]
    w = cotangents(Nz, NH, 5)
    _, g1 = record_and_sweep(d, calls, w)
    _, g2 = record_and_sweep(d, calls, {name: 2.0 * x for name, x in w.items()})
    _, g0 = record_and_sweep(d, calls, {})
    for pair in PAIRS:
        if pair in active_pairs(bcs):
            assert np.all(g1[pair] != 0.0), pair
        else:
            assert np.all(g1[pair] == 0.0), pair               # the pair's kind reads no value: exact zeros
        assert np.array_equal(bits(g2[pair]), bits(2.0 * g1[pair])), pair
        assert np.all(g0[pair] == 0.0), pair
    # doubling a seed doubles the tangents
    d.open_tangent()
    rng = np.random.default_rng(13)
    seeds = {pair: rng.normal(0.0, 1.0, NH) for pair in active_pairs(bcs)}
    t1 = seeded_tangent(d, calls, 0.0, seeds)
    t2 = seeded_tangent(d, calls, 0.0, {pair: 2.0 * s for pair, s in seeds.items()})
    for x in TANGENTS:
        assert np.array_equal(bits(t2[x]), bits(2.0 * t1[x])), x
    if seeds:
        assert np.any(t1["internal_energy"] != 0.0)


@pytest.mark.parametrize("halo", HALOS)
@pytest.mark.parametrize("bcset", SETS)
@pytest.mark.parametrize("Nz", SIZES)
def test_boundary_gradient_reaches_as_far_as_the_steps(Nz, bcset, halo):
    """a one-hot cotangent on level i and n steps: the top gradient is exactly 0 for Nz - 1 - i >= n, the bottom gradient for i >= n"""
    Nh, n = 66, 3
    d, bcs = case_device(Nz, bcset, halo, Nh=Nh, seed=13)
    dense = cotangents(Nz, Nh, 17)
    for i in (0, n - 1, n, Nz - 1 - n, Nz - n, Nz - 1):
        w = {name: np.zeros((Nz, Nh)) for name in TANGENTS}
        for name in TANGENTS:
            w[name][i] = dense[name][i]
        _, g = record_and_sweep(d, [(DT, n)], w)
        for var, side in PAIRS:
            if side == "top" and Nz - 1 - i >= n or side == "bottom" and i >= n:
                assert np.all(g[(var, side)] == 0.0), (i, var, side)
            if (var, side) in active_pairs(bcs) and (side == "top" and i == Nz - 1 or side == "bottom" and i == 0):
                assert np.all(g[(var, side)] != 0.0), (i, var, side)


# ---- 3. the sum does not depend on how the tape is cut ------------------------------------------------------------------------------
@pytest.mark.parametrize("halo", HALOS)
@pytest.mark.parametrize("bcset", SETS)
@pytest.mark.parametrize("Nz", SIZES)
def test_boundary_gradients_do_not_depend_on_the_partition(Nz, bcset, halo):
    d, bcs = case_device(Nz, bcset, halo, seed=19)
    w = cotangents(Nz, NH, 23)
    for calls in ([(DT, 4), (DT, 4), (DT, 3)], [(DT, 4), (0.5 * DT, 3)]):       # (K = 4: segments of 4 4 3; of 4 3)
        d.set_option("steps_per_launch", 0)
        g_ref, ref = record_and_sweep(d, calls, w)
        assert not d.last_program()["checkpointed"] and d.last_program()["boundary_gradient"]
        d.set_option("steps_per_launch", 2)
        g, got = record_and_sweep(d, calls, w)
        assert np.array_equal(bits(g), bits(g_ref))
        assert_same_gradients(got, ref, ("steps_per_launch 2", calls))
        d.set_option("steps_per_launch", 0)
        for K in (1, 4, 16):
            g, got = record_and_sweep(d, calls, w, checkpoint_every=K)
            assert d.last_program()["checkpointed"] and d.last_program()["boundary_gradient"]
            assert np.array_equal(bits(g), bits(g_ref))
            assert_same_gradients(got, ref, ("checkpointed", K, calls))
        for pair in active_pairs(bcs):
            assert np.any(ref[pair] != 0.0)


@pytest.mark.parametrize("Nz", SIZES)
def test_thirteen_columns_are_the_same_columns_in_a_wider_launch(Nz):
    """Nh = 13: a tail in both layouts.  The same 13 columns twice over in a launch of 26 give the same bits in both copies."""
    Nh, n = 13, 5
    p = params()
    U, sat = mixed_state(Nz, Nh, p, seed=43)
    bcs = boundary_sets(Nh)["gradient_bottom+T_top"]
    wide = {pair: (kind, np.tile(np.broadcast_to(np.asarray(value, dtype=np.float64), (Nh,)), 2)) for pair, (kind, value) in bcs.items()}
    w = cotangents(Nz, Nh, 71)
    seeds = {pair: np.random.default_rng(73).normal(0.0, 1.0, Nh) for pair in active_pairs(bcs)}
    a = device(Nz, Nh, p, U, sat, bcs)
    b = device(Nz, 2 * Nh, p, np.tile(U, (1, 2)), np.tile(sat, (1, 2)), wide)
    for d in (a, b):
        d.save_state()
        d.open_tangent()
    ga, gb = record_and_sweep(a, [(DT, n)], w)[1], record_and_sweep(b, [(DT, n)], {x: np.tile(v, (1, 2)) for x, v in w.items()})[1]
    gk = record_and_sweep(a, [(DT, n)], w, checkpoint_every=4)[1]
    ta = seeded_tangent(a, [(DT, n)], w["internal_energy"], seeds)
    tb = seeded_tangent(b, [(DT, n)], np.tile(w["internal_energy"], (1, 2)), {pair: np.tile(v, 2) for pair, v in seeds.items()})
    for pair in PAIRS:
        assert np.any(ga[pair] != 0.0) == (pair in active_pairs(bcs)), pair
        assert np.array_equal(bits(gb[pair][:Nh]), bits(ga[pair])) and np.array_equal(bits(gb[pair][Nh:]), bits(ga[pair])), pair
        assert np.array_equal(bits(gk[pair]), bits(ga[pair])), pair
    for x in TANGENTS:
        assert np.array_equal(bits(tb[x][:, :Nh]), bits(ta[x])) and np.array_equal(bits(tb[x][:, Nh:]), bits(ta[x])), x


# ---- 4. the transpose of the seeded tangent program ----------------------------------------------------------------------------------
def seeded_jacobians(d, Nz, calls, pairs, cols=slice(None), state=True):
    """(J, Jb) of the saved state by the seeded tangent program: J[X][i, j, column] = dX_n[i] / dU_0[j] from one-hot dU with zero seeds,
    Jb[pair][X][i, column] = dX_n[i] / d(value of pair) from dU = 0 and a seed of 1 on that pair in every column"""
    Nh = d.grid.Nh
    J = None
    if state:
        J = {x: np.zeros((Nz, Nz, len(range(Nh)[cols]))) for x in TANGENTS}
        for j in range(Nz):
            e = np.zeros((Nz, Nh))
            e[j] = 1.0
            t = seeded_tangent(d, calls, e, {})
            for x in TANGENTS:
                J[x][:, j, :] = t[x][:, cols]
    Jb = {}
    for pair in pairs:
        t = seeded_tangent(d, calls, 0.0, {pair: 1.0})
        Jb[pair] = {x: t[x][:, cols] for x in TANGENTS}
    return J, Jb


def seeded_tangent_error(d, J, Jb, Nz, calls, seed):
    """err_tan: one launch with a dense dU and dense seeds on every pair of Jb against the extended-precision contraction"""
    rng = np.random.default_rng(seed)
    Nh = d.grid.Nh
    v = rng.normal(0.0, 1e3, (Nz, Nh))
    seeds = {pair: rng.normal(0.0, 1.0, Nh) for pair in Jb}
    t = seeded_tangent(d, calls, v, seeds)
    err = 0.0
    for x in TANGENTS:
        ref = np.einsum("ijc,jc->ic", J[x].astype(LD), v.astype(LD))
        S = np.einsum("ijc,jc->ic", np.abs(J[x]).astype(LD), np.abs(v).astype(LD))
        for pair, s in seeds.items():
            ref = ref + Jb[pair][x].astype(LD) * s.astype(LD)[None, :]
            S = S + np.abs(Jb[pair][x]).astype(LD) * np.abs(s).astype(LD)[None, :]
        err = max(err, normalised_error(t[x], ref, S, ("seeded tangent", x)))
    return err


def boundary_reference(Jb_pair, w):
    """(g_ref, S)[column] = sum_X sum_i J_X,b[i] w_X[i] in extended precision, and the same sum of absolute values"""
    g = sum(np.sum(Jb_pair[x].astype(LD) * w[x].astype(LD), axis=0) for x in TANGENTS)
    S = sum(np.sum(np.abs(Jb_pair[x]).astype(LD) * np.abs(w[x]).astype(LD), axis=0) for x in TANGENTS)
    return g, S


@pytest.fixture(scope="module")
def yardstick():
    """(tolerance, {case: err_tan}, {case: (device, boundary Jacobians)}): 8 x the largest err_tan over TRANSPOSE_BC_CASES"""
    err, kept = {}, {}
    calls = [(DT, TRANSPOSE_STEPS)]
    for case in TRANSPOSE_BC_CASES:
        Nz, bcset, halo = case
        d, bcs = case_device(Nz, bcset, halo, Nh=TRANSPOSE_COLUMNS, seed=29)
        d.open_tangent()
        J, Jb = seeded_jacobians(d, Nz, calls, active_pairs(bcs))
        err[case] = seeded_tangent_error(d, J, Jb, Nz, calls, seed=31)
        kept[case] = (d, Jb)
        print(f"yardstick Nz={Nz} {bcset} {halo}: err_tan = {err[case]:.3e}")
    tol = 8.0 * max(err.values())
    print(f"yardstick: largest err_tan = {max(err.values()):.3e}, transpose tolerance = {tol:.3e}")
    # (above the additivity tolerance of test_tangent_is_exactly_linear the measurement itself would be wrong)
    assert 0.0 < tol <= 1e-12
    return tol, err, kept


@pytest.mark.parametrize("Nz,bcset,halo", TRANSPOSE_BC_CASES)
def test_boundary_gradient_is_the_transpose_of_the_seeded_tangent(Nz, bcset, halo, yardstick):
    tol, err_tan, kept = yardstick
    d, Jb = kept[(Nz, bcset, halo)]
    assert len(Jb) == 2
    w = cotangents(Nz, TRANSPOSE_COLUMNS, 37)
    _, g = record_and_sweep(d, [(DT, TRANSPOSE_STEPS)], w)
    errs = {}
    for pair in Jb:
        g_ref, S = boundary_reference(Jb[pair], w)
        assert np.all(S > 0)
        errs[pair] = normalised_error(g[pair], g_ref, S, ("boundary gradient", pair))
    print(f"transpose Nz={Nz} {bcset} {halo}: err_tan = {err_tan[(Nz, bcset, halo)]:.3e}, "
          + ", ".join(f"err_adj{pair} = {e:.3e}" for pair, e in errs.items()) + f", tolerance = {tol:.3e}")
    assert max(errs.values()) <= tol


# ---- 5. at size -------------------------------------------------------------------------------------------------------------------------
def test_boundary_gradient_is_the_transpose_at_size(yardstick):
    tol = yardstick[0]
    lat, lon = W.columns_from_mask("N145")
    Nz, n = 32, 10
    w = W.make_workload("heat", lat, lon, Nz)
    d = W.setup_device(w, steps_per_launch=0)
    d.closure()
    Nh = d.grid.Nh
    assert Nh % 2 == 1                                         # two columns per wave: the last wave is a tail
    d.save_state()
    d.open_tangent()
    calls = [(w["dt"], n)]
    pairs = active_pairs(w["bcs"])
    assert pairs == [("temperature", "top")]
    _, Jb = seeded_jacobians(d, Nz, calls, pairs, state=False)
    d.close_tangent()
    cot = cotangents(Nz, Nh, 47)
    _, g = record_and_sweep(d, calls, cot)
    prog = d.last_program()
    assert prog["family"] == "column_adjoint" and prog["lanes_per_column"] == 32 and prog["boundary_gradient"]
    for pair in pairs:
        g_ref, S = boundary_reference(Jb[pair], cot)
        err = normalised_error(g[pair], g_ref, S, ("boundary gradient at size", pair))
        print(f"transpose at size {pair}: {Nh} columns, err_adj = {err:.3e}, tolerance = {tol:.3e}")
        assert np.all(np.isfinite(g[pair])) and np.any(g[pair] != 0.0)
        assert err <= tol


# ---- 6. central differences of the oracle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("halo", HALOS)
@pytest.mark.parametrize("bcset", B.FD_SETS)
def test_boundary_derivatives_match_central_differences_of_the_oracle(bcset, halo):
    p, U0, sat, bcs, w = B.fd_inputs(bcset, halo)
    keep = B.fd_kept_columns(p, U0, sat, bcs)
    print(f"{bcset} {halo}: kept share {keep.mean():.4f}")
    assert keep.mean() >= B.FD_KEEP_SHARE
    grid = trm.ColumnGrid(trm.PrescribedSpacing(dz=B.FD_DZ), B.FD_NH)
    d = trm.DeviceState(grid, p)
    d.set("saturation_water_ice", sat)
    d.set("internal_energy", U0)
    for (var, side), (kind, value) in bcs.items():
        d.set_bc(var, side, kind, value)
    d.closure()
    d.save_state()
    calls = [(DT, B.FD_STEPS)]
    assert bool(d.get_option("info_generic_boundary_kernels")) == bcset.startswith("gradient")
    _, g = record_and_sweep(d, calls, w)
    d.open_tangent()
    for pair in active_pairs(bcs):
        h = B.FD_H[bcs[pair][0]]
        plus, minus, fd, S = B.fd_central(p, U0, sat, bcs, pair, w, h)
        floor = 1e-9 * np.max(S[keep])
        err = np.abs(fd - g[pair].astype(LD))[keep]
        print(f"central differences {bcset} {halo} {pair}: h = {h:g}, max err / S = {float(np.max(err / S[keep])):.3e}")
        t = seeded_tangent(d, calls, 0.0, {pair: 1.0})
        for x in TANGENTS:
            scale = np.max(np.abs(t[x][:, keep]), axis=0)
            fdx = (plus[x] - minus[x]) / (2.0 * h)
            bound = 1e-6 * scale[None, :] + 1e-9 * np.max(scale)           # (assert_close_by_column's)
            print(f"    tangent of {x}: max err / (1e-6 column scale + floor) = {float(np.max(np.abs(fdx[:, keep] - t[x][:, keep]) / bound)):.3e}")
        assert np.all(err <= 1e-6 * S[keep] + floor), pair
        for x in TANGENTS:
            assert_close_by_column(plus[x], minus[x], h, t[x], keep, 1e-6, (x, pair))


# ---- 7. the Python layer -------------------------------------------------------------------------------------------------------------------
def build_integrator(Nh=5):
    grid = trm.ColumnGrid(trm.ExponentialSpacing(N=20), num_columns=Nh)
    model = trm.SoilModel(grid, initializer=trm.SoilInitializer(energy=trm.QuasiThermalSteadyState(T0=-1.0)))
    bcs = trm.merge_boundary_conditions(trm.PrescribedSurfaceTemperature("T_ub", 1.0))
    bcs[("internal_energy", "bottom")] = ("flux", 0.05)
    return trm.initialize(model, trm.ForwardEuler(), boundary_conditions=bcs)


@pytest.mark.parametrize("checkpoint_every", [None, 4])
def test_vjp_with_respect_to_boundary_values(checkpoint_every, yardstick):
    tol = yardstick[0]
    Nz, Nh, n = 20, 5, 11
    w = cotangents(Nz, Nh, 61)
    a, b = build_integrator(Nh), build_integrator(Nh)
    g, gb = trm.vjp(a, n, checkpoint_every=checkpoint_every, wrt_boundary=True, **w)
    assert set(gb) == {("temperature", "top"), ("internal_energy", "bottom")}
    plain = trm.vjp(build_integrator(Nh), n, checkpoint_every=checkpoint_every, **w)
    assert isinstance(plain, np.ndarray) and np.array_equal(bits(plain), bits(g))
    st = b.state
    st.save_state()
    g2, gb2 = record_and_sweep(st, [(b.timestepper.dt, n)], w, checkpoint_every=checkpoint_every)
    assert np.array_equal(bits(g), bits(g2))
    for pair in gb:
        assert gb[pair].shape == (Nh,) and np.any(gb[pair] != 0.0)
        assert np.array_equal(bits(gb[pair]), bits(gb2[pair])), pair
    # <w, jvp(seed)> = <boundary gradient, seed>, one pair at a time; seeds of +-2^k scale the tangent of a seed of one exactly, so this
    # is the identity of the transpose check
    rng = np.random.default_rng(67)
    for pair in gb:
        seed = np.ldexp(rng.choice([-1.0, 1.0], Nh), rng.integers(-3, 4, Nh))
        tan = trm.jvp(build_integrator(Nh), 0.0, n, d_boundary={pair: seed})
        lhs = sum(np.sum(w[x].astype(LD) * tan[x].astype(LD), axis=0) for x in TANGENTS)
        S = sum(np.sum(np.abs(w[x]).astype(LD) * np.abs(tan[x]).astype(LD), axis=0) for x in TANGENTS)
        err = normalised_error(gb[pair] * seed, lhs, S, ("jvp against vjp", pair))
        print(f"jvp against vjp {pair} checkpoint_every={checkpoint_every}: err = {err:.3e}, tolerance = {tol:.3e}")
        assert err <= tol


def test_the_example_runs(yardstick):
    tol = yardstick[0]
    path = os.path.join(ROOT, "examples", "surface_temperature_sensitivity.py")
    spec = importlib.util.spec_from_file_location("surface_temperature_sensitivity", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    dT, zs = ex.forward(3)
    Nz = dT.shape[0]
    g = ex.reverse(3)
    assert g.shape == (Nz,) and zs.shape == (Nz,)
    err = np.abs(g - dT)
    print(f"example: max |vjp - jvp| / |jvp| = {float(np.max(err[dT != 0] / np.abs(dT)[dT != 0])):.3e}, tolerance = {tol:.3e}")
    assert np.all(err <= tol * np.abs(dT))
    assert np.all(dT[: Nz - 3] == 0.0) and np.any(dT != 0.0)                    # three steps reach three levels down
    levels = [0, 1, Nz // 2, Nz - 1]
    dT, _ = ex.forward()
    g = ex.reverse(levels=levels, checkpoint_every=16)
    print(f"example, {ex.N_T} steps: jvp {dT[levels]}, vjp {g}")
    assert dT.shape == (Nz,) and np.all(np.isfinite(dT)) and np.any(dT != 0.0)
    assert g.shape == (len(levels),) and np.all(np.isfinite(g)) and np.any(g != 0.0)


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    U, E, S, I = CAPI.TRM_EUNSUPPORTED, CAPI.TRM_EINVAL, CAPI.TRM_ESTALE, CAPI.TRM_OK
    T, top = CAPI.BC_VAR["temperature"], CAPI.SIDE["top"]
    d = small()
    buf = (ctypes.c_double * 16)()
    dev = ctypes.c_void_p()
    # nothing open
    assert code_of(d.set_bc_tangent, "temperature", "top", 1.0) == E
    assert code_of(d.open_bc_gradient) == E
    assert code_of(d.bc_gradient, "temperature", "top") == E
    assert d._lib.trm_adjoint_bc_device_ptr(d._ctx, T, top, ctypes.byref(dev)) == E
    d.open_tangent()
    d.open_adjoint(4)
    # before trm_adjoint_bc_open
    assert code_of(d.bc_gradient, "temperature", "top") == E
    assert d._lib.trm_adjoint_bc_device_ptr(d._ctx, T, top, ctypes.byref(dev)) == E
    assert code_of(d.open_bc_gradient) == I
    assert code_of(d.bc_gradient, "temperature", "top") == I
    assert d._lib.trm_adjoint_bc_device_ptr(d._ctx, T, top, ctypes.byref(dev)) == I and dev.value
    # bad pairs and pointers
    for var in ("saturation_water_ice", "liquid_water_fraction", "pressure_head"):
        assert d._lib.trm_tangent_bc_upload(d._ctx, CAPI.BC_VAR[var], top, buf) == E, var
        assert d._lib.trm_adjoint_bc_download(d._ctx, CAPI.BC_VAR[var], top, buf) == E, var
        assert d._lib.trm_adjoint_bc_device_ptr(d._ctx, CAPI.BC_VAR[var], top, ctypes.byref(dev)) == E, var
    for var in (-1, 5):
        assert d._lib.trm_tangent_bc_upload(d._ctx, var, top, buf) == E
        assert d._lib.trm_adjoint_bc_download(d._ctx, var, top, buf) == E
    for side in (2, -1):
        assert d._lib.trm_tangent_bc_upload(d._ctx, T, side, buf) == E
        assert d._lib.trm_adjoint_bc_download(d._ctx, T, side, buf) == E
        assert d._lib.trm_adjoint_bc_device_ptr(d._ctx, T, side, ctypes.byref(dev)) == E
    assert d._lib.trm_tangent_bc_upload(d._ctx, T, top, None) == E
    assert d._lib.trm_adjoint_bc_download(d._ctx, T, top, None) == E
    assert d._lib.trm_adjoint_bc_device_ptr(d._ctx, T, top, None) == E
    # the rules of the step and the sweep answer first: an attached series, a stale tape, a stale tangent
    d.set_tangent("internal_energy", 1.0)
    d.set_bc_tangent("temperature", "top", 1.0)
    assert code_of(d.step_tangent, DT, 1) == I and d.last_program()["boundary_seeds"]
    d.open_adjoint(4)                                              # (the tangent step is a state change for a tape)
    assert code_of(d.step_record, DT, 2) == I
    d.set_bc_series("temperature", "top", "value", [0.0, 1e6], np.ones((2, 16)))
    assert code_of(d.step_tangent, DT, 1) == U
    assert code_of(d.adjoint_backward) == U
    d.clear_series()
    assert code_of(d.adjoint_backward) == S                        # (the series was a change of a boundary condition)
    assert code_of(d.step_tangent, DT, 1) == S                     # (the record was a state change for the tangent)
    assert code_of(d.set_bc_tangent, "temperature", "top", 2.0) == I
    assert code_of(d.step_tangent, DT, 1) == S                     # (a seed upload does not seed dU)
    d.set_tangent("internal_energy", 1.0)
    assert code_of(d.step_tangent, DT, 1) == I
    d.open_adjoint(4)
    assert code_of(d.step_record, DT, 1) == I
    assert code_of(d.adjoint_backward) == I and d.last_program()["boundary_gradient"]
    assert np.all(d.bc_gradient("temperature", "top") == 0.0)      # (zero cotangents)
    # open_tangent zeroes the seeds and goes back to the unseeded instance; closing frees
    d.open_tangent()
    assert code_of(d.step_tangent, DT, 1) == I and not d.last_program()["boundary_seeds"]
    d.close_adjoint()
    assert code_of(d.bc_gradient, "temperature", "top") == E
    d.close_tangent()
    assert code_of(d.set_bc_tangent, "temperature", "top", 1.0) == E
    # fp32 and Richards: nothing to open
    assert code_of(small(dtype=np.float32).open_tangent) == U
    f = small(dtype=np.float32)
    assert code_of(f.set_bc_tangent, "temperature", "top", 1.0) == E and code_of(f.open_bc_gradient) == E
    rich = params()
    rich.flow = CAPI.FLOW["richards"]
    r = small(p=rich)
    assert code_of(r.open_adjoint, 4) == U and code_of(r.open_bc_gradient) == E
