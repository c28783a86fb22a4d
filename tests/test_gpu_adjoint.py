"""Reverse-mode gradients of the heat-only SoilModel run (trm_adjoint_*, trm_step_record, trm_adjoint_backward, trm.vjp).

The recorded primal is checked bit for bit against a twin context stepped by trm_step.  The gradient is checked for what holds exactly
(scaling, locality, the closure transpose of an empty tape), as the transpose of the linear map trm_step_tangent applies (column
Jacobians built from one-hot tangent seeds, contracted on the host in extended precision), against central differences of the
oracle's scalar loss, on the reference's own differentiability test and example, at the size of the N145 grid, and for every refusal
and staleness rule of the ABI.

The transpose tolerance is a reassociation error, measured against the tangent program itself when the module runs (the fixture
`yardstick`): err_tan is the largest normalised difference between one trm_step_tangent launch with a dense seed v and the
extended-precision contraction J v of the one-hot Jacobian J of the same program, over the cases of
test_adjoint_is_the_transpose_of_the_tangent.  The adjoint sums the same products along the transposed tree and gets 8 x err_tan.
Nothing of the adjoint enters the bound.  Each test prints the figures it measures before it asserts."""
import ctypes

import numpy as np
import pytest

import workloads as W
import terrarium_jl_amd as trm
from test_gpu_tangent import (CAPI, DT, STATE, TANGENTS, bits, boundary_sets, code_of, device, latent, load_example, mixed_state,
                              oracle_state, params, regime_distance, small)

pytestmark = pytest.mark.gpu

LD = np.longdouble
TRANSPOSE_CASES = [(Nz, bcset, halo) for Nz in (10, 32, 50) for bcset in ("T_top+flux_bottom", "gradient_top+flux_bottom")
                   for halo in ("reference_zero", "mirror")]
TRANSPOSE_STEPS, TRANSPOSE_COLUMNS = 6, 48


def cotangents(Nz, Nh, seed):
    """dense random cotangents of (U, T, liq), scaled so that each field's share of the gradient is of order one (dT/dU ~ 1 / C,
    dliq/dU ~ 1 / L_theta)"""
    rng = np.random.default_rng(seed)
    return {"internal_energy": rng.normal(0.0, 1.0, (Nz, Nh)), "temperature": rng.normal(0.0, 3.0e6, (Nz, Nh)),
            "liquid_water_fraction": rng.normal(0.0, 1.0e8, (Nz, Nh))}


def pull_back(d, calls, w, capacity=None):
    """g = dL/dU_0 of the saved state: restores it, records `calls` = [(dt, nsteps), ...] on a fresh tape, pulls `w` back"""
    d.restore_state()
    d.open_adjoint(capacity or max(1, sum(n for _, n in calls)))
    for dt, n in calls:
        d.step_record(dt, n)
    for name in TANGENTS:
        d.set_cotangent(name, w.get(name, 0.0))
    d.adjoint_backward()
    return d.cotangent("internal_energy")


def jacobians(d, Nz, calls, cols=slice(None)):
    """{X: J_X[i, j, column]} = dX_n[i] / dU_0[j] of the saved state by one-hot trm_step_tangent seeds: round j seeds level j of every column"""
    J = None
    for j in range(Nz):
        e = np.zeros((Nz, d.grid.Nh))
        e[j] = 1.0
        d.restore_state()
        d.set_tangent("internal_energy", e)
        for dt, n in calls:
            d.step_tangent(dt, n)
        for name in TANGENTS:
            t = d.tangent(name)[:, cols]
            if J is None:
                J = {x: np.zeros((Nz, Nz, t.shape[1])) for x in TANGENTS}
            J[name][:, j, :] = t
    return J


def transpose_reference(J, w):
    """(g_ref, S): g_ref[j] = sum_X sum_i J_X[i, j] w_X[i] in extended precision, S the same sum of absolute values"""
    g = sum(np.einsum("ijc,ic->jc", J[x].astype(LD), w[x].astype(LD)) for x in TANGENTS)
    S = sum(np.einsum("ijc,ic->jc", np.abs(J[x]).astype(LD), np.abs(w[x]).astype(LD)) for x in TANGENTS)
    return g, S


def normalised_error(dev, ref, S, what):
    """max |dev - ref| / S; where S is zero every product is, and the device's value must be zero too"""
    zero = S == 0
    assert np.all(dev[zero] == 0.0), what
    if zero.all():
        return 0.0
    return float(np.max(np.abs(dev.astype(LD) - ref)[~zero] / S[~zero]))


def tangent_error(d, J, Nz, calls, cols, seed):
    """err_tan: one dense trm_step_tangent against the extended-precision contraction of the one-hot Jacobian"""
    v = np.random.default_rng(seed).normal(0.0, 1e3, (Nz, d.grid.Nh))
    d.restore_state()
    d.set_tangent("internal_energy", v)
    for dt, n in calls:
        d.step_tangent(dt, n)
    vc = v[:, cols]
    err = 0.0
    for x in TANGENTS:
        ref = np.einsum("ijc,jc->ic", J[x].astype(LD), vc.astype(LD))
        S = np.einsum("ijc,jc->ic", np.abs(J[x]).astype(LD), np.abs(vc).astype(LD))
        err = max(err, normalised_error(d.tangent(x)[:, cols], ref, S, ("tangent", x)))
    return err


def transpose_case(Nz, bcset, halo):
    """the device of a transpose case, its initial state saved and a tangent open"""
    p = params(halo)
    U, sat = mixed_state(Nz, TRANSPOSE_COLUMNS, p, seed=29)
    d = device(Nz, TRANSPOSE_COLUMNS, p, U, sat, boundary_sets(TRANSPOSE_COLUMNS)[bcset])
    d.save_state()
    d.open_tangent()
    return d


@pytest.fixture(scope="module")
def yardstick():
    """(tolerance of the transpose checks, {case: err_tan}): 8 x the largest err_tan over TRANSPOSE_CASES -- what evaluating this linear
    map in another order costs in fp64 on this device, measured on the tangent program alone"""
    err = {}
    for Nz, bcset, halo in TRANSPOSE_CASES:
        d = transpose_case(Nz, bcset, halo)
        calls = [(DT, TRANSPOSE_STEPS)]
        err[(Nz, bcset, halo)] = tangent_error(d, jacobians(d, Nz, calls), Nz, calls, slice(None), seed=31)
        print(f"yardstick Nz={Nz} {bcset} {halo}: err_tan = {err[(Nz, bcset, halo)]:.3e}")
    tol = 8.0 * max(err.values())
    print(f"yardstick: largest err_tan = {max(err.values()):.3e}, transpose tolerance = {tol:.3e}")
    # (above the additivity tolerance of test_tangent_is_exactly_linear the measurement itself would be wrong)
    assert 0.0 < tol <= 1e-12
    return tol, err


# ---- 1. the recorded primal: bit for bit what trm_step computes ------------------------------------------------------------------
@pytest.mark.parametrize("halo", ["reference_zero", "mirror"])
@pytest.mark.parametrize("bcset", list(boundary_sets(2)))
@pytest.mark.parametrize("Nz", [10, 32, 50])
def test_recorded_primal_is_trm_step_bit_for_bit(Nz, bcset, halo):
    Nh, n = 301, 7
    p = params(halo)
    U, sat = mixed_state(Nz, Nh, p)
    bcs = boundary_sets(Nh)[bcset]
    a = device(Nz, Nh, p, U, sat, bcs, steps_per_launch=3)      # 7 steps: launches of 3, 3 and 1
    b = device(Nz, Nh, p, U, sat, bcs)                          # the library's own choice of program
    a.open_adjoint(9)
    a.step_record(DT, n)
    b.step(DT, n, finalize=True)
    for name in STATE:
        assert np.array_equal(bits(a.get(name)), bits(b.get(name))), name
    assert a.status() == b.status() and a.clock() == b.clock()
    assert a.adjoint_tape() == (n, 9)
    prog = a.last_program()
    assert prog["family"] == "column_adjoint" and prog["lanes_per_column"] == (32 if Nz <= 32 else 64) and not prog["backward"]
    assert prog["generic_boundaries"] == bool(b.get_option("info_generic_boundary_kernels"))
    for name, w in cotangents(Nz, Nh, 2).items():
        a.set_cotangent(name, w)
    a.adjoint_backward()
    prog = a.last_program()
    assert prog["family"] == "column_adjoint" and prog["lanes_per_column"] == (32 if Nz <= 32 else 64) and prog["backward"]
    assert prog["generic_boundaries"] == bool(b.get_option("info_generic_boundary_kernels"))
    assert a.adjoint_tape() == (0, 9)
    assert np.all(np.isfinite(a.cotangent("internal_energy")))
    for name in STATE:                                          # the sweep leaves the state alone
        assert np.array_equal(bits(a.get(name)), bits(b.get(name))), name


# ---- 2. what holds exactly ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bcset", ["T_top+flux_bottom", "gradient_bottom+T_top"])
@pytest.mark.parametrize("Nz", [32, 50])
def test_doubling_the_cotangents_doubles_the_gradient_bit_for_bit(Nz, bcset):
    Nh, n = 301, 5
    p = params()
    U, sat = mixed_state(Nz, Nh, p, seed=11)
    d = device(Nz, Nh, p, U, sat, boundary_sets(Nh)[bcset], steps_per_launch=2)
    d.save_state()
    w = cotangents(Nz, Nh, 5)
    g1 = pull_back(d, [(DT, n)], w)
    g2 = pull_back(d, [(DT, n)], {name: 2.0 * x for name, x in w.items()})
    assert np.any(g1 != 0.0)
    assert np.array_equal(bits(g2), bits(2.0 * g1))


@pytest.mark.parametrize("halo", ["reference_zero", "mirror"])
@pytest.mark.parametrize("Nz", [10, 32, 50])
def test_gradient_is_local(Nz, halo):
    Nh, n = 66, 3
    p = params(halo)
    U, sat = mixed_state(Nz, Nh, p, seed=13)
    d = device(Nz, Nh, p, U, sat, boundary_sets(Nh)["flux_top+T_bottom"])
    d.save_state()
    dense = cotangents(Nz, Nh, 17)
    for i in (0, Nz // 2, Nz - 1):
        w = {name: np.zeros((Nz, Nh)) for name in TANGENTS}
        for name in TANGENTS:
            w[name][i] = dense[name][i]
        g = pull_back(d, [(DT, n)], w)
        far = np.abs(np.arange(Nz) - i) > n
        assert np.all(g[far] == 0.0), i
        assert np.all(g[i] != 0.0), i


def test_empty_tape_is_the_transpose_of_the_closure():
    Nz, Nh = 12, 96
    p = params()
    U, sat = mixed_state(Nz, Nh, p, seed=19)
    d = device(Nz, Nh, p, U, sat, {})
    d.open_tangent()
    d.set_tangent("internal_energy", 1.0)
    d.tangent_closure()
    a, b = d.tangent("temperature"), d.tangent("liquid_water_fraction")
    assert np.any(a != 0.0) and np.any(b != 0.0) and np.any(a == 0.0) and np.any(b == 0.0)
    # positive cotangents and slopes: no cancellation, so the result carries the relative rounding of one multiply-add chain per cell
    rng = np.random.default_rng(23)
    w = {"internal_energy": rng.uniform(0.5, 1.5, (Nz, Nh)), "temperature": rng.uniform(0.5e6, 1.5e6, (Nz, Nh)),
         "liquid_water_fraction": rng.uniform(0.5e8, 1.5e8, (Nz, Nh))}
    assert np.all(a >= 0.0) and np.all(b >= 0.0)
    d.open_adjoint(1)
    for name in TANGENTS:
        d.set_cotangent(name, w[name])
    d.adjoint_backward()
    assert d.adjoint_tape() == (0, 1)
    g = d.cotangent("internal_energy")
    np.testing.assert_allclose(g, w["internal_energy"] + a * w["temperature"] + b * w["liquid_water_fraction"], rtol=1e-14)
    assert np.all(d.cotangent("temperature") == 0.0) and np.all(d.cotangent("liquid_water_fraction") == 0.0)    # folded in
    assert d.last_program()["family"] == "column_adjoint" and d.last_program()["backward"]


# ---- 3. the transpose of the tangent program ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nz,bcset,halo", TRANSPOSE_CASES)
def test_adjoint_is_the_transpose_of_the_tangent(Nz, bcset, halo, yardstick):
    tol, err_tan = yardstick
    d = transpose_case(Nz, bcset, halo)
    assert bool(d.get_option("info_generic_boundary_kernels")) == bcset.startswith("gradient")
    calls = [(DT, TRANSPOSE_STEPS)]
    J = jacobians(d, Nz, calls)
    w = cotangents(Nz, TRANSPOSE_COLUMNS, 37)
    g = pull_back(d, calls, w)
    g_ref, S = transpose_reference(J, w)
    err_adj = normalised_error(g, g_ref, S, "adjoint")
    print(f"transpose Nz={Nz} {bcset} {halo}: err_tan = {err_tan[(Nz, bcset, halo)]:.3e}, err_adj = {err_adj:.3e}, tolerance = {tol:.3e}")
    assert err_adj <= tol


# ---- 4. central differences of the oracle's scalar loss ---------------------------------------------------------------------------
@pytest.mark.parametrize("bcset", ["T_top+flux_bottom", "gradient_top+flux_bottom"])
def test_gradient_matches_central_differences_of_the_oracle(bcset):
    Nz, Nh, n, h = 10, 64, 6, 100.0
    p = params()
    U0, sat = mixed_state(Nz, Nh, p, seed=3)
    L = latent(p, sat)
    bcs = boundary_sets(Nh)[bcset]
    o = oracle_state(Nz, Nh, p, U0, sat, bcs)
    dist = regime_distance(o.get("internal_energy"), L)
    for _ in range(n):
        o.timestep(DT)
        dist = np.minimum(dist, regime_distance(o.get("internal_energy"), L))
    keep = dist > 1e3 * h
    assert keep.mean() >= 0.8
    kept = U0[:, keep]
    Lk = L[:, keep]
    assert (kept >= 0).any() and ((kept < 0) & (kept >= -Lk)).any() and (kept < -Lk).any()   # all three regimes

    w = cotangents(Nz, Nh, 41)
    v = np.random.default_rng(43).uniform(-1.0, 1.0, (Nz, Nh))

    def loss(U):
        """per column: sum_k (wU U_n + wT T_n + wliq liq_n)[k, i] of the oracle's run from U"""
        q = oracle_state(Nz, Nh, p, U, sat, bcs)
        for _ in range(n):
            q.timestep(DT)
        return sum(np.sum(w[name].astype(LD) * q.get(name).astype(LD), axis=0) for name in TANGENTS)

    fd = (loss(U0 + h * v) - loss(U0 - h * v)) / (2.0 * h)
    d = device(Nz, Nh, p, U0, sat, bcs)
    d.save_state()
    g = pull_back(d, [(DT, n)], w)
    gv = np.sum(g.astype(LD) * v.astype(LD), axis=0)
    scale = np.sum(np.abs(g) * np.abs(v), axis=0)
    floor = 1e-9 * np.max(scale[keep])
    err = np.abs(fd - gv)[keep]
    print(f"central differences {bcset}: kept {keep.mean():.4f}, max err / scale = {float(np.max(err / scale[keep])):.3e}")
    assert np.all(err <= 1e-6 * scale[keep] + floor)


# ---- 5. the reference's test and example -------------------------------------------------------------------------------------------
def test_reference_differentiability_test_mean_temperature_step():
    """soil_energy_diff.jl:68-76: d mean(T_1) / dU_0 of one timestep! is finite"""
    grid = trm.ColumnGrid(trm.ExponentialSpacing(N=10), num_columns=1)
    model = trm.SoilModel(grid, initializer=trm.SoilInitializer())
    integ = trm.initialize(model, trm.ForwardEuler())
    g = trm.vjp(integ, 1, temperature=1.0 / 10)
    assert g.shape == (10, 1)
    assert np.all(np.isfinite(g)) and np.any(g != 0.0)


def test_example_gradient_is_row_one_of_the_jacobian(yardstick):
    tol, _ = yardstick
    ex = load_example()
    J_T, J_U, zs = ex.jacobian(3)
    g = ex.gradient(3)
    Nz = J_T.shape[0]
    assert g.shape == (Nz,)
    err = np.abs(g - J_T[1])
    print(f"example: max |gradient - J_T[1]| / |J_T[1]| = {float(np.max(err[J_T[1] != 0] / np.abs(J_T[1])[J_T[1] != 0])):.3e}")
    assert np.all(err <= tol * np.abs(J_T[1]))
    assert np.all(g[np.abs(np.arange(Nz) - 1) > 3] == 0.0) and np.any(g != 0.0)
    g = ex.gradient()
    assert g.shape == (50,) and np.all(np.isfinite(g)) and np.any(g != 0.0)


def test_vjp_leaves_the_integrator_where_run_leaves_it():
    def build():
        grid = trm.ColumnGrid(trm.ExponentialSpacing(N=20), num_columns=3)
        model = trm.SoilModel(grid, initializer=trm.SoilInitializer(energy=trm.QuasiThermalSteadyState(T0=-1.0)))
        bcs = trm.merge_boundary_conditions(trm.PrescribedSurfaceTemperature("T_ub", 1.0))
        return trm.initialize(model, trm.ForwardEuler(), boundary_conditions=bcs)
    a, b = build(), build()
    g = trm.vjp(a, 20, temperature=1.0)
    trm.run(b, steps=20)
    assert g.shape == (20, 3) and np.all(np.isfinite(g)) and np.any(g != 0.0)
    for name in STATE:
        assert np.array_equal(bits(a.state.get(name)), bits(b.state.get(name))), name
    assert a.state.clock() == b.state.clock()
    with pytest.raises(ValueError):
        trm.vjp(trm.initialize(build().model, trm.Heun()), 1, temperature=1.0)


# ---- 6. at size ---------------------------------------------------------------------------------------------------------------------
def test_adjoint_is_the_transpose_of_the_tangent_at_size(yardstick):
    tol, _ = yardstick
    lat, lon = W.columns_from_mask("N145")
    Nz, n = 32, 10
    w = W.make_workload("heat", lat, lon, Nz)
    d = W.setup_device(w, steps_per_launch=0)
    d.closure()
    Nh = d.grid.Nh
    assert Nh % 2 == 1                                         # two columns per wave: the last wave is a tail
    d.save_state()
    d.open_tangent()
    cols = slice(None, None, 25)
    calls = [(w["dt"], n)]
    J = jacobians(d, Nz, calls, cols)
    d.close_tangent()
    cot = cotangents(Nz, Nh, 47)
    g = pull_back(d, calls, cot)
    assert d.last_program()["family"] == "column_adjoint" and d.last_program()["lanes_per_column"] == 32
    assert np.all(np.isfinite(g))
    g_ref, S = transpose_reference(J, {name: x[:, cols] for name, x in cot.items()})
    err_adj = normalised_error(g[:, cols], g_ref, S, "adjoint at size")
    print(f"transpose at size: {g_ref.shape[1]} of {Nh} columns, err_adj = {err_adj:.3e}, tolerance = {tol:.3e}")
    assert err_adj <= tol


# ---- 7. refusals and staleness -----------------------------------------------------------------------------------------------------
def test_refusals():
    U, E, M, I = CAPI.TRM_EUNSUPPORTED, CAPI.TRM_EINVAL, CAPI.TRM_ENOMEM, CAPI.TRM_OK
    assert code_of(small(dtype=np.float32).open_adjoint, 4) == U
    rich = params()
    rich.flow = CAPI.FLOW["richards"]
    assert code_of(small(p=rich).open_adjoint, 4) == U
    land = params()
    land.flow, land.seb = CAPI.FLOW["richards"], 1
    assert code_of(small(p=land).open_adjoint, 4) == U
    veg = small()
    veg.set_vegetation(CAPI.default_vegetation_params(), "standalone")
    assert code_of(veg.open_adjoint, 4) == U
    assert code_of(small(Nz=80).open_adjoint, 4) == U
    # no adjoint open
    d = small()
    assert code_of(d.step_record, DT, 1) == E
    assert code_of(d.adjoint_backward) == E
    assert code_of(d.set_cotangent, "internal_energy", 1.0) == E
    assert code_of(d.cotangent, "internal_energy") == E
    assert code_of(d.adjoint_tape) == E
    assert code_of(d.close_adjoint) == E
    # bad arguments
    assert code_of(d.open_adjoint, 0) == E
    assert code_of(d.open_adjoint, -3) == E
    assert code_of(d.open_adjoint, 2**31 - 1) == M                # 2 TiB of tape
    assert code_of(d.adjoint_tape) == E
    d.open_adjoint(4)
    assert d.adjoint_tape() == (0, 4)
    assert code_of(d.step_record, DT, -1) == E
    buf = (ctypes.c_double * (8 * 16))()
    dev, pitch = ctypes.c_void_p(), ctypes.c_int64()
    for which in (-1, 3):
        assert d._lib.trm_adjoint_upload(d._ctx, which, buf) == E
        assert d._lib.trm_adjoint_download(d._ctx, which, buf) == E
        assert d._lib.trm_adjoint_device_ptr(d._ctx, which, ctypes.byref(dev), ctypes.byref(pitch)) == E
    assert d._lib.trm_adjoint_upload(d._ctx, 0, None) == E
    assert d._lib.trm_adjoint_device_ptr(d._ctx, 0, ctypes.byref(dev), ctypes.byref(pitch)) == I and dev.value and pitch.value >= 8
    # refusals of the record and the sweep: an attached series, an open time average
    assert code_of(d.step_record, DT, 1) == I
    assert d.last_program()["family"] == "column_adjoint" and not d.last_program()["backward"]
    h = d.open_average("temperature")
    assert code_of(d.step_record, DT, 1) == U
    assert code_of(d.adjoint_backward) == U
    d.close_average(h)
    assert code_of(d.step_record, DT, 1) == I
    assert d.adjoint_tape() == (2, 4)
    assert code_of(d.adjoint_backward) == I
    assert d.adjoint_tape() == (0, 4)
    d.close_adjoint()
    assert code_of(d.cotangent, "internal_energy") == E


def test_recording_past_the_capacity_is_refused_and_changes_nothing():
    E, I = CAPI.TRM_EINVAL, CAPI.TRM_OK
    d = small()
    d.open_adjoint(5)
    d.step_record(DT, 3)
    before = {name: d.get(name) for name in STATE}
    clock, status = d.clock(), d.status()
    assert code_of(d.step_record, DT, 3) == E
    assert d.adjoint_tape() == (3, 5)
    for name in STATE:
        assert np.array_equal(bits(d.get(name)), bits(before[name])), name
    assert d.clock() == clock and d.status() == status
    assert code_of(d.step_record, DT, 2) == I
    assert d.adjoint_tape() == (5, 5)
    assert code_of(d.step_record, DT, 1) == E
    assert code_of(d.step_record, DT, 0) == I
    assert code_of(d.adjoint_backward) == I
    assert d.adjoint_tape() == (0, 5)


@pytest.mark.parametrize("change", ["step", "step_heun", "upload_internal_energy", "restore_state", "reset", "set_bc", "step_tangent"])
def test_state_changes_make_the_tape_stale(change):
    S, I = CAPI.TRM_ESTALE, CAPI.TRM_OK
    d = small()
    d.save_state()
    d.open_tangent()
    d.open_adjoint(8)
    d.step_record(DT, 2)
    d.set_tangent("internal_energy", 1.0)                          # (seeds the tangent the record has made stale)
    {"step": lambda: d.step(DT, 1), "step_heun": lambda: d.step_heun(DT, 1), "restore_state": d.restore_state, "reset": d.reset,
     "upload_internal_energy": lambda: d.set("internal_energy", d.get("internal_energy")),
     "set_bc": lambda: d.set_bc("temperature", "top", "value", 2.0), "step_tangent": lambda: d.step_tangent(DT, 1)}[change]()
    clock = d.clock()
    assert code_of(d.adjoint_backward) == S
    assert code_of(d.step_record, DT, 1) == S
    assert d.adjoint_tape() == (2, 8) and d.clock() == clock
    d.open_adjoint(8)                                              # a fresh tape
    assert d.adjoint_tape() == (0, 8)
    assert code_of(d.step_record, DT, 1) == I
    assert code_of(d.adjoint_backward) == I


def test_changes_before_the_first_taped_step_do_not_make_the_tape_stale():
    I = CAPI.TRM_OK
    d = small()
    d.open_adjoint(4)
    d.step(DT, 1)
    d.set_bc("temperature", "top", "value", 2.0)
    assert code_of(d.step_record, DT, 2) == I
    assert code_of(d.adjoint_backward) == I
    d.step(DT, 1)                                                  # the sweep has emptied the tape
    assert code_of(d.step_record, DT, 1) == I
    assert code_of(d.adjoint_backward) == I


def test_step_record_makes_an_open_tangent_stale():
    S, I = CAPI.TRM_ESTALE, CAPI.TRM_OK
    d = small()
    d.open_tangent()
    d.open_adjoint(4)
    d.set_tangent("internal_energy", 1.0)
    d.step_tangent(DT, 1)
    assert code_of(d.tangent, "temperature") == I
    d.step_record(DT, 1)
    assert code_of(d.tangent, "temperature") == S
    assert code_of(d.step_tangent, DT, 1) == S
    d.set_tangent("internal_energy", 1.0)
    assert code_of(d.tangent, "temperature") == I


@pytest.mark.parametrize("bcset", ["T_top+flux_bottom", "gradient_top+flux_bottom"])
def test_each_taped_step_is_pulled_back_with_its_own_dt(bcset, yardstick):
    tol, _ = yardstick
    Nz, Nh = 32, 48
    p = params()
    U, sat = mixed_state(Nz, Nh, p, seed=53)
    d = device(Nz, Nh, p, U, sat, boundary_sets(Nh)[bcset], steps_per_launch=3)
    d.save_state()
    d.open_tangent()
    calls = [(DT, 4), (0.5 * DT, 3)]                               # backward: launches of 3 (dt / 2), then 3 and 1 (dt)
    J = jacobians(d, Nz, calls)
    w = cotangents(Nz, Nh, 59)
    g = pull_back(d, calls, w)
    g_ref, S = transpose_reference(J, w)
    err_adj = normalised_error(g, g_ref, S, "adjoint")
    # the same steps with one dt are another map: the check tells them apart
    J_one = jacobians(d, Nz, [(DT, 7)])
    g_one, S_one = transpose_reference(J_one, w)
    print(f"two dt {bcset}: err_adj = {err_adj:.3e}, tolerance = {tol:.3e}, "
          f"against one dt = {normalised_error(g, g_one, S_one, 'adjoint, one dt'):.3e}")
    assert err_adj <= tol
    assert normalised_error(g, g_one, S_one, "adjoint, one dt") > 1e-3
