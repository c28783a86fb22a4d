"""Derivatives of the heat-only run through boundary time series (TRM_OPT_DERIVATIVE_SERIES): trm_step_tangent, trm_step_record and
trm_adjoint_backward evaluate the series in the launch; seeds and gradients have the series' shape, [nt][Nh]
(trm_tangent_bc_series_upload, trm_adjoint_bc_series_download), trm.jvp(d_boundary=...) and trm.vjp(wrt_boundary=True).

What holds exactly is checked exactly: the primal is trm_step's with the same series bit for bit, a one-node series is the constant
run, scaling by two scales bit for bit, zero cotangents and untouched nodes give exact zeros, and the node gradients do not depend on
how the tape is cut into launches, record calls or segments.  The node gradients are then checked as the transpose of the seeded
series tangent (extended-precision contraction of its one-node runs) and both against central differences of the oracle.

The transpose tolerance is 8 x err_tan, err_tan measured when the module runs (the fixture `series_yardstick`) on the seeded series
tangent alone: one launch sequence with dense seeds on every node of both series against the extended-precision contraction of the
one-node runs.  Nothing of the adjoint enters the bound.  Each test prints the figures it measures before it asserts."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import terrarium_jl_amd as trm
import boundary_derivatives as B
import series_derivatives as S
from boundary_derivatives import HALOS, LD
from series_derivatives import NH, NT, SIZES, SPL, STEPS
from test_gpu_adjoint import cotangents, normalised_error
from test_gpu_boundary_gradient import yardstick as boundary_yardstick      # (the bound of the jvp-against-vjp identity)  # noqa: F401
from test_gpu_tangent import CAPI, DT, ROOT, STATE, TANGENTS, assert_close_by_column, bits, boundary_sets, code_of, device, mixed_state, params

pytestmark = pytest.mark.gpu

PRIMAL_SETS = S.SETS + ("zero_gradient_bottom+T_top",)


def series_pairs(bcs):
    """the pairs of a boundary set that may carry a series: Value on temperature, Flux on internal energy"""
    return [pair for pair in B.active_pairs(bcs) if bcs[pair][0] in ("value", "flux")]


def series_device(Nz, bcset, halo, indexing, nt=NT, steps_per_launch=SPL, Nh=NH, seed=7, pairs=None):
    """(device with the option on and the state saved, boundary set, {pair: series})"""
    p = params(halo)
    U, sat = mixed_state(Nz, Nh, p, seed=seed)
    bcs = boundary_sets(Nh)[bcset]
    d = device(Nz, Nh, p, U, sat, bcs, steps_per_launch=steps_per_launch)
    series = S.series_on(bcs, series_pairs(bcs) if pairs is None else pairs, indexing, Nh, nt)
    S.attach(d, series)
    d.set_option("derivative_series", 1)
    d.save_state()
    return d, bcs, series


def seeded(d, calls, dU, seeds):
    """{X: tangent of X} of the saved state under dU and the node seeds {pair: [nt][Nh]} (a fresh open_tangent zeroes every other seed)"""
    d.restore_state()
    d.open_tangent()
    d.set_tangent("internal_energy", dU)
    for pair, s in seeds.items():
        d.set_bc_series_tangent(*pair, s)
    for dt, n in calls:
        d.step_tangent(dt, n)
    assert d.last_program()["boundary_seeds"]
    return {x: d.tangent(x) for x in TANGENTS}


def sweep(d, calls, w, series, checkpoint_every=None):
    """(dL/dU_0, {pair: node gradients [nt][Nh]}) of the saved state: restores it, records `calls` on a fresh tape, pulls `w` back"""
    d.restore_state()
    steps = sum(n for _, n in calls)
    if checkpoint_every is None:
        d.open_adjoint(max(1, steps))
    else:
        d.open_adjoint(max(1, steps), checkpoint_every)
    for dt, n in calls:
        d.step_record(dt, n)
    for name in TANGENTS:
        d.set_cotangent(name, w.get(name, 0.0))
    d.adjoint_backward()
    assert d.last_program()["boundary_gradient"] and d.get_option("info_derivative_series") == len(series)
    return d.cotangent("internal_energy"), {pair: d.bc_series_gradient(*pair) for pair in series}


def last_error(d):
    return d._lib.trm_last_error(d._ctx).decode()


def boundary_values(d, pair):
    """the boundary value array of a pair whose series has been cleared: what the last evaluated step left there"""
    import torch
    return torch.as_tensor(d.bc_device_array(*pair), device=f"cuda:{int(d.grid.device)}").cpu().numpy()


def assert_same(a, b, what):
    assert np.array_equal(bits(a[0]), bits(b[0])), (what, "dL/dU_0")
    for pair in a[1]:
        assert np.array_equal(bits(a[1][pair]), bits(b[1][pair])), (what, pair)


# ---- 1. the primal is trm_step's with the same series ------------------------------------------------------------------------------------
@pytest.mark.parametrize("indexing", S.INDEXINGS)
@pytest.mark.parametrize("halo", HALOS)
@pytest.mark.parametrize("bcset", PRIMAL_SETS)
@pytest.mark.parametrize("Nz", SIZES)
def test_primal_is_trm_step_with_the_series_bit_for_bit(Nz, bcset, halo, indexing):
    a, bcs, series = series_device(Nz, bcset, halo, indexing)
    b, _, _ = series_device(Nz, bcset, halo, indexing, steps_per_launch=0)
    b.set_option("derivative_series", 0)                         # (trm_step does not read it)
    b.step(DT, STEPS, finalize=True)
    want = {name: bits(b.get(name)) for name in STATE}

    def same_state(what):
        for name in STATE:
            assert np.array_equal(bits(a.get(name)), want[name]), (what, name)
        assert a.status() == b.status() and a.clock() == b.clock(), what
        assert a.get_option("info_derivative_series") == len(series) == a.last_program()["series"], what

    a.open_tangent()
    a.set_tangent("internal_energy", np.random.default_rng(1).normal(0.0, 1e3, (Nz, NH)))
    a.step_tangent(DT, STEPS)
    same_state("step_tangent")
    assert a.last_program()["family"] == "column_tangent" and a.last_program()["lanes_per_column"] == (32 if Nz <= 32 else 64)
    for name in TANGENTS:
        assert np.all(np.isfinite(a.tangent(name))), name
    a.close_tangent()
    for K in (None, 4):
        a.restore_state()
        if K is None:
            a.open_adjoint(STEPS)
        else:
            a.open_adjoint(STEPS, K)
        a.step_record(DT, STEPS)
        same_state(("step_record", K))
        prog = a.last_program()
        assert prog["family"] == "column_adjoint" and not prog["backward"] and prog["checkpointed"] == (K is not None)
    # the option off: today's refusal
    a.set_option("derivative_series", 0)
    assert code_of(a.step_record, DT, 1) == CAPI.TRM_EUNSUPPORTED
    # the boundary value arrays hold what the last step evaluated, as after trm_step
    a.clear_series()
    b.clear_series()
    for pair in series:
        assert np.array_equal(bits(boundary_values(a, pair)), bits(boundary_values(b, pair))), pair


# ---- 2. a series of one node is the constant run -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("halo", HALOS)
@pytest.mark.parametrize("bcset", S.SETS)
@pytest.mark.parametrize("Nz", SIZES)
def test_one_node_series_is_the_constant_run(Nz, bcset, halo):
    a, bcs, series = series_device(Nz, bcset, halo, "linear", nt=1)
    assert len(series) == 2
    p = params(halo)
    U, sat = mixed_state(Nz, NH, p, seed=7)
    const = dict(bcs)
    for pair, (kind, _, values, _) in series.items():
        const[pair] = (kind, values[0].copy())
    b = device(Nz, NH, p, U, sat, const, steps_per_launch=SPL)
    b.save_state()
    rng = np.random.default_rng(5)
    dU = rng.normal(0.0, 1e3, (Nz, NH))
    seeds = {pair: rng.normal(0.0, 1.0, NH) for pair in series}
    ta = seeded(a, [(DT, STEPS)], dU, {pair: s[None, :] for pair, s in seeds.items()})
    b.open_tangent()
    b.set_tangent("internal_energy", dU)
    for pair, s in seeds.items():
        b.set_bc_tangent(*pair, s)
    b.step_tangent(DT, STEPS)
    for x in TANGENTS:
        assert np.array_equal(bits(ta[x]), bits(b.tangent(x))), x
    for name in STATE:
        assert np.array_equal(bits(a.get(name)), bits(b.get(name))), name
    w = cotangents(Nz, NH, 37)
    for K in (None, 4):
        g, gn = sweep(a, [(DT, STEPS)], w, series, checkpoint_every=K)
        b.restore_state()
        if K is None:
            b.open_adjoint(STEPS)
        else:
            b.open_adjoint(STEPS, K)
        b.open_bc_gradient()
        b.step_record(DT, STEPS)
        for name in TANGENTS:
            b.set_cotangent(name, w[name])
        b.adjoint_backward()
        assert np.array_equal(bits(g), bits(b.cotangent("internal_energy"))), K
        for pair in series:
            assert gn[pair].shape == (1, NH) and np.any(gn[pair] != 0.0)
            assert np.array_equal(bits(gn[pair][0]), bits(b.bc_gradient(*pair))), (K, pair)


# ---- 3. linearity ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("indexing", S.INDEXINGS)
@pytest.mark.parametrize("bcset", S.SETS)
@pytest.mark.parametrize("Nz", SIZES)
def test_scaling_and_zeros_are_exact(Nz, bcset, indexing):
    halo = HALOS[(Nz + len(indexing)) % 2]
    d, bcs, series = series_device(Nz, bcset, halo, indexing)
    calls = [(DT, STEPS)]
    rng = np.random.default_rng(11)
    dU = rng.normal(0.0, 1e3, (Nz, NH))
    seeds = {pair: rng.normal(0.0, 1.0, (NT, NH)) for pair in series}
    t1 = seeded(d, calls, dU, seeds)
    t2 = seeded(d, calls, 2.0 * dU, {pair: 2.0 * s for pair, s in seeds.items()})
    t0 = seeded(d, calls, 0.0, {pair: 0.0 * s for pair, s in seeds.items()})
    for x in TANGENTS:
        assert np.any(t1[x] != 0.0) and np.array_equal(bits(2.0 * t1[x]), bits(t2[x])), x
        assert np.all(t0[x] == 0.0), x
    # the series seeds alone reach the state
    ts = seeded(d, calls, 0.0, seeds)
    assert np.any(ts["internal_energy"] != 0.0)
    w = cotangents(Nz, NH, 37)
    g1 = sweep(d, calls, w, series)
    g2 = sweep(d, calls, {x: 2.0 * w[x] for x in w}, series)
    g0 = sweep(d, calls, {}, series)
    assert np.array_equal(bits(2.0 * g1[0]), bits(g2[0])) and np.all(g0[0] == 0.0)
    for pair in series:
        assert g1[1][pair].shape == (NT, NH) and np.any(g1[1][pair] != 0.0)
        assert np.array_equal(bits(2.0 * g1[1][pair]), bits(g2[1][pair])), pair
        assert np.all(g0[1][pair] == 0.0), pair
    # the per-column calls name the series calls for a seriesed pair
    for pair in series:
        assert code_of(d.bc_gradient, *pair) == CAPI.TRM_EINVAL


@pytest.mark.parametrize("bcset", S.SETS)
@pytest.mark.parametrize("Nz", SIZES)
def test_a_node_beyond_the_run_stays_zero(Nz, bcset):
    d, bcs, series = series_device(Nz, bcset, "reference_zero", "linear", nt=NT + 1)
    first = next(iter(series))
    assert series[first][1][NT - 1] > (STEPS - 1) * DT          # (no step's bracket reaches the fifth node of the first series)
    g, gn = sweep(d, [(DT, STEPS)], cotangents(Nz, NH, 37), series)
    assert np.all(gn[first][NT] == 0.0) and np.all(gn[first][:NT].any(axis=1))
    # ... and its seed reaches nothing
    seeds = np.zeros((NT + 1, NH))
    seeds[NT] = 1.0
    t = seeded(d, [(DT, STEPS)], 0.0, {first: seeds})
    for x in TANGENTS:
        assert np.all(t[x] == 0.0), x


# ---- 4. the node gradients do not depend on the partition -------------------------------------------------------------------------------
@pytest.mark.parametrize("indexing", S.INDEXINGS)
@pytest.mark.parametrize("halo", HALOS)
@pytest.mark.parametrize("bcset", S.SETS)
@pytest.mark.parametrize("Nz", SIZES)
def test_node_gradients_do_not_depend_on_the_partition(Nz, bcset, halo, indexing):
    d, bcs, series = series_device(Nz, bcset, halo, indexing, steps_per_launch=0)
    w = cotangents(Nz, NH, 37)
    ref = sweep(d, [(DT, STEPS)], w, series)
    d.set_option("steps_per_launch", 2)
    assert_same(ref, sweep(d, [(DT, STEPS)], w, series), "steps_per_launch 2")
    d.set_option("steps_per_launch", SPL)
    assert_same(ref, sweep(d, [(DT, STEPS)], w, series), "steps_per_launch 3")
    assert_same(ref, sweep(d, [(DT, 5), (DT, 3)], w, series), "record 5 + 3")
    for K in (1, 4, 16):
        assert_same(ref, sweep(d, [(DT, STEPS)], w, series, checkpoint_every=K), ("checkpointed", K))
        assert d.last_program()["checkpointed"]
    assert_same(ref, sweep(d, [(DT, 5), (DT, 3)], w, series, checkpoint_every=4), "checkpointed 4, record 5 + 3")


# ---- 5. the transpose of the seeded series tangent -------------------------------------------------------------------------------------
TRANSPOSE_SERIES_CASES = [(Nz, bcset, halo, S.INDEXINGS[(n + m + k) % 4]) for n, Nz in enumerate(SIZES) for m, bcset in enumerate(S.SETS)
                          for k, halo in enumerate(HALOS)]


def node_jacobians(d, series, calls):
    """Jb[pair][node][X][i, column] = dX_n[i] / d(node value): dU = 0 and a seed of 1 on that node in every column"""
    Jb = {}
    for pair in series:
        Jb[pair] = []
        for node in range(NT):
            s = np.zeros((NT, NH))
            s[node] = 1.0
            Jb[pair].append(seeded(d, calls, 0.0, {pair: s}))
    return Jb


def series_tangent_error(d, series, Jb, calls, seed):
    """err_tan: dense seeds on every node of every series against the extended-precision contraction of the one-node runs"""
    rng = np.random.default_rng(seed)
    seeds = {pair: rng.normal(0.0, 1.0, (NT, NH)) for pair in series}
    t = seeded(d, calls, 0.0, seeds)
    err = 0.0
    for x in TANGENTS:
        ref = sum(Jb[pair][node][x].astype(LD) * seeds[pair][node].astype(LD)[None, :] for pair in series for node in range(NT))
        Ssum = sum(np.abs(Jb[pair][node][x]).astype(LD) * np.abs(seeds[pair][node]).astype(LD)[None, :] for pair in series for node in range(NT))
        err = max(err, normalised_error(t[x], ref, Ssum, ("seeded series tangent", x)))
    return err


@pytest.fixture(scope="module")
def series_yardstick():
    """(tolerance, {case: err_tan}, {case: (device, series, node Jacobians)}): 8 x the largest err_tan over TRANSPOSE_SERIES_CASES"""
    err, kept = {}, {}
    calls = [(DT, STEPS)]
    for case in TRANSPOSE_SERIES_CASES:
        Nz, bcset, halo, indexing = case
        d, bcs, series = series_device(Nz, bcset, halo, indexing, seed=29)
        assert len(series) == 2
        Jb = node_jacobians(d, series, calls)
        err[case] = series_tangent_error(d, series, Jb, calls, seed=31)
        kept[case] = (d, series, Jb)
        print(f"series yardstick Nz={Nz} {bcset} {halo} {indexing}: err_tan = {err[case]:.3e}")
    tol = 8.0 * max(err.values())
    print(f"series yardstick: largest err_tan = {max(err.values()):.3e}, transpose tolerance = {tol:.3e}")
    assert 0.0 < tol <= 8.0 * 1e-12 and max(err.values()) <= 1e-12
    return tol, err, kept


@pytest.mark.parametrize("Nz,bcset,halo,indexing", TRANSPOSE_SERIES_CASES)
def test_node_gradient_is_the_transpose_of_the_seeded_series_tangent(Nz, bcset, halo, indexing, series_yardstick):
    tol, err_tan, kept = series_yardstick
    d, series, Jb = kept[(Nz, bcset, halo, indexing)]
    w = cotangents(Nz, NH, 37)
    _, gn = sweep(d, [(DT, STEPS)], w, series)
    errs = {}
    for pair in series:
        for node in range(NT):
            g_ref = sum(np.sum(Jb[pair][node][x].astype(LD) * w[x].astype(LD), axis=0) for x in TANGENTS)
            Ssum = sum(np.sum(np.abs(Jb[pair][node][x]).astype(LD) * np.abs(w[x]).astype(LD), axis=0) for x in TANGENTS)
            errs[(pair, node)] = normalised_error(gn[pair][node], g_ref, Ssum, ("node gradient", pair, node))
    print(f"transpose Nz={Nz} {bcset} {halo} {indexing}: err_tan = {err_tan[(Nz, bcset, halo, indexing)]:.3e}, "
          f"largest err_adj = {max(errs.values()):.3e}, tolerance = {tol:.3e}")
    assert max(errs.values()) <= tol


# ---- 6. central differences of the oracle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bcset,pair,indexing,halo", S.fd_cases())
def test_series_derivatives_match_central_differences_of_the_oracle(bcset, pair, indexing, halo):
    p, U0, sat, bcs, w = S.fd_inputs(bcset, halo)
    series = S.series_on(bcs, [pair], indexing, B.FD_NH)
    keep = S.fd_kept_columns(p, U0, sat, bcs, series)
    print(f"{bcset} {pair} {indexing} {halo}: kept share {keep.mean():.4f}")
    assert keep.mean() >= S.FD_KEEP_SHARE
    grid = trm.ColumnGrid(trm.PrescribedSpacing(dz=B.FD_DZ), B.FD_NH)
    d = trm.DeviceState(grid, p)
    d.set_option("steps_per_launch", SPL)
    d.set("saturation_water_ice", sat)
    d.set("internal_energy", U0)
    for (var, side), (kind, value) in bcs.items():
        d.set_bc(var, side, kind, value)
    S.attach(d, series)
    d.set_option("derivative_series", 1)
    d.closure()
    d.save_state()
    calls = [(DT, STEPS)]
    _, gn = sweep(d, calls, w, series)
    other = [q for q in B.active_pairs(bcs) if q != pair]
    assert len(other) == 1 and np.any(d.bc_gradient(*other[0]) != 0.0)      # (the pair without a series keeps its per-column gradient)
    h = B.FD_H[bcs[pair][0]]
    for node in range(NT):
        plus, minus, fd, Ssum = S.fd_central(p, U0, sat, bcs, series, pair, node, w, h)
        floor = 1e-9 * np.max(Ssum[keep])
        err = np.abs(fd - gn[pair][node].astype(LD))[keep]
        print(f"    node {node}: h = {h:g}, max err / S = {float(np.max(err / Ssum[keep])):.3e}")
        s = np.zeros((NT, B.FD_NH))
        s[node] = 1.0
        t = seeded(d, calls, 0.0, {pair: s})
        for x in TANGENTS:
            scale = np.max(np.abs(t[x][:, keep]), axis=0)
            fdx = (plus[x] - minus[x]) / (2.0 * h)
            bound = 1e-6 * scale[None, :] + 1e-9 * np.max(scale)           # (assert_close_by_column's)
            print(f"        tangent of {x}: max err / (1e-6 column scale + floor) = {float(np.max(np.abs(fdx[:, keep] - t[x][:, keep]) / bound)):.3e}")
        assert np.all(err <= 1e-6 * Ssum[keep] + floor), (pair, node)
        for x in TANGENTS:
            assert_close_by_column(plus[x], minus[x], h, t[x], keep, 1e-6, (x, pair, node))


# ---- 7. refusals and errors ------------------------------------------------------------------------------------------------------------------
def test_refusals_and_errors():
    I, E, U, St = CAPI.TRM_OK, CAPI.TRM_EINVAL, CAPI.TRM_EUNSUPPORTED, CAPI.TRM_ESTALE
    Nz, Nh = 10, 16
    p = params()
    Ustate, sat = mixed_state(Nz, Nh, p)
    T, En, top, bot = CAPI.BC_VAR["temperature"], CAPI.BC_VAR["internal_energy"], CAPI.SIDE["top"], CAPI.SIDE["bottom"]
    times, ones = [0.0, 1e6], np.ones((2, Nh))

    def fresh(bcset="T_top+flux_bottom", option=1):
        d = device(Nz, Nh, p, Ustate, sat, boundary_sets(Nh)[bcset])
        d.set_option("derivative_series", option)
        return d

    def refused(d, why):
        d.open_tangent()
        d.set_tangent("internal_energy", 1.0)
        d.open_adjoint(4)
        for fn, args in ((d.step_tangent, (DT, 1)), (d.step_record, (DT, 1)), (d.adjoint_backward, ())):
            assert code_of(fn, *args) == U, (why, fn.__name__)
            assert why in last_error(d), (why, last_error(d))

    # the option off: today's refusal, whatever the series
    d = fresh(option=0)
    assert d.get_option("derivative_series") == 0
    d.set_bc_series("temperature", "top", "value", times, ones)
    refused(d, "no time series may be attached")
    # a series of kind Gradient (off the branch-free kinds: the generic halos answer first), on the generic kinds, an input series
    d = fresh()
    d.set_bc_series("temperature", "top", "gradient", times, ones)
    refused(d, "generic boundary kinds")
    d = fresh("gradient_top+flux_bottom")
    d.set_bc_series("internal_energy", "bottom", "flux", times, ones)
    refused(d, "generic boundary kinds")
    d = fresh()
    d.set_bc_series("internal_energy", "top", "gradient", times, ones)
    refused(d, "not of kind Gradient")
    d = fresh()
    d.set_forcing_series("air_temperature", times, ones)
    refused(d, "input (forcing)")
    # windowed, trimmed
    d = fresh()
    d.set_bc_series("temperature", "top", "value", times, ones)
    d.series_window(("temperature", "top"), 4)
    refused(d, "windowed or trimmed")
    d = fresh()
    d.set_bc_series("temperature", "top", "value", times, ones)
    d.series_append(("temperature", "top"), [2e6, 3e6], ones)
    refused(d, "windowed or trimmed")
    # parameter seeds / an open parameter gradient together with a series
    d = fresh()
    d.set_bc_series("temperature", "top", "value", times, ones)
    d.open_tangent()
    assert code_of(d.set_param_tangent, {"k_mineral": 1.0}) == U and "time series" in last_error(d)
    d.open_adjoint(4)
    assert code_of(d.open_param_gradient) == U and "time series" in last_error(d)
    d = fresh()
    d.open_tangent()
    d.set_tangent("internal_energy", 1.0)
    d.set_param_tangent({"k_mineral": 1.0})
    d.open_adjoint(4)
    d.open_param_gradient()
    d.set_bc_series("temperature", "top", "value", times, ones)
    for fn, args in ((d.step_tangent, (DT, 1)), (d.step_record, (DT, 1)), (d.adjoint_backward, ())):
        assert code_of(fn, *args) == U and "time series" in last_error(d), fn.__name__
    # everything else derivative_unsupported refuses stays refused
    d = fresh()
    d.set_bc_series("temperature", "top", "value", times, ones)
    d.open_tangent()
    d.set_tangent("internal_energy", 1.0)
    h = d.open_average("temperature")
    assert code_of(d.step_tangent, DT, 1) == U
    d.close_average(h)
    assert code_of(d.step_tangent, DT, 1) == I and d.get_option("info_derivative_series") == 1

    # TRM_EINVAL of the three new calls
    d = fresh()
    L, ctx = d._lib, d._ctx
    buf = np.zeros((2, Nh))
    dev, nt = ctypes.c_void_p(), ctypes.c_int32()
    d.set_bc_series("temperature", "top", "value", times, ones)
    assert L.trm_tangent_bc_series_upload(ctx, T, top, 2, buf.ctypes.data) == E and "no tangent is open" in last_error(d)
    assert L.trm_adjoint_bc_series_download(ctx, T, top, 2, buf.ctypes.data) == E and "no adjoint is open" in last_error(d)
    assert L.trm_adjoint_bc_series_device_ptr(ctx, T, top, ctypes.byref(dev), ctypes.byref(nt)) == E
    d.open_tangent()
    d.open_adjoint(4)
    assert L.trm_tangent_bc_series_upload(ctx, T, top, 2, buf.ctypes.data) == I
    assert L.trm_tangent_bc_series_upload(ctx, En, bot, 2, buf.ctypes.data) == E and "no time series" in last_error(d)     # a pair without
    assert L.trm_tangent_bc_series_upload(ctx, T, top, 3, buf.ctypes.data) == E and "levels" in last_error(d)               # a wrong nt
    assert L.trm_tangent_bc_series_upload(ctx, T, top, 2, None) == E
    assert L.trm_tangent_bc_series_upload(ctx, CAPI.BC_VAR["pressure_head"], top, 2, buf.ctypes.data) == E
    assert L.trm_adjoint_bc_series_download(ctx, T, top, 2, buf.ctypes.data) == I and np.all(buf == 0.0)                       # zeros before a sweep
    assert L.trm_adjoint_bc_series_download(ctx, En, bot, 2, buf.ctypes.data) == E and "no time series" in last_error(d)
    assert L.trm_adjoint_bc_series_download(ctx, T, top, 1, buf.ctypes.data) == E and "levels" in last_error(d)
    assert L.trm_adjoint_bc_series_download(ctx, T, top, 2, None) == E
    assert L.trm_adjoint_bc_series_device_ptr(ctx, T, top, ctypes.byref(dev), ctypes.byref(nt)) == I and dev.value and nt.value == 2
    assert L.trm_adjoint_bc_series_device_ptr(ctx, T, top, None, ctypes.byref(nt)) == E
    assert L.trm_adjoint_bc_series_device_ptr(ctx, T, top, ctypes.byref(dev), None) == E
    assert L.trm_adjoint_bc_series_device_ptr(ctx, En, bot, ctypes.byref(dev), ctypes.byref(nt)) == E
    # ... and of the three per-column calls on a seriesed pair: they name the series call
    col = np.zeros(Nh)
    d.open_bc_gradient()
    assert L.trm_tangent_bc_upload(ctx, T, top, col.ctypes.data) == E and "trm_tangent_bc_series_upload" in last_error(d)
    assert L.trm_adjoint_bc_download(ctx, T, top, col.ctypes.data) == E and "trm_adjoint_bc_series_download" in last_error(d)
    assert L.trm_adjoint_bc_device_ptr(ctx, T, top, ctypes.byref(dev)) == E and "trm_adjoint_bc_series_download" in last_error(d)
    assert L.trm_tangent_bc_upload(ctx, En, bot, col.ctypes.data) == I and L.trm_adjoint_bc_download(ctx, En, bot, col.ctypes.data) == I

    # a series replaced, cleared or appended over a tape that holds steps: stale
    for change in ("replace", "clear", "append", "window"):
        d = fresh()
        d.set_bc_series("temperature", "top", "value", times, ones)
        d.open_adjoint(4)
        assert code_of(d.step_record, DT, 2) == I
        if change == "replace":
            d.set_bc_series("temperature", "top", "value", times, 2.0 * ones)
        elif change == "clear":
            d.clear_series()
        elif change == "append":
            d.series_append(("temperature", "top"), [2e6], ones[:1])
        else:
            d.series_window(("temperature", "top"), 4)
        got = code_of(d.adjoint_backward)
        assert got == (St if change in ("replace", "clear") else U), (change, got)     # (a windowed series is refused before the tape is looked at)
        d.clear_series()
        assert code_of(d.adjoint_backward) == St and code_of(d.step_record, DT, 1) == St, change
        d.open_adjoint(4)
        assert code_of(d.step_record, DT, 1) == I, change


# ---- 8. the Python layer -------------------------------------------------------------------------------------------------------------------
def build_series_integrator(Nh=5, nt=5, steps=11):
    grid = trm.ColumnGrid(trm.ExponentialSpacing(N=20), num_columns=Nh)
    model = trm.SoilModel(grid, initializer=trm.SoilInitializer(energy=trm.QuasiThermalSteadyState(T0=-1.0)))
    dt = trm.ForwardEuler().dt
    times = np.linspace(0.0, (steps - 1) * dt * 1.05, nt)
    values = 1.0 + 2.0 * np.sin(1.3 * np.arange(nt)[:, None] + 0.1 * np.arange(Nh)[None, :])
    bcs = trm.merge_boundary_conditions(trm.PrescribedSurfaceTemperature("T_ub", trm.FieldTimeSeries(times, values)))
    bcs[("internal_energy", "bottom")] = ("flux", 0.05)
    return trm.initialize(model, trm.ForwardEuler(), boundary_conditions=bcs)


@pytest.mark.parametrize("checkpoint_every", [None, 4])
def test_vjp_and_jvp_through_a_field_time_series(checkpoint_every, boundary_yardstick):
    tol = boundary_yardstick[0]
    Nz, Nh, nt, n = 20, 5, 5, 11
    w = cotangents(Nz, Nh, 61)
    a = build_series_integrator(Nh, nt, n)
    assert a.state.get_option("derivative_series") == 0
    g, gb = trm.vjp(a, n, checkpoint_every=checkpoint_every, wrt_boundary=True, **w)
    assert a.state.get_option("derivative_series") == 0                       # restored
    assert set(gb) == {("temperature", "top"), ("internal_energy", "bottom")}
    gs, gf = gb[("temperature", "top")], gb[("internal_energy", "bottom")]
    assert gs.shape == (nt, Nh) and gf.shape == (Nh,) and np.any(gf != 0.0) and np.all(np.any(gs != 0.0, axis=1))
    plain = trm.vjp(build_series_integrator(Nh, nt, n), n, checkpoint_every=checkpoint_every, **w)
    assert isinstance(plain, np.ndarray) and np.array_equal(bits(plain), bits(g))
    # <g, s> = <w, J s>, one node at a time; seeds of +-2^k scale the tangent of a seed of one exactly
    rng = np.random.default_rng(67)
    for node in range(nt):
        seed = np.zeros((nt, Nh))
        seed[node] = np.ldexp(rng.choice([-1.0, 1.0], Nh), rng.integers(-3, 4, Nh))
        b = build_series_integrator(Nh, nt, n)
        tan = trm.jvp(b, 0.0, n, d_boundary={("temperature", "top"): seed})
        assert b.state.get_option("derivative_series") == 0
        lhs = sum(np.sum(w[x].astype(LD) * tan[x].astype(LD), axis=0) for x in TANGENTS)
        Ssum = sum(np.sum(np.abs(w[x]).astype(LD) * np.abs(tan[x]).astype(LD), axis=0) for x in TANGENTS)
        err = normalised_error(gs[node] * seed[node], lhs, Ssum, ("jvp against vjp", node))
        print(f"jvp against vjp node {node} checkpoint_every={checkpoint_every}: err = {err:.3e}, tolerance = {tol:.3e}")
        assert err <= tol
    # an exception inside the call restores the option too
    c = build_series_integrator(Nh, nt, n)
    with pytest.raises(trm.TerrariumHipError):
        trm.jvp(c, 0.0, n, d_boundary={("temperature", "top"): np.zeros((nt + 1, Nh))})
    assert c.state.get_option("derivative_series") == 0


def test_the_example_runs(boundary_yardstick):
    tol = boundary_yardstick[0]
    path = os.path.join(ROOT, "examples", "surface_temperature_history_sensitivity.py")
    spec = importlib.util.spec_from_file_location("surface_temperature_history_sensitivity", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    steps, nodes = 12, 4
    g, times = ex.reverse(steps, nodes, checkpoint_every=4)
    assert g.shape == (nodes,) and times.shape == (nodes,) and np.all(np.isfinite(g)) and np.all(g != 0.0)
    for node in range(nodes):
        f = ex.forward(node, steps, nodes)
        print(f"example node {node}: vjp {g[node]:.6e}, jvp {f:.6e}, |difference| / |jvp| = {abs(f - g[node]) / abs(f):.3e}, tolerance = {tol:.3e}")
        # (the weights and the responses of the levels to a surface node are of one sign: S = sum |w| |tangent| is |jvp| itself)
        assert abs(f - g[node]) <= tol * abs(f)
