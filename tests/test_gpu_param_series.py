"""Thermal-parameter seeds and gradients together with boundary time series (TRM_OPT_DERIVATIVE_SERIES_PARAMS): what holds exactly,
checked exactly, on Nz in (10, 32, 50) x 16 columns under all four time indexings.

Ten zero parameter seeds give the series ride's tangents; with the parameter gradient open dL/dU_0 and the node gradients are those of
the series-only sweep (the parameter sums do not feed lam); a one-node series gives the tangents and the ten parameter gradients of the
constant-boundary parameter ride; doubling seeds or cotangents doubles bit for bit; node and parameter gradients do not depend on how
the steps are cut into launches.  The ten parameter gradients are then checked as the transpose of ten one-hot parameter tangent
sweeps (extended-precision contraction with the cotangents) within 8 x err_tan, err_tan measured when the module runs on the tangent
program of the new ride alone (the fixture `yardstick`, the pattern of test_gpu_adjoint.py), refused above 1e-12 -- this covers the
raster indexing, which the exact Jacobian of test_gpu_param_series_edges.py does not.  Then the refusals, and trm.jvp / trm.vjp on an
integrator driven by a FieldTimeSeries."""
import importlib.util
import os

import numpy as np
import pytest

import series_derivatives as S
import terrarium_jl_amd as trm
from boundary_derivatives import HALOS, LD
from parameter_derivatives import PARAMS
from series_derivatives import NT, SIZES, STEPS
from test_gpu_adjoint import cotangents, normalised_error
from test_gpu_series_derivative import build_series_integrator, last_error, seeded, series_device
from test_gpu_series_derivative import sweep as series_sweep
from test_gpu_tangent import CAPI, DT, ROOT, TANGENTS, bits, boundary_sets, code_of, device, mixed_state, params

pytestmark = pytest.mark.gpu

NH = 16
CALLS = [(DT, STEPS)]
CASES = [(Nz, bcset, HALOS[(n + m + k) % 2], indexing) for n, Nz in enumerate(SIZES) for m, bcset in enumerate(S.SETS)
         for k, indexing in enumerate(S.INDEXINGS)]


def joint_device(Nz, bcset, halo, indexing, **kw):
    """(device with both options on and the state saved, boundary set, {pair: series}): both pairs of the set carry a series"""
    d, bcs, series = series_device(Nz, bcset, halo, indexing, Nh=NH, **kw)
    assert len(series) == 2
    d.set_option("derivative_series_params", 1)
    return d, bcs, series


def joint_tangent(d, dU, node_seeds, param_seeds, calls=CALLS):
    """{X: tangent} of the saved state under dU, {pair: [nt][Nh]} and {name: value}: always the ride with both"""
    d.restore_state()
    d.open_tangent()
    d.set_tangent("internal_energy", dU)
    for pair, s in node_seeds.items():
        d.set_bc_series_tangent(*pair, s)
    d.set_param_tangent(param_seeds)
    for dt, n in calls:
        d.step_tangent(dt, n)
    prog = d.last_program()
    assert prog["family"] == "column_tangent" and prog["boundary_seeds"] and prog["parameter_seeds"] and prog["series"] == 2
    return {x: d.tangent(x) for x in TANGENTS}


def joint_sweep(d, w, series, calls=CALLS, checkpoint_every=None):
    """(dL/dU_0, {pair: node gradients}, [10][Nh] parameter gradients) from one sweep with the parameter gradient open"""
    d.restore_state()
    steps = sum(n for _, n in calls)
    d.open_adjoint(max(1, steps), checkpoint_every)
    d.open_param_gradient()
    for dt, n in calls:
        d.step_record(dt, n)
    for name in TANGENTS:
        d.set_cotangent(name, w.get(name, 0.0))
    d.adjoint_backward()
    prog = d.last_program()
    assert prog["boundary_gradient"] and prog["parameter_gradient"] and prog["series"] == len(series)
    out = d.cotangent("internal_energy"), {pair: d.bc_series_gradient(*pair) for pair in series}, np.stack([d.param_gradient(name) for name in PARAMS])
    d.close_adjoint()                                                            # (a later series-only sweep starts without the accumulators)
    return out


def dense_seeds(series, seed):
    rng = np.random.default_rng(seed)
    return {pair: rng.normal(0.0, 1.0, (NT, NH)) for pair in series}


def dense_params(p, seed):
    rng = np.random.default_rng(seed)
    return {name: getattr(p, name) * rng.uniform(0.5, 1.5) * rng.choice([-1.0, 1.0]) for name in PARAMS}


# ---- 1. the two families leave each other alone ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nz,bcset,halo,indexing", CASES)
def test_zero_parameter_seeds_give_the_series_ride(Nz, bcset, halo, indexing):
    d, bcs, series = joint_device(Nz, bcset, halo, indexing)
    dU = np.random.default_rng(3).normal(0.0, 1e3, (Nz, NH))
    seeds = dense_seeds(series, 5)
    plain = seeded(d, CALLS, dU, seeds)
    assert not d.last_program()["parameter_seeds"]
    both = joint_tangent(d, dU, seeds, {name: 0.0 for name in PARAMS})
    for x in TANGENTS:
        assert np.any(plain[x] != 0.0) and np.array_equal(bits(both[x]), bits(plain[x])), x


@pytest.mark.parametrize("Nz,bcset,halo,indexing", CASES)
def test_initial_state_and_node_gradients_are_the_series_sweeps(Nz, bcset, halo, indexing):
    d, bcs, series = joint_device(Nz, bcset, halo, indexing)
    w = cotangents(Nz, NH, 37)
    for K in (None, 4):
        g, gn = series_sweep(d, CALLS, w, series, checkpoint_every=K)
        assert not d.last_program()["parameter_gradient"]
        d.close_adjoint()
        g2, gn2, gp = joint_sweep(d, w, series, checkpoint_every=K)
        assert np.array_equal(bits(g2), bits(g)), K
        for pair in series:
            assert np.any(gn[pair] != 0.0) and np.array_equal(bits(gn2[pair]), bits(gn[pair])), (K, pair)
        assert np.all(np.isfinite(gp)) and np.any(gp != 0.0)


# ---- 2. a series of one node is the constant-boundary parameter ride ---------------------------------------------------------------------
@pytest.mark.parametrize("halo", HALOS)
@pytest.mark.parametrize("bcset", S.SETS)
@pytest.mark.parametrize("Nz", SIZES)
def test_one_node_series_is_the_constant_parameter_ride(Nz, bcset, halo):
    a, bcs, series = joint_device(Nz, bcset, halo, "linear", nt=1)
    p = params(halo)
    U, sat = mixed_state(Nz, NH, p, seed=7)
    const = dict(bcs)
    for pair, (kind, _, values, _) in series.items():
        const[pair] = (kind, values[0].copy())
    b = device(Nz, NH, p, U, sat, const, steps_per_launch=S.SPL)
    b.save_state()
    rng = np.random.default_rng(5)
    dU = rng.normal(0.0, 1e3, (Nz, NH))
    seeds = {pair: rng.normal(0.0, 1.0, NH) for pair in series}
    ps = dense_params(p, 9)
    ta = joint_tangent(a, dU, {pair: s[None, :] for pair, s in seeds.items()}, ps)
    b.open_tangent()
    b.set_tangent("internal_energy", dU)
    for pair, s in seeds.items():
        b.set_bc_tangent(*pair, s)
    b.set_param_tangent(ps)
    b.step_tangent(DT, STEPS)
    assert b.last_program()["parameter_seeds"] and b.last_program()["series"] == 0
    for x in TANGENTS:
        assert np.array_equal(bits(ta[x]), bits(b.tangent(x))), x
    w = cotangents(Nz, NH, 37)
    for K in (None, 4):
        g, gn, gp = joint_sweep(a, w, series, checkpoint_every=K)
        b.restore_state()
        b.open_adjoint(STEPS, K)
        b.open_param_gradient()
        b.step_record(DT, STEPS)
        for name in TANGENTS:
            b.set_cotangent(name, w[name])
        b.adjoint_backward()
        assert np.array_equal(bits(g), bits(b.cotangent("internal_energy"))), K
        for pair in series:
            assert np.array_equal(bits(gn[pair][0]), bits(b.bc_gradient(*pair))), (K, pair)
        for q, name in enumerate(PARAMS):
            assert np.array_equal(bits(gp[q]), bits(b.param_gradient(name))), (K, name)
        assert np.any(gp != 0.0)


# ---- 3. linearity, the partition ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nz,bcset,halo,indexing", CASES)
def test_scaling_is_exact(Nz, bcset, halo, indexing):
    d, bcs, series = joint_device(Nz, bcset, halo, indexing)
    dU = np.random.default_rng(11).normal(0.0, 1e3, (Nz, NH))
    seeds, ps = dense_seeds(series, 13), dense_params(params(halo), 15)
    t1 = joint_tangent(d, dU, seeds, ps)
    t2 = joint_tangent(d, 2.0 * dU, {pair: 2.0 * s for pair, s in seeds.items()}, {name: 2.0 * v for name, v in ps.items()})
    tp = joint_tangent(d, 0.0, {}, ps)                                          # (the parameter seeds alone reach the state)
    for x in TANGENTS:
        assert np.any(t1[x] != 0.0) and np.array_equal(bits(2.0 * t1[x]), bits(t2[x])), x
    assert np.any(tp["internal_energy"] != 0.0)
    w = cotangents(Nz, NH, 37)
    g1 = joint_sweep(d, w, series)
    g2 = joint_sweep(d, {x: 2.0 * w[x] for x in w}, series)
    g0 = joint_sweep(d, {}, series)
    assert np.array_equal(bits(2.0 * g1[0]), bits(g2[0])) and np.all(g0[0] == 0.0)
    for pair in series:
        assert np.array_equal(bits(2.0 * g1[1][pair]), bits(g2[1][pair])) and np.all(g0[1][pair] == 0.0), pair
    assert np.any(g1[2] != 0.0) and np.array_equal(bits(2.0 * g1[2]), bits(g2[2])) and np.all(g0[2] == 0.0)


@pytest.mark.parametrize("Nz,bcset,halo,indexing", CASES)
def test_gradients_do_not_depend_on_the_partition(Nz, bcset, halo, indexing):
    d, bcs, series = joint_device(Nz, bcset, halo, indexing, steps_per_launch=0)
    w = cotangents(Nz, NH, 37)
    ref = joint_sweep(d, w, series)
    for spl in (1, 4):
        d.set_option("steps_per_launch", spl)
        for K in (None, 4):
            got = joint_sweep(d, w, series, checkpoint_every=K)
            assert np.array_equal(bits(got[0]), bits(ref[0])), (spl, K)
            for pair in series:
                assert np.array_equal(bits(got[1][pair]), bits(ref[1][pair])), (spl, K, pair)
            assert np.array_equal(bits(got[2]), bits(ref[2])), (spl, K)
    got = joint_sweep(d, w, series, calls=[(DT, 5), (DT, 3)])
    assert np.array_equal(bits(got[2]), bits(ref[2])) and all(np.array_equal(bits(got[1][pair]), bits(ref[1][pair])) for pair in series)


# ---- 4. the transpose of the parameter-seeded tangent of the new ride --------------------------------------------------------------------
def param_jacobians(d):
    """Jp[q][X][i, column] = dX_n[i] / d(parameter q): dU = 0, zero node seeds, a seed of 1 on that parameter"""
    return [joint_tangent(d, 0.0, {}, {name: 1.0}) for name in PARAMS]


@pytest.fixture(scope="module")
def yardstick():
    """(tolerance, {case: err_tan}, {case: (device, series, Jp)}): 8 x the largest err_tan over CASES -- all ten parameter seeds in one
    launch of the new ride against the extended-precision contraction of its ten one-hot runs; nothing of the adjoint enters"""
    err, kept = {}, {}
    for case in CASES:
        Nz, bcset, halo, indexing = case
        d, bcs, series = joint_device(Nz, bcset, halo, indexing, seed=29)
        Jp = param_jacobians(d)
        ps = dense_params(params(halo), 31)
        t = joint_tangent(d, 0.0, {}, ps)
        e = 0.0
        for x in TANGENTS:
            ref = sum(Jp[q][x].astype(LD) * LD(ps[name]) for q, name in enumerate(PARAMS))
            Ssum = sum(np.abs(Jp[q][x]).astype(LD) * abs(LD(ps[name])) for q, name in enumerate(PARAMS))
            e = max(e, normalised_error(t[x], ref, Ssum, ("parameter-seeded series tangent", x)))
        err[case], kept[case] = e, (d, series, Jp)
        print(f"yardstick Nz={Nz} {bcset} {halo} {indexing}: err_tan = {e:.3e}")
    tol = 8.0 * max(err.values())
    print(f"yardstick: largest err_tan = {max(err.values()):.3e}, transpose tolerance = {tol:.3e}")
    assert 0.0 < tol <= 1e-12
    return tol, err, kept


@pytest.mark.parametrize("Nz,bcset,halo,indexing", CASES)
def test_parameter_gradient_is_the_transpose_of_the_seeded_tangent(Nz, bcset, halo, indexing, yardstick):
    tol, err_tan, kept = yardstick
    d, series, Jp = kept[(Nz, bcset, halo, indexing)]
    w = cotangents(Nz, NH, 37)
    errs = {}
    for K in (None, 4):
        _, _, gp = joint_sweep(d, w, series, checkpoint_every=K)
        for q, name in enumerate(PARAMS):
            g_ref = sum(np.sum(Jp[q][x].astype(LD) * w[x].astype(LD), axis=0) for x in TANGENTS)
            Ssum = sum(np.sum(np.abs(Jp[q][x]).astype(LD) * np.abs(w[x]).astype(LD), axis=0) for x in TANGENTS)
            errs[(K, name)] = normalised_error(gp[q], g_ref, Ssum, ("parameter gradient", name, K))
    print(f"transpose Nz={Nz} {bcset} {halo} {indexing}: err_tan = {err_tan[(Nz, bcset, halo, indexing)]:.3e}, "
          f"largest err_adj = {max(errs.values()):.3e}, tolerance = {tol:.3e}")
    assert max(errs.values()) <= tol


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    I, U = CAPI.TRM_OK, CAPI.TRM_EUNSUPPORTED
    Nz, Nh = 10, 16
    p = params()
    Ustate, sat = mixed_state(Nz, Nh, p)
    times, ones = [0.0, 1e6], np.ones((2, Nh))

    def fresh(bcset="T_top+flux_bottom", series=1, both=1):
        d = device(Nz, Nh, p, Ustate, sat, boundary_sets(Nh)[bcset])
        d.set_option("derivative_series", series)
        d.set_option("derivative_series_params", both)
        assert d.get_option("derivative_series_params") == both
        return d

    def stepping(d):
        return ((d.step_tangent, (DT, 1)), (d.step_record, (DT, 1)), (d.adjoint_backward, ()))

    # the default is 0
    assert device(Nz, Nh, p, Ustate, sat, boundary_sets(Nh)["T_top+flux_bottom"]).get_option("derivative_series_params") == 0
    # the new option at 0: the two calls and the three stepping calls refuse, as before
    d = fresh(both=0)
    d.set_bc_series("temperature", "top", "value", times, ones)
    d.open_tangent()
    assert code_of(d.set_param_tangent, {"k_mineral": 1.0}) == U and "time series" in last_error(d)
    d.open_adjoint(4)
    assert code_of(d.open_param_gradient) == U and "time series" in last_error(d)
    d = fresh(both=0)
    d.open_tangent()
    d.set_tangent("internal_energy", 1.0)
    d.set_param_tangent({"k_mineral": 1.0})
    d.open_adjoint(4)
    d.open_param_gradient()
    d.set_bc_series("temperature", "top", "value", times, ones)
    for fn, args in stepping(d):
        assert code_of(fn, *args) == U and "time series" in last_error(d), fn.__name__
    # ... and the same context with the option at 1 runs all three
    d.set_option("derivative_series_params", 1)
    for fn, args in stepping(d):
        assert code_of(fn, *args) == I, (fn.__name__, last_error(d))
    assert d.last_program()["parameter_gradient"] and d.last_program()["series"] == 1
    # the new option at 1 without derivative_series: no series may be attached, as before
    d = fresh(series=0)
    d.set_bc_series("temperature", "top", "value", times, ones)
    d.open_tangent()
    d.set_tangent("internal_energy", 1.0)
    d.set_param_tangent({"k_mineral": 1.0})
    d.open_adjoint(4)
    d.open_param_gradient()
    for fn, args in stepping(d):
        assert code_of(fn, *args) == U and "no time series may be attached" in last_error(d), fn.__name__
    # both at 1: what the series ride refuses stays refused, with its messages
    def refused(d, why):
        d.open_tangent()
        d.set_tangent("internal_energy", 1.0)
        d.set_param_tangent({"k_mineral": 1.0})
        d.open_adjoint(4)
        d.open_param_gradient()
        for fn, args in stepping(d):
            assert code_of(fn, *args) == U, (why, fn.__name__)
            assert why in last_error(d), (why, last_error(d))

    d = fresh("gradient_top+flux_bottom")
    d.set_bc_series("internal_energy", "bottom", "flux", times, ones)
    refused(d, "generic boundary kinds")
    d = fresh()
    d.set_bc_series("internal_energy", "top", "gradient", times, ones)
    refused(d, "not of kind Gradient")
    d = fresh()
    d.set_forcing_series("air_temperature", times, ones)
    refused(d, "input (forcing)")
    d = fresh()
    d.set_bc_series("temperature", "top", "value", times, ones)
    d.series_window(("temperature", "top"), 4)
    refused(d, "windowed or trimmed")


# ---- 6. the Python layer ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("checkpoint_every", [None, 4])
def test_vjp_and_jvp_with_parameters_through_a_field_time_series(checkpoint_every, yardstick):
    tol = yardstick[0]
    Nz, Nh, nt, n = 20, 5, 5, 11
    w = cotangents(Nz, Nh, 61)
    a = build_series_integrator(Nh, nt, n)
    options = ("derivative_series", "derivative_series_params")
    assert [a.state.get_option(o) for o in options] == [0, 0]
    g, gb, gp = trm.vjp(a, n, checkpoint_every=checkpoint_every, wrt_boundary=True, wrt_params=True, **w)
    assert [a.state.get_option(o) for o in options] == [0, 0]                     # restored
    assert set(gb) == {("temperature", "top"), ("internal_energy", "bottom")} and tuple(gp) == PARAMS
    assert gb[("temperature", "top")].shape == (nt, Nh) and gb[("internal_energy", "bottom")].shape == (Nh,)
    g2, gb2 = trm.vjp(build_series_integrator(Nh, nt, n), n, checkpoint_every=checkpoint_every, wrt_boundary=True, **w)
    assert np.array_equal(bits(g2), bits(g)) and all(np.array_equal(bits(gb2[pair]), bits(gb[pair])) for pair in gb)
    rng = np.random.default_rng(67)
    for name in PARAMS:
        seed = float(np.ldexp(rng.choice([-1.0, 1.0]), int(rng.integers(-3, 4))))
        b = build_series_integrator(Nh, nt, n)
        tan = trm.jvp(b, 0.0, n, d_params={name: seed})
        assert [b.state.get_option(o) for o in options] == [0, 0]
        lhs = sum(np.sum(w[x].astype(LD) * tan[x].astype(LD), axis=0) for x in TANGENTS)
        Ssum = sum(np.sum(np.abs(w[x]).astype(LD) * np.abs(tan[x]).astype(LD), axis=0) for x in TANGENTS)
        err = normalised_error(gp[name] * seed, lhs, Ssum, ("jvp against vjp", name))
        print(f"jvp against vjp {name} checkpoint_every={checkpoint_every}: seed = {seed:g}, err = {err:.3e}, tolerance = {tol:.3e}")
        assert err <= tol
    assert all(np.any(gp[name] != 0.0) for name in ("k_water", "k_ice", "k_mineral", "c_water", "c_ice", "c_mineral"))
    # an exception inside the call restores both options
    c = build_series_integrator(Nh, nt, n)
    with pytest.raises(trm.TerrariumHipError):
        trm.jvp(c, 0.0, n, d_boundary={("temperature", "top"): np.zeros((nt + 1, Nh))}, d_params={"k_water": 1.0})
    assert [c.state.get_option(o) for o in options] == [0, 0]


def test_the_example_runs(yardstick):
    tol = yardstick[0]
    path = os.path.join(ROOT, "examples", "thermal_parameter_history_sensitivity.py")
    spec = importlib.util.spec_from_file_location("thermal_parameter_history_sensitivity", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    steps, nodes, columns = 12, 4, 3
    g, g_nodes, g_params = ex.reverse(steps, nodes, checkpoint_every=4, num_columns=columns)
    assert g.shape[1] == columns and g_nodes.shape == (nodes, columns) and np.all(g_nodes != 0.0) and tuple(g_params) == PARAMS
    for name in PARAMS:
        f, Ssum = ex.forward(name, steps, nodes, columns)
        err = normalised_error(g_params[name], f.astype(LD), Ssum.astype(LD), ("example", name))
        print(f"example {name}: vjp {g_params[name][0]:.6e}, jvp {f[0]:.6e}, err = {err:.3e}, tolerance = {tol:.3e}")
        assert err <= tol, name
