"""Derivatives of the heat-only run with respect to the ten thermal parameters: seeds on trm_step_tangent (trm_tangent_param_set),
gradients from trm_adjoint_backward (trm_adjoint_param_*), trm.jvp(d_params=...) and trm.vjp(wrt_params=True).

What holds exactly is checked exactly: the primal, g = dL/dU_0 and the boundary gradients are bit for bit what they are without, zero
seeds change nothing, scaling by two scales bit for bit, the gradients do not depend on how the tape is cut into launches and segments,
a constituent a column does not hold gives exact zeros, and the empty tape is the fold alone.  The gradients are then checked as the
transpose of the parameter-seeded tangent program (extended-precision contraction of its one-hot Jacobians) and both against
Richardson-extrapolated central differences of the oracle (parameter_derivatives.py).

The transpose tolerance is 8 x err_tan, err_tan measured when the module runs (the fixture `yardstick`) on the parameter-seeded tangent
program alone: one launch with a dense dU, dense boundary seeds and all ten parameter seeds against the extended-precision contraction
of that program's one-hot Jacobians, over TRANSPOSE_PARAM_CASES.  Nothing of the adjoint enters the bound.  Each test prints the
figures it measures before it asserts.

Measured on one MI355X (Parameter gradients): largest err_tan 9.9e-16, tolerance 7.9e-15, adjoint errors at most 5.4e-16
(3.7e-15 at size), central differences within 4.9e-10 of S."""
import ctypes

import numpy as np
import pytest

import workloads as W
import terrarium_jl_amd as trm
import parameter_derivatives as P
from boundary_derivatives import FD_DZ, FD_NH, FD_STEPS, HALOS, LD, PAIRS, active_pairs
from parameter_derivatives import PARAMS
from test_gpu_adjoint import TRANSPOSE_CASES, TRANSPOSE_COLUMNS, TRANSPOSE_STEPS, cotangents, normalised_error
from test_gpu_boundary_gradient import build_integrator
from test_gpu_tangent import (CAPI, DT, STATE, TANGENTS, assert_close_by_column, bits, boundary_sets, code_of, device, latent, mixed_state, oracle_state,
                              porosity, small)

pytestmark = pytest.mark.gpu

SETS = list(boundary_sets(2))
SIZES = (10, 32, 50)        # fewer than 32 lanes a column, exactly 32, the 64-lane layout (a partly filled wave)
NH = 48
# the cases of test_gpu_adjoint.py, one with organic matter, and the reference-zero halo with a Flux at both ends: no boundary value on
# temperature, so the dry halo cell is the only way the boundary faces see the parameters
TRANSPOSE_PARAM_CASES = [case + (0.0,) for case in TRANSPOSE_CASES] + [(32, "T_top+flux_bottom", "mirror", 26.0),
                                                                       (10, "flux_top+flux_bottom", "reference_zero", 0.0)]


def bc_of(bcset, Nh):
    if bcset == "flux_top+flux_bottom":
        return {("internal_energy", "top"): ("flux", 5.0), ("internal_energy", "bottom"): ("flux", 0.05)}
    return boundary_sets(Nh)[bcset]


def case_device(Nz, bcset, halo, Nh=NH, seed=7, rho_soc=0.0, steps_per_launch=0):
    p = P.thermal_params(halo, rho_soc)
    U, sat = mixed_state(Nz, Nh, p, seed=seed)
    bcs = bc_of(bcset, Nh)
    d = device(Nz, Nh, p, U, sat, bcs, steps_per_launch=steps_per_launch)
    d.save_state()
    return d, bcs


def sweep(d, calls, w, capacity=None, checkpoint_every=None, params=True, bc=True):
    """(g, {pair: boundary gradient}, {name: parameter gradient}) of the saved state: restores it, records `calls` on a fresh tape, pulls
    `w` back"""
    d.restore_state()
    steps = sum(n for _, n in calls)
    if checkpoint_every is None:
        d.open_adjoint(capacity or max(1, steps))
    else:
        d.open_adjoint(capacity or max(1, steps), checkpoint_every)      # (a slot per step is enough for any interval and split)
    if bc:
        d.open_bc_gradient()
    if params:
        d.open_param_gradient()
    for dt, n in calls:
        d.step_record(dt, n)
    for name in TANGENTS:
        d.set_cotangent(name, w.get(name, 0.0))
    d.adjoint_backward()
    return (d.cotangent("internal_energy"), {pair: d.bc_gradient(*pair) for pair in PAIRS} if bc or params else {},
            {name: d.param_gradient(name) for name in PARAMS} if params else {})


def param_tangent(d, calls, dU, bc_seeds, seeds):
    """{X: tangent of X} of the saved state under the seed dU, the boundary seeds {pair: values} and the parameter seeds {name: value};
    every seed left out is zero.  Always the parameter-seeded program."""
    d.restore_state()
    d.set_tangent("internal_energy", dU)
    for pair in PAIRS:
        d.set_bc_tangent(*pair, bc_seeds.get(pair, 0.0))
    d.set_param_tangent(seeds)
    for dt, n in calls:
        d.step_tangent(dt, n)
    prog = d.last_program()
    assert prog["parameter_seeds"] and prog["boundary_seeds"]
    return {x: d.tangent(x) for x in TANGENTS}


def fresh_device(d):
    """a device like `d` was built (closing what is open): tape, tangent and accumulators gone"""
    for close in (d.close_adjoint, d.close_tangent):
        code_of(close)


# ---- 1. the primal, zero seeds, scaling ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("halo", HALOS)
@pytest.mark.parametrize("bcset", ["T_top+flux_bottom", "gradient_bottom+T_top"])
@pytest.mark.parametrize("Nz", SIZES)
def test_primal_is_unchanged_and_seeds_are_linear(Nz, bcset, halo):
    n = 7
    p = P.thermal_params(halo, 26.0)
    U, sat = mixed_state(Nz, NH, p)
    bcs = boundary_sets(NH)[bcset]
    c = device(Nz, NH, p, U, sat, bcs)                          # trm_step, the library's own choice of program
    c.step(DT, n, finalize=True)
    dU = np.random.default_rng(1).normal(0.0, 1e3, (Nz, NH))
    rng = np.random.default_rng(3)
    bc_seeds = {pair: rng.normal(0.0, 1.0, NH) for pair in PAIRS}
    seeds = {name: (rng.normal(0.0, 0.1) if name.startswith("k_") else rng.normal(0.0, 1e4)) for name in PARAMS}
    t, u, z = (device(Nz, NH, p, U, sat, bcs, steps_per_launch=3) for _ in range(3))      # 7 steps: launches of 3, 3 and 1
    for d in (t, u, z):
        d.save_state()
        d.open_tangent()
    full = param_tangent(t, [(DT, n)], dU, bc_seeds, seeds)
    for name in STATE:
        assert np.array_equal(bits(t.get(name)), bits(c.get(name))), name
    assert t.status() == c.status() and t.clock() == c.clock()
    # ten zero seeds: the unseeded run's tangents, from the other program
    u.set_tangent("internal_energy", dU)
    u.step_tangent(DT, n)
    pu = u.last_program()
    assert not pu["parameter_seeds"] and not pu["boundary_seeds"]
    zero = param_tangent(z, [(DT, n)], dU, {}, {name: 0.0 for name in PARAMS})
    pz = z.last_program()
    assert {k: v for k, v in pz.items() if k not in ("parameter_seeds", "boundary_seeds")} == \
           {k: v for k, v in pu.items() if k not in ("parameter_seeds", "boundary_seeds")}
    for x in TANGENTS:
        assert np.array_equal(zero[x], u.tangent(x)), x
    assert any(not np.array_equal(full[x], zero[x]) for x in TANGENTS)
    # doubling every seed doubles every tangent
    twice = param_tangent(t, [(DT, n)], 2.0 * dU, {pair: 2.0 * s for pair, s in bc_seeds.items()}, {name: 2.0 * s for name, s in seeds.items()})
    for x in TANGENTS:
        assert np.array_equal(bits(twice[x]), bits(2.0 * full[x])), x
    # trm_tangent_closure carries the heat-capacity term: from the step's dU it forms the step's dT and dliq again (the same expression
    # on the same stored U, by the cell-per-thread closure: a few roundings of fp64 apart at the most), and with dU = 0 what is left
    # is -(T / C) dC, zero exactly where the cell is in phase change
    t.tangent_closure()
    for x in ("temperature", "liquid_water_fraction"):
        assert np.allclose(t.tangent(x), twice[x], rtol=1e-12, atol=1e-12 * np.max(np.abs(twice[x]))), x
    t.set_tangent("internal_energy", 0.0)
    t.set_param_tangent({"c_mineral": 1.0})
    t.tangent_closure()
    T, dT = t.get("temperature"), t.tangent("temperature")
    assert np.all(dT[T == 0.0] == 0.0) and np.all(dT[T > 0.0] < 0.0) and np.all(dT[T < 0.0] > 0.0)
    assert np.all(t.tangent("liquid_water_fraction") == 0.0)


# ---- 2. nothing else moves ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("halo", HALOS)
@pytest.mark.parametrize("bcset", SETS)
@pytest.mark.parametrize("Nz", SIZES)
def test_initial_state_and_boundary_gradients_are_unchanged(Nz, bcset, halo):
    n = 7
    d, bcs = case_device(Nz, bcset, halo, steps_per_launch=3)
    w = cotangents(Nz, NH, 2)
    g, gb, gp = sweep(d, [(DT, n)], w)
    pa = d.last_program()
    final = {name: d.get(name) for name in STATE}
    fresh_device(d)
    g0, gb0, _ = sweep(d, [(DT, n)], w, params=False)
    pb = d.last_program()
    assert pa["family"] == "column_adjoint" and pa["backward"] and pa["boundary_gradient"] and pa["parameter_gradient"]
    assert pb["boundary_gradient"] and not pb["parameter_gradient"]
    assert {k: v for k, v in pa.items() if k != "parameter_gradient"} == {k: v for k, v in pb.items() if k != "parameter_gradient"}
    assert np.array_equal(bits(g), bits(g0))
    for pair in PAIRS:
        assert np.array_equal(bits(gb[pair]), bits(gb0[pair])), pair
    for name in STATE:
        assert np.array_equal(bits(final[name]), bits(d.get(name))), name
    fresh_device(d)
    g1, _, _ = sweep(d, [(DT, n)], w, params=False, bc=False)
    assert np.array_equal(bits(g), bits(g1)) and not d.last_program()["boundary_gradient"]
    for name in PARAMS:
        assert gp[name].shape == (NH,) and np.all(np.isfinite(gp[name])), name
        if not name.endswith("organic"):
            assert np.any(gp[name] != 0.0), name


# ---- 3. the sums do not depend on how the tape is cut -----------------------------------------------------------------------------------
@pytest.mark.parametrize("halo", HALOS)
@pytest.mark.parametrize("bcset", ["T_top+flux_bottom", "gradient_top+flux_bottom", "flux_top+T_bottom"])
@pytest.mark.parametrize("Nz", SIZES)
def test_parameter_gradients_do_not_depend_on_the_partition(Nz, bcset, halo):
    d, bcs = case_device(Nz, bcset, halo, seed=19, rho_soc=26.0)
    w = cotangents(Nz, NH, 23)
    for calls in ([(DT, 4), (DT, 4), (DT, 3)], [(DT, 4), (0.5 * DT, 3)]):       # (K = 4: segments of 4 4 3; of 4 3)
        d.set_option("steps_per_launch", 0)
        g_ref, _, ref = sweep(d, calls, w)
        assert not d.last_program()["checkpointed"] and d.last_program()["parameter_gradient"]
        d.set_option("steps_per_launch", 2)
        g, _, got = sweep(d, calls, w)
        assert np.array_equal(bits(g), bits(g_ref))
        for name in PARAMS:
            assert np.array_equal(bits(got[name]), bits(ref[name])), ("steps_per_launch 2", calls, name)
        d.set_option("steps_per_launch", 0)
        for K in (1, 4, 16):
            g, _, got = sweep(d, calls, w, checkpoint_every=K)
            assert d.last_program()["checkpointed"] and d.last_program()["parameter_gradient"]
            assert np.array_equal(bits(g), bits(g_ref))
            for name in PARAMS:
                assert np.array_equal(bits(got[name]), bits(ref[name])), ("checkpointed", K, calls, name)
        _, _, twice = sweep(d, calls, {name: 2.0 * x for name, x in w.items()})
        _, _, none = sweep(d, calls, {})
        for name in PARAMS:
            assert np.any(ref[name] != 0.0), name
            assert np.array_equal(bits(twice[name]), bits(2.0 * ref[name])), name
            assert np.all(none[name] == 0.0), name


# ---- 4. exact zeros --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("halo", HALOS)
@pytest.mark.parametrize("Nz", SIZES)
def test_a_constituent_a_column_does_not_hold_has_a_zero_gradient(Nz, halo):
    """no organic matter: nothing depends on k_organic or c_organic.  Columns frozen throughout hold no liquid water, columns thawed
    throughout no ice -- a Value on the surface temperature of the same sign keeps them so, which the oracle confirms."""
    n = 6
    p = P.thermal_params(halo, 0.0)
    rng = np.random.default_rng(53)
    sat = rng.uniform(0.3, 1.0, (Nz, NH))
    L = latent(p, sat)
    far = rng.uniform(2e5, 8e6, (Nz, NH))
    frozen = np.arange(NH) % 2 == 0
    U = np.where(frozen[None, :], -L - far, far)
    bcs = {("temperature", "top"): ("value", np.where(frozen, -3.0, 3.0))}
    o = oracle_state(Nz, NH, p, U, sat, bcs)
    for _ in range(n + 1):
        Uo = o.get("internal_energy")
        assert np.all(Uo[:, frozen] < -L[:, frozen]) and np.all(Uo[:, ~frozen] > 0.0)
        o.timestep(DT)
    d = device(Nz, NH, p, U, sat, bcs, steps_per_launch=4)
    d.save_state()
    _, _, g = sweep(d, [(DT, n)], cotangents(Nz, NH, 59))
    assert np.all(g["k_organic"] == 0.0) and np.all(g["c_organic"] == 0.0)
    assert np.all(g["k_water"][frozen] == 0.0) and np.all(g["c_water"][frozen] == 0.0)
    assert np.all(g["k_ice"][~frozen] == 0.0) and np.all(g["c_ice"][~frozen] == 0.0)
    assert np.all(g["c_water"][~frozen] != 0.0) and np.all(g["k_water"][~frozen] != 0.0)
    assert np.all(g["c_ice"][frozen] != 0.0) and np.all(g["k_ice"][frozen] != 0.0)
    for name in ("k_air", "k_mineral", "c_air", "c_mineral"):
        assert np.all(g[name] != 0.0), name
    # a seed on k_organic alone: every tangent stays zero
    d.open_tangent()
    t = param_tangent(d, [(DT, n)], 0.0, {}, {"k_organic": 1.0})
    for x in TANGENTS:
        assert np.all(t[x] == 0.0), x
    t = param_tangent(d, [(DT, n)], 0.0, {}, {"k_mineral": 1.0})
    assert np.any(t["internal_energy"] != 0.0)


# ---- 5. the empty tape --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("halo", HALOS)
@pytest.mark.parametrize("rho_soc", P.RHO_SOC)
def test_empty_tape_is_the_fold_alone(rho_soc, halo):
    """no taped step: the heat-capacity gradients are sum_i wT_i (-T_i / C_i) theta_i of the stored state, the conductivity gradients 0"""
    Nz, Nh = 12, 96
    p = P.thermal_params(halo, rho_soc)
    U, sat = mixed_state(Nz, Nh, p, seed=19)
    d = device(Nz, Nh, p, U, sat, {("temperature", "top"): ("value", 1.0)})
    d.save_state()
    T, liq = d.get("temperature"), d.get("liquid_water_fraction")
    w = cotangents(Nz, Nh, 29)
    # (every term of a column's sum with one sign, so that rtol = 1e-14 of the sum is 1e-14 of its terms)
    w["temperature"] = np.abs(w["temperature"]) * np.where(T < 0, -1.0, 1.0)
    for K in (None, 4):
        _, _, g = sweep(d, [], w, checkpoint_every=K)
        por = porosity(p)
        org = p.rho_soc / ((1.0 - p.por_organic) * p.rho_org)
        theta = {"c_water": sat * por * liq, "c_ice": sat * por * (1.0 - liq), "c_air": (1.0 - sat) * por,
                 "c_mineral": np.full((Nz, Nh), (1.0 - por) * (1.0 - org)), "c_organic": np.full((Nz, Nh), (1.0 - por) * org)}
        C = sum(getattr(p, name) * theta[name] for name in P.CAPACITIES)
        for name in P.CAPACITIES:
            ref = np.sum(w["temperature"].astype(LD) * (-T.astype(LD) / C.astype(LD)) * theta[name].astype(LD), axis=0).astype(np.float64)
            worst = float(np.max(np.abs(g[name] - ref) / np.maximum(np.abs(ref), 1e-300))) if np.any(ref != 0) else 0.0
            print(f"empty tape rho_soc={rho_soc:g} {halo} K={K} {name}: max relative error {worst:.3e}")
            np.testing.assert_allclose(g[name], ref, rtol=1e-14, atol=0.0, err_msg=name)
        for name in P.CONDUCTIVITIES:
            assert np.all(g[name] == 0.0), name


# ---- 6. the transpose of the parameter-seeded tangent program ---------------------------------------------------------------------------
def param_jacobians(d, Nz, calls, pairs, cols=slice(None), state=True):
    """(J, Jb, Jp) of the saved state by the parameter-seeded tangent program: J[X][i, j, column] = dX_n[i] / dU_0[j] from one-hot dU,
    Jb[pair][X][i, column] from a seed of 1 on that pair, Jp[name][X][i, column] from dU = 0 and a unit seed on that parameter"""
    Nh = d.grid.Nh
    J = None
    if state:
        J = {x: np.zeros((Nz, Nz, len(range(Nh)[cols]))) for x in TANGENTS}
        for j in range(Nz):
            e = np.zeros((Nz, Nh))
            e[j] = 1.0
            t = param_tangent(d, calls, e, {}, {})
            for x in TANGENTS:
                J[x][:, j, :] = t[x][:, cols]
    Jb = {}
    for pair in pairs:
        t = param_tangent(d, calls, 0.0, {pair: 1.0}, {})
        Jb[pair] = {x: t[x][:, cols] for x in TANGENTS}
    Jp = {}
    for name in PARAMS:
        t = param_tangent(d, calls, 0.0, {}, {name: 1.0})
        Jp[name] = {x: t[x][:, cols] for x in TANGENTS}
    return J, Jb, Jp


def param_tangent_error(d, J, Jb, Jp, Nz, calls, seed):
    """err_tan: one launch with a dense dU, dense seeds on every pair of Jb and all ten parameter seeds against the extended-precision
    contraction of the one-hot Jacobians, normalised by the sum of absolute values"""
    rng = np.random.default_rng(seed)
    Nh = d.grid.Nh
    v = rng.normal(0.0, 1e3, (Nz, Nh))
    bc_seeds = {pair: rng.normal(0.0, 1.0, Nh) for pair in Jb}
    seeds = {name: float(rng.normal(0.0, 0.1) if name.startswith("k_") else rng.normal(0.0, 1e4)) for name in PARAMS}
    t = param_tangent(d, calls, v, bc_seeds, seeds)
    err = 0.0
    for x in TANGENTS:
        ref = np.einsum("ijc,jc->ic", J[x].astype(LD), v.astype(LD))
        S = np.einsum("ijc,jc->ic", np.abs(J[x]).astype(LD), np.abs(v).astype(LD))
        for pair, s in bc_seeds.items():
            ref = ref + Jb[pair][x].astype(LD) * s.astype(LD)[None, :]
            S = S + np.abs(Jb[pair][x]).astype(LD) * np.abs(s).astype(LD)[None, :]
        for name, s in seeds.items():
            ref = ref + Jp[name][x].astype(LD) * LD(s)
            S = S + np.abs(Jp[name][x]).astype(LD) * abs(LD(s))
        err = max(err, normalised_error(t[x], ref, S, ("parameter-seeded tangent", x)))
    return err


def parameter_reference(Jp_name, w):
    """(g_ref, S)[column] = sum_X sum_i J_X,q[i] w_X[i] in extended precision, and the same sum of absolute values"""
    g = sum(np.sum(Jp_name[x].astype(LD) * w[x].astype(LD), axis=0) for x in TANGENTS)
    S = sum(np.sum(np.abs(Jp_name[x]).astype(LD) * np.abs(w[x]).astype(LD), axis=0) for x in TANGENTS)
    return g, S


@pytest.fixture(scope="module")
def yardstick():
    """(tolerance, {case: err_tan}, {case: (device, parameter Jacobians)}): 8 x the largest err_tan over TRANSPOSE_PARAM_CASES"""
    err, kept = {}, {}
    calls = [(DT, TRANSPOSE_STEPS)]
    for case in TRANSPOSE_PARAM_CASES:
        Nz, bcset, halo, rho_soc = case
        d, bcs = case_device(Nz, bcset, halo, Nh=TRANSPOSE_COLUMNS, seed=29, rho_soc=rho_soc)
        d.open_tangent()
        J, Jb, Jp = param_jacobians(d, Nz, calls, active_pairs(bcs))
        err[case] = param_tangent_error(d, J, Jb, Jp, Nz, calls, seed=31)
        kept[case] = (d, Jp)
        print(f"yardstick Nz={Nz} {bcset} {halo} rho_soc={rho_soc:g}: err_tan = {err[case]:.3e}")
    tol = 8.0 * max(err.values())
    print(f"yardstick: largest err_tan = {max(err.values()):.3e}, transpose tolerance = {tol:.3e}")
    # (above the additivity tolerance of test_tangent_is_exactly_linear the measurement itself would be wrong)
    assert 0.0 < tol <= 1e-12
    return tol, err, kept


@pytest.mark.parametrize("Nz,bcset,halo,rho_soc", TRANSPOSE_PARAM_CASES)
def test_parameter_gradient_is_the_transpose_of_the_seeded_tangent(Nz, bcset, halo, rho_soc, yardstick):
    tol, err_tan, kept = yardstick
    d, Jp = kept[(Nz, bcset, halo, rho_soc)]
    w = cotangents(Nz, TRANSPOSE_COLUMNS, 37)
    _, _, g = sweep(d, [(DT, TRANSPOSE_STEPS)], w)
    errs = {}
    for name in PARAMS:
        g_ref, S = parameter_reference(Jp[name], w)
        if rho_soc == 0.0 and name.endswith("organic"):
            assert np.all(S == 0)
        else:
            assert np.any(S > 0), name
        errs[name] = normalised_error(g[name], g_ref, S, ("parameter gradient", name))       # (columns with S = 0: == 0.0)
    print(f"transpose Nz={Nz} {bcset} {halo} rho_soc={rho_soc:g}: err_tan = {err_tan[(Nz, bcset, halo, rho_soc)]:.3e}, tolerance = {tol:.3e}, "
          + ", ".join(f"{name} {e:.3e}" for name, e in errs.items()))
    assert max(errs.values()) <= tol


# ---- 7. central differences of the oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bcset,halo,rho_soc", P.FD_CASES)
def test_parameter_derivatives_match_central_differences_of_the_oracle(bcset, halo, rho_soc):
    (p, U0, sat, bcs, w), keep, ref = P.fd_reference(bcset, halo, rho_soc)
    print(f"{bcset} {halo} rho_soc={rho_soc:g}: kept share {keep.mean():.4f}")
    assert keep.mean() >= P.FD_KEEP_SHARE
    grid = trm.ColumnGrid(trm.PrescribedSpacing(dz=FD_DZ), FD_NH)
    d = trm.DeviceState(grid, p)
    d.set("saturation_water_ice", sat)
    d.set("internal_energy", U0)
    for (var, side), (kind, value) in bcs.items():
        d.set_bc(var, side, kind, value)
    d.closure()
    d.save_state()
    calls = [(DT, FD_STEPS)]
    _, _, g = sweep(d, calls, w)
    d.open_tangent()
    failures = []
    for name in PARAMS:
        rich = ref[name][0]
        fd, S = P.loss_and_scale(rich, w)
        floor = 1e-9 * np.max(S[keep])
        err = np.abs(fd - g[name].astype(LD))[keep]
        worst = float(np.max(err / np.maximum(S[keep], LD(1e-300)))) if np.any(S[keep] > 0) else 0.0
        print(f"central differences {bcset} {halo} rho_soc={rho_soc:g} {name}: h = {P.fd_step(p, name):g}, max err / S = {worst:.3e}")
        t = param_tangent(d, calls, 0.0, {}, {name: 1.0})
        for x in TANGENTS:
            scale = np.max(np.abs(t[x][:, keep]), axis=0)
            bound = 1e-6 * scale[None, :] + 1e-9 * np.max(scale)           # (assert_close_by_column's)
            ratio = float(np.max(np.abs(rich[x][:, keep] - t[x][:, keep]) / np.maximum(bound, 1e-300))) if np.max(scale) > 0 else 0.0
            print(f"    tangent of {x}: max err / (1e-6 column scale + floor) = {ratio:.3e}")
        if not np.all(err <= 1e-6 * S[keep] + floor):
            failures.append(name)
        for x in TANGENTS:      # (the extrapolation as a central difference over a unit step)
            assert_close_by_column(rich[x].astype(np.float64), np.zeros_like(t[x]), 0.5, t[x], keep, 1e-6, (x, name))
    assert not failures, failures


# ---- 8. at size ---------------------------------------------------------------------------------------------------------------------------
def test_parameter_gradient_is_the_transpose_at_size(yardstick):
    tol = yardstick[0]
    lat, lon = W.columns_from_mask("N145")
    Nz, n = 32, 10
    w = W.make_workload("heat", lat, lon, Nz)
    d = W.setup_device(w, steps_per_launch=0)
    d.closure()
    Nh = d.grid.Nh
    d.save_state()
    d.open_tangent()
    calls = [(w["dt"], n)]
    assert active_pairs(w["bcs"]) == [("temperature", "top")]
    cols = slice(None, None, 25)
    _, _, Jp = param_jacobians(d, Nz, calls, [], cols=cols, state=False)
    d.close_tangent()
    cot = cotangents(Nz, Nh, 47)
    _, _, g = sweep(d, calls, cot, checkpoint_every=16)
    prog = d.last_program()
    assert prog["family"] == "column_adjoint" and prog["lanes_per_column"] == 32 and prog["checkpointed"] and prog["parameter_gradient"]
    some = {x: cot[x][:, cols] for x in TANGENTS}
    errs = {}
    for name in PARAMS:
        g_ref, S = parameter_reference(Jp[name], some)
        errs[name] = normalised_error(g[name][cols], g_ref, S, ("parameter gradient at size", name))
        assert np.all(np.isfinite(g[name]))
    print(f"transpose at size: {Nh} columns, every 25th checked, tolerance = {tol:.3e}, " + ", ".join(f"{name} {e:.3e}" for name, e in errs.items()))
    assert np.any(g["k_mineral"] != 0.0) and np.any(g["c_mineral"] != 0.0)
    assert max(errs.values()) <= tol


# ---- 9. refusals and the Python layer --------------------------------------------------------------------------------------------------
def test_refusals():
    U, E, S, I = CAPI.TRM_EUNSUPPORTED, CAPI.TRM_EINVAL, CAPI.TRM_ESTALE, CAPI.TRM_OK
    d = small()
    buf = (ctypes.c_double * 16)()
    seed = (ctypes.c_double * 10)()
    dev = ctypes.c_void_p()
    # nothing open
    assert code_of(d.set_param_tangent, {"k_water": 1.0}) == E
    assert code_of(d.open_param_gradient) == E
    assert code_of(d.param_gradient, "k_water") == E
    assert d._lib.trm_adjoint_param_device_ptr(d._ctx, 0, ctypes.byref(dev)) == E
    d.open_tangent()
    d.open_adjoint(4)
    # before trm_adjoint_param_open, also with boundary gradients open
    assert code_of(d.open_bc_gradient) == I
    assert code_of(d.param_gradient, "k_water") == E
    assert d._lib.trm_adjoint_param_device_ptr(d._ctx, 0, ctypes.byref(dev)) == E
    assert code_of(d.open_param_gradient) == I
    assert code_of(d.bc_gradient, "temperature", "top") == I           # (it implies trm_adjoint_bc_open)
    for which in range(10):
        assert d._lib.trm_adjoint_param_download(d._ctx, which, buf) == I
        assert d._lib.trm_adjoint_param_device_ptr(d._ctx, which, ctypes.byref(dev)) == I and dev.value
    # a bad `which`, NULL pointers
    for which in (-1, 10, 99):
        assert d._lib.trm_adjoint_param_download(d._ctx, which, buf) == E
        assert d._lib.trm_adjoint_param_device_ptr(d._ctx, which, ctypes.byref(dev)) == E
    assert d._lib.trm_adjoint_param_download(d._ctx, 0, None) == E
    assert d._lib.trm_adjoint_param_device_ptr(d._ctx, 0, None) == E
    assert d._lib.trm_tangent_param_set(d._ctx, None) == E
    with pytest.raises(KeyError):
        d.set_param_tangent({"porosity": 1.0})
    # a stale tape stays stale with parameters open; seeds are not state
    d.set_tangent("internal_energy", 1.0)
    assert d._lib.trm_tangent_param_set(d._ctx, seed) == I
    assert code_of(d.step_tangent, DT, 1) == I and d.last_program()["parameter_seeds"]
    d.open_adjoint(4)
    assert code_of(d.step_record, DT, 2) == I
    d.step(DT, 1)                                                   # (a state change behind the tape's back)
    assert code_of(d.adjoint_backward) == S
    assert code_of(d.step_tangent, DT, 1) == S
    assert code_of(d.set_param_tangent, {"c_ice": 1.0}) == I
    assert code_of(d.step_tangent, DT, 1) == S                     # (a parameter seed does not seed dU)
    d.open_adjoint(4)
    assert code_of(d.step_record, DT, 1) == I
    assert code_of(d.adjoint_backward) == I and d.last_program()["parameter_gradient"]
    assert all(np.all(d.param_gradient(name) == 0.0) for name in PARAMS)      # (zero cotangents)
    # open_tangent zeroes the seeds and goes back to the unseeded instance; closing frees
    d.open_tangent()
    assert code_of(d.step_tangent, DT, 1) == I and not d.last_program()["parameter_seeds"]
    d.close_adjoint()
    assert code_of(d.param_gradient, "k_water") == E
    d.open_adjoint(4)
    assert code_of(d.param_gradient, "k_water") == E               # (closed with the adjoint: not open again)
    d.close_tangent()
    assert code_of(d.set_param_tangent, {"k_water": 1.0}) == E
    # a conductivity of zero: sqrt has no derivative there
    dry = P.thermal_params()
    dry.k_air = 0.0
    z = small(p=dry)
    z.open_tangent()
    z.open_adjoint(4)
    assert code_of(z.set_param_tangent, {"k_water": 1.0}) == E and code_of(z.open_param_gradient) == E
    assert code_of(z.open_bc_gradient) == I
    # fp32 and Richards: unsupported
    f = small(dtype=np.float32)
    assert code_of(f.set_param_tangent, {"k_water": 1.0}) == U and code_of(f.open_param_gradient) == U
    rich = P.thermal_params()
    rich.flow = CAPI.FLOW["richards"]
    r = small(p=rich)
    assert code_of(r.open_adjoint, 4) == U and code_of(r.open_param_gradient) == U and code_of(r.set_param_tangent, {"k_water": 1.0}) == U


@pytest.mark.parametrize("checkpoint_every", [None, 4])
def test_vjp_and_jvp_with_respect_to_parameters(checkpoint_every, yardstick):
    tol = yardstick[0]
    Nz, Nh, n = 20, 5, 11
    w = cotangents(Nz, Nh, 61)
    g, gp = trm.vjp(build_integrator(Nh), n, checkpoint_every=checkpoint_every, wrt_params=True, **w)
    assert tuple(gp) == PARAMS
    plain = trm.vjp(build_integrator(Nh), n, checkpoint_every=checkpoint_every, **w)
    assert isinstance(plain, np.ndarray) and np.array_equal(bits(plain), bits(g))
    g3, gb3, gp3 = trm.vjp(build_integrator(Nh), n, checkpoint_every=checkpoint_every, wrt_boundary=True, wrt_params=True, **w)
    g2, gb2 = trm.vjp(build_integrator(Nh), n, checkpoint_every=checkpoint_every, wrt_boundary=True, **w)
    assert np.array_equal(bits(g3), bits(g)) and np.array_equal(bits(g2), bits(g))
    assert set(gb3) == set(gb2) == {("temperature", "top"), ("internal_energy", "bottom")}
    for pair in gb2:
        assert np.array_equal(bits(gb3[pair]), bits(gb2[pair])), pair
    for name in PARAMS:
        assert gp[name].shape == (Nh,) and np.array_equal(bits(gp[name]), bits(gp3[name])), name
    # <w, jvp(seed)> = <parameter gradient, seed>, one parameter at a time; a seed of +-2^k scales the tangent of a unit seed exactly,
    # so this is the identity of the transpose check
    rng = np.random.default_rng(67)
    for name in PARAMS:
        seed = float(np.ldexp(rng.choice([-1.0, 1.0]), int(rng.integers(-3, 4))))
        tan = trm.jvp(build_integrator(Nh), 0.0, n, d_params={name: seed})
        lhs = sum(np.sum(w[x].astype(LD) * tan[x].astype(LD), axis=0) for x in TANGENTS)
        S = sum(np.sum(np.abs(w[x]).astype(LD) * np.abs(tan[x]).astype(LD), axis=0) for x in TANGENTS)
        err = normalised_error(gp[name] * seed, lhs, S, ("jvp against vjp", name))
        print(f"jvp against vjp {name} checkpoint_every={checkpoint_every}: seed = {seed:g}, err = {err:.3e}, tolerance = {tol:.3e}")
        assert err <= tol
        assert np.any(gp[name] != 0.0) == bool(np.any(S > 0)), name      # (a saturated column holds no air, this one no organic matter)
    assert all(np.any(gp[name] != 0.0) for name in ("k_water", "k_ice", "k_mineral", "c_water", "c_ice", "c_mineral"))
