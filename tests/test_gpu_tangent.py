"""Forward-mode tangents of the heat-only SoilModel step (trm_tangent_*, trm_step_tangent, trm.jvp).

The primal of trm_step_tangent is checked bit for bit against a twin context stepped by trm_step; the tangent against the closure
slopes of the reference's differentiability test (soil_energy_diff.jl:28-76), against central differences of the oracle's primal and
of the device's own trm_step, for exact linearity and for locality; and every refusal and staleness rule of the ABI."""
import importlib.util
import os

import numpy as np
import pytest

import workloads as W
import terrarium_jl_amd as trm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPI = trm._capi
STATE = ("internal_energy", "temperature", "liquid_water_fraction", "saturation_water_ice", "hydraulic_conductivity", "tend_internal_energy")
TANGENTS = ("internal_energy", "temperature", "liquid_water_fraction")
DT = 300.0


def params(halo="reference_zero"):
    p = CAPI.default_params()
    p.halo_policy = CAPI.HALO[halo]
    return p


def porosity(p):
    org = p.rho_soc / ((1.0 - p.por_organic) * p.rho_org)
    return (1.0 - org) * p.por_mineral + org * p.por_organic


def latent(p, sat):
    """L_theta = rho_w Lsl sat por"""
    return p.rho_w * p.Lsl * sat * porosity(p)


def mixed_state(Nz, Nh, p, seed=7):
    """(U, sat): every cell drawn thawed, in phase change or frozen, 0.2 MJ/m3 or more from the regime boundaries"""
    rng = np.random.default_rng(seed)
    sat = rng.uniform(0.3, 1.0, (Nz, Nh))
    L = latent(p, sat)
    regime = rng.integers(0, 3, (Nz, Nh))
    far = rng.uniform(2e5, 8e6, (Nz, Nh))
    U = np.where(regime == 0, far, np.where(regime == 1, -rng.uniform(0.1, 0.9, (Nz, Nh)) * L, -L - far))
    return U, sat


def boundary_sets(Nh):
    T_top, T_bot = np.linspace(-4.0, 4.0, Nh), np.linspace(3.0, -3.0, Nh)
    return {
        "noflux": {},
        "T_top": {("temperature", "top"): ("value", T_top)},
        "T_top+flux_bottom": {("temperature", "top"): ("value", T_top), ("internal_energy", "bottom"): ("flux", 0.05)},
        "flux_top+T_bottom": {("internal_energy", "top"): ("flux", 5.0), ("temperature", "bottom"): ("value", T_bot)},
        "gradient_bottom+T_top": {("temperature", "bottom"): ("gradient", 0.03), ("temperature", "top"): ("value", T_top)},
        "gradient_top+flux_bottom": {("temperature", "top"): ("gradient", -0.5), ("internal_energy", "bottom"): ("flux", 0.05)},
        "zero_gradient_bottom+T_top": {("temperature", "bottom"): ("gradient", 0.0), ("temperature", "top"): ("value", T_top)},
    }


def thickness(Nz):
    return trm.ExponentialSpacing(N=Nz).get_spacing()


def device(Nz, Nh, p, U, sat, bcs, steps_per_launch=0):
    grid = trm.ColumnGrid(trm.PrescribedSpacing(dz=list(thickness(Nz))), Nh)
    d = trm.DeviceState(grid, p)
    d.set_option("steps_per_launch", steps_per_launch)
    d.set("saturation_water_ice", sat)
    d.set("internal_energy", U)
    for (var, side), (kind, value) in bcs.items():
        d.set_bc(var, side, kind, value)
    d.closure()
    return d


def oracle_state(Nz, Nh, p, U, sat, bcs):
    import oracle
    o = oracle.Oracle(Nh, thickness(Nz), oracle.default_params(halo_policy=p.halo_policy))
    o.set("saturation_water_ice", sat)
    o.set("internal_energy", U)
    for (var, side), (kind, value) in bcs.items():
        o.set_bc(var, side, kind, value)
    o.closure()
    return o


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def code_of(fn, *args):
    try:
        fn(*args)
    except trm.TerrariumHipError as e:
        return e.code
    return CAPI.TRM_OK


# ---- the primal: bit for bit what trm_step computes ---------------------------------------------------------------------------
@pytest.mark.parametrize("halo", ["reference_zero", "mirror"])
@pytest.mark.parametrize("bcset", list(boundary_sets(2)))
@pytest.mark.parametrize("Nz", [10, 32, 50])
def test_primal_is_trm_step_bit_for_bit(Nz, bcset, halo):
    Nh, n = 301, 7
    p = params(halo)
    U, sat = mixed_state(Nz, Nh, p)
    bcs = boundary_sets(Nh)[bcset]
    a = device(Nz, Nh, p, U, sat, bcs, steps_per_launch=3)      # 7 steps: launches of 3, 3 and 1
    b = device(Nz, Nh, p, U, sat, bcs)                          # the library's own choice of program
    a.open_tangent()
    a.set_tangent("internal_energy", np.random.default_rng(1).normal(0.0, 1e3, (Nz, Nh)))
    a.step_tangent(DT, n)
    b.step(DT, n, finalize=True)
    for name in STATE:
        assert np.array_equal(bits(a.get(name)), bits(b.get(name))), name
    assert a.status() == b.status() and a.clock() == b.clock()
    prog = a.last_program()
    assert prog["family"] == "column_tangent" and prog["lanes_per_column"] == (32 if Nz <= 32 else 64)
    assert prog["generic_boundaries"] == bool(b.get_option("info_generic_boundary_kernels"))
    for name in TANGENTS:
        assert np.all(np.isfinite(a.tangent(name))), name


# ---- closure slopes (soil_energy_diff.jl:28-76) ---------------------------------------------------------------------------------
def test_closure_slopes_match_the_reference_cases():
    Nz, Nh = 4, 64
    p = params()
    por = porosity(p)
    sat = np.ones((Nz, Nh))
    sat[:, 48:] = 0.0                                           # L_theta = 0
    L = latent(p, sat)
    regime = np.tile(np.arange(Nh) % 3, (Nz, 1))               # 0 thawed, 1 phase change, 2 frozen
    regime[:, 48:] = np.where(np.arange(Nh - 48) % 2 == 0, 0, 2)
    U = np.where(regime == 0, 1.0e7, np.where(regime == 1, -0.5 * L, -L - 1.0e7))
    d = device(Nz, Nh, p, U, sat, {})
    d.open_tangent()
    d.set_tangent("internal_energy", 1.0)
    d.tangent_closure()
    dT, dl = d.tangent("temperature"), d.tangent("liquid_water_fraction")
    solid = p.c_mineral * (1.0 - por)
    C_thawed = p.c_water * sat * por + p.c_air * (1.0 - sat) * por + solid
    C_frozen = p.c_ice * sat * por + p.c_air * (1.0 - sat) * por + solid
    th, pc, fr = regime == 0, regime == 1, regime == 2
    assert th.any() and pc.any() and fr.any()
    np.testing.assert_allclose(dl[pc], 1.0 / L[pc], rtol=1e-14)     # dliq/dU = 1 / L_theta
    assert np.all(dT[pc] == 0.0)                                     # T = 0 in phase change
    np.testing.assert_allclose(dT[th], 1.0 / C_thawed[th], rtol=1e-14)
    np.testing.assert_allclose(dT[fr], 1.0 / C_frozen[fr], rtol=1e-14)
    assert np.all(dl[th | fr] == 0.0)
    assert np.all(dl[sat == 0.0] == 0.0)                             # L_theta = 0


# ---- finite differences -------------------------------------------------------------------------------------------------------
def regime_distance(U, L):
    """per column: the smallest distance of a cell to a regime boundary (U = 0, U = -L_theta)"""
    return np.min(np.minimum(np.abs(U), np.abs(U + L)), axis=0)


def assert_close_by_column(plus, minus, h, tan, keep, rtol, what):
    """central difference (plus - minus) / 2h against the tangent: rtol relative to the column's largest tangent value, with a floor of
    1e-9 of the largest over all columns.  (The floor is the rounding of the perturbed states: a response of a few ulps of U over 2h
    -- a cell the seed reaches only through the conductivity of a neighbour -- is all rounding in the difference.)"""
    fd = (plus - minus) / (2.0 * h)
    scale = np.max(np.abs(tan[:, keep]), axis=0)
    floor = 1e-9 * np.max(scale)
    err = np.abs(fd[:, keep] - tan[:, keep])
    assert np.all(err <= rtol * scale[None, :] + floor), (what, float(np.max(err / np.maximum(scale[None, :], 1e-300))))


@pytest.mark.parametrize("bcset", ["T_top+flux_bottom", "gradient_top+flux_bottom"])
def test_tangent_matches_central_differences_of_the_oracle(bcset):
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

    d = device(Nz, Nh, p, U0, sat, bcs)
    d.save_state()
    d.open_tangent()
    for j in range(Nz):
        e = np.zeros((Nz, Nh))
        e[j] = 1.0
        d.restore_state()
        d.set_tangent("internal_energy", e)
        d.step_tangent(DT, n)
        out = []
        for sign in (1.0, -1.0):
            q = oracle_state(Nz, Nh, p, U0 + sign * h * e, sat, bcs)
            for _ in range(n):
                q.timestep(DT)
            out.append({name: q.get(name) for name in TANGENTS})
        for name in TANGENTS:
            assert_close_by_column(out[0][name], out[1][name], h, d.tangent(name), keep, 1e-6, (name, j))


def test_tangent_matches_central_differences_at_size():
    lat, lon = W.columns_from_mask("N145")
    w = W.make_workload("heat", lat, lon, 32)
    n, h = 10, 100.0
    d = W.setup_device(w, steps_per_launch=0)
    d.closure()
    U0 = d.get("internal_energy")
    L = latent(params(), d.get("saturation_water_ice"))
    d.save_state()
    dist = regime_distance(U0, L)
    for _ in range(n):
        d.step(w["dt"], 1, finalize=True)
        dist = np.minimum(dist, regime_distance(d.get("internal_energy"), L))
    keep = dist > 1e3 * h
    assert keep.mean() >= 0.8
    sample = np.flatnonzero(keep)[::25]
    keep = np.zeros_like(keep)
    keep[sample] = True
    d.open_tangent()
    for j in (0, 16, 31):
        e = np.zeros_like(U0)
        e[j] = 1.0
        d.restore_state()
        d.set_tangent("internal_energy", e)
        d.step_tangent(w["dt"], n)
        tan = {name: d.tangent(name) for name in TANGENTS}
        out = []
        for sign in (1.0, -1.0):
            d.restore_state()
            d.set("internal_energy", U0 + sign * h * e)
            d.closure()
            d.step(w["dt"], n, finalize=True)
            out.append({name: d.get(name) for name in TANGENTS})
        for name in TANGENTS:
            assert_close_by_column(out[0][name], out[1][name], h, tan[name], keep, 1e-6, (name, j))


# ---- linearity and locality ---------------------------------------------------------------------------------------------------
def test_tangent_is_exactly_linear():
    Nz, Nh, n = 32, 301, 5
    p = params()
    U, sat = mixed_state(Nz, Nh, p, seed=11)
    d = device(Nz, Nh, p, U, sat, boundary_sets(Nh)["T_top+flux_bottom"])
    d.save_state()
    d.open_tangent()
    rng = np.random.default_rng(5)
    v, w = rng.normal(0.0, 1e3, (Nz, Nh)), rng.normal(0.0, 1e3, (Nz, Nh))

    def tangent_of(seed):
        d.restore_state()
        d.set_tangent("internal_energy", seed)
        d.step_tangent(DT, n)
        return {name: d.tangent(name) for name in TANGENTS}

    tv, t2v, tw, tvw = tangent_of(v), tangent_of(2.0 * v), tangent_of(w), tangent_of(v + w)
    for name in TANGENTS:
        assert np.array_equal(bits(t2v[name]), bits(2.0 * tv[name])), name
        scale = np.max(np.abs(tv[name]) + np.abs(tw[name]), axis=0)
        assert np.all(np.abs(tvw[name] - (tv[name] + tw[name])) <= 1e-12 * scale[None, :]), name


def load_example():
    path = os.path.join(ROOT, "examples", "differentiating_soil_column.py")
    spec = importlib.util.spec_from_file_location("differentiating_soil_column", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_jacobian_is_local_and_the_example_runs():
    ex = load_example()
    J_T, J_U, zs = ex.jacobian(3)
    Nz = J_T.shape[0]
    far = np.abs(np.subtract.outer(np.arange(Nz), np.arange(Nz))) > 3
    assert np.all(J_U[far] == 0.0) and np.all(J_T[far] == 0.0)
    assert np.all(np.diag(J_U) != 0.0)
    J_T, J_U, zs = ex.jacobian()
    assert J_T.shape == (50, 50) and zs.shape == (50,)
    assert np.all(np.isfinite(J_T)) and np.all(np.isfinite(J_U))
    assert np.any(J_T[1] != 0.0)


def test_jvp_leaves_the_integrator_where_run_leaves_it():
    def build():
        grid = trm.ColumnGrid(trm.ExponentialSpacing(N=20), num_columns=3)
        model = trm.SoilModel(grid, initializer=trm.SoilInitializer(energy=trm.QuasiThermalSteadyState(T0=-1.0)))
        bcs = trm.merge_boundary_conditions(trm.PrescribedSurfaceTemperature("T_ub", 1.0))
        return trm.initialize(model, trm.ForwardEuler(), boundary_conditions=bcs)
    a, b = build(), build()
    tan = trm.jvp(a, 1.0, 20)
    trm.run(b, steps=20)
    assert set(tan) == set(TANGENTS) and tan["temperature"].shape == (20, 3)
    for name in STATE:
        assert np.array_equal(bits(a.state.get(name)), bits(b.state.get(name))), name
    assert a.state.clock() == b.state.clock()
    with pytest.raises(ValueError):
        trm.jvp(trm.initialize(build().model, trm.Heun()), 1.0, 1)


# ---- refusals and staleness ---------------------------------------------------------------------------------------------------
def small(Nz=8, Nh=16, p=None, dtype=np.float64):
    grid = trm.ColumnGrid(trm.PrescribedSpacing(dz=list(thickness(Nz))), Nh, dtype=dtype)
    d = trm.DeviceState(grid, p or params())
    d.set("temperature", np.linspace(-2.0, 2.0, Nz))
    d.set_bc("temperature", "top", "value", 1.0)
    d.initialize()
    return d


def test_refusals():
    U, E, S, I = CAPI.TRM_EUNSUPPORTED, CAPI.TRM_EINVAL, CAPI.TRM_ESTALE, CAPI.TRM_OK
    assert code_of(small(dtype=np.float32).open_tangent) == U
    rich = params()
    rich.flow = CAPI.FLOW["richards"]
    assert code_of(small(p=rich).open_tangent) == U
    land = params()
    land.flow, land.seb = CAPI.FLOW["richards"], 1
    assert code_of(small(p=land).open_tangent) == U
    veg = small()
    veg.set_vegetation(CAPI.default_vegetation_params(), "standalone")
    assert code_of(veg.open_tangent) == U
    assert code_of(small(Nz=80).open_tangent) == U
    # no tangent open
    d = small()
    assert code_of(d.step_tangent, DT, 1) == E
    assert code_of(d.tangent_closure) == E
    assert code_of(d.set_tangent, "internal_energy", 1.0) == E
    assert code_of(d.tangent, "temperature") == E
    # refusals of the step: an attached series, an open time average
    d.open_tangent()
    assert code_of(d.step_tangent, DT, 1) == I
    assert d.last_program()["family"] == "column_tangent"
    h = d.open_average("temperature")
    assert code_of(d.step_tangent, DT, 1) == U
    d.close_average(h)
    d.set_bc_series("temperature", "top", "value", [0.0, 1e6], np.ones((2, 16)))
    assert code_of(d.step_tangent, DT, 1) == U
    d.clear_series()
    assert code_of(d.step_tangent, DT, 1) == I
    d.close_tangent()
    assert code_of(d.tangent, "temperature") == E


@pytest.mark.parametrize("change", ["step", "step_heun", "upload_internal_energy", "restore_state", "reset"])
def test_state_changes_make_the_tangent_stale(change):
    S, I = CAPI.TRM_ESTALE, CAPI.TRM_OK
    d = small()
    d.save_state()
    d.open_tangent()
    d.set_tangent("internal_energy", 1.0)
    d.step_tangent(DT, 2)
    assert code_of(d.tangent, "temperature") == I
    {"step": lambda: d.step(DT, 1), "step_heun": lambda: d.step_heun(DT, 1), "restore_state": d.restore_state, "reset": d.reset,
     "upload_internal_energy": lambda: d.set("internal_energy", d.get("internal_energy"))}[change]()
    assert code_of(d.tangent, "temperature") == S
    assert code_of(d.tangent, "liquid_water_fraction") == S
    assert code_of(d.tangent_closure) == S
    assert code_of(d.step_tangent, DT, 1) == S
    assert code_of(d.tangent, "internal_energy") == I
    d.set_tangent("internal_energy", 1.0)
    assert code_of(d.tangent, "temperature") == I
    assert code_of(d.step_tangent, DT, 1) == I
