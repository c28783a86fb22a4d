"""The yardstick of tests/test_gpu_accuracy.py, checked without a GPU: the wide oracle (the model evaluated in long double)
against the fp64 and fp32 oracles on every case of the accuracy suite, the model precision of the wide instance -- of the
soil model and of the vegetation and canopy processes, whose conductance floor sqrt(eps) is the model's -- and the metric
itself: it must reject mutants that the tolerance `tol * max(1, |x|)` of the parity tests accepts."""
import numpy as np
import pytest

import oracle
import accuracy as A

pytestmark = pytest.mark.skipif(A.wide_skip_reason() is not None, reason=str(A.wide_skip_reason()))

# sanity rails against a broken wide build, an order above the measured worst (fp64 5e-14, fp32 8.6e-5 -- the latter
# hydraulic_conductivity under van Genuchten)
RAIL = {np.dtype(np.float64): 1.0e-12, np.dtype(np.float32): 1.0e-3}


@pytest.mark.parametrize("case", A.CASES, ids=lambda c: c.id)
def test_oracle_against_wide_oracle(case):
    """Every case runs its steps with status 0 and finite fields in the same-precision oracle and in the wide one, and the
    same-precision oracle is within the rail of the wide one in units of each field's maximum."""
    w = case.workload()
    orc, ref, names, _ = case.references(w)
    for n in names:
        assert np.all(np.isfinite(orc[n])), n
        assert np.all(np.isfinite(ref[n])), n
        assert ref[n].dtype == np.longdouble
    rows = A.compare(orc, orc, ref, names, case.dtype, label=case.id + " (orc as dev)")
    for q in rows:
        assert np.isfinite(q["e_orc"]) and q["e_orc"] <= RAIL[case.dtype], (q["name"], q["e_orc"])
        if q["r_orc"] is not None:
            assert np.isfinite(q["r_orc"]), q["name"]
        assert q["left_out"] == 0, (q["name"], q["left_out"])      # no regime flip between the oracle and the wide oracle
    assert A.violations(rows, case.dtype, 1) == []                  # the oracle passes its own yardstick with M = 1
    if case in A.VEG_COUPLED:
        # the vegetation fields of the coupled model lose a few eps to rounding and nothing else (measured: at most 8.1 eps in fp64,
        # 13.6 eps in fp32).  A wide instance that does not restate the model -- the conductance floor sqrt(eps) taken from the
        # arithmetic instead of the model put transpiration 9.8e-7 (fp64) and 3.8e-2 (fp32) of its maximum away -- trips this.
        for q in rows:
            if q["name"] in A.VEG_FIELDS:
                assert q["e_orc"] < 64 * A.eps(case.dtype), (q["name"], q["e_orc"])
            if q["name"] in ("transpiration", "evaporation_canopy"):
                # per cell: rounding times the conditioning of the vapour pressure deficit e_sat(T) - e_air, which is floored at
                # 0.1 Pa under an e_sat of up to 3.2e3 Pa (25 C): below 2^15 eps, or the field does not belong in REL_FIELDS
                assert q["r_orc"] is not None and q["r_orc"] < 2.0 ** 15 * A.eps(case.dtype), (q["name"], q["r_orc"])
    if case in A.VEG_STANDALONE:
        assert case.measured == case.nsteps or case.dtype == np.float32, case.measured
        print(f"  measured after {case.measured} of {case.nsteps} steps")


@pytest.mark.parametrize("case", [c for c in A.VEG_COUPLED if c.sat_scale is not None], ids=lambda c: c.id)
def test_dry_vegetation_cases_occupy_the_ramp(case):
    """In the wide reference, at least a quarter of the cells of a dry case have 0 < plant_available_water < 1 after
    initialisation and after every step of the run; the undried workload has none (which is why the dry cases exist)."""
    w = case.workload()
    ref = A.setup_oracle(w, wide=True)
    ref.update_state(False)
    fractions = []
    for n in range(case.nsteps + 1):
        paw = ref.get("plant_available_water")
        fractions.append(float(np.mean((paw > 0) & (paw < 1))))
        if n < case.nsteps:
            (ref.timestep_heun if case.heun else ref.timestep)(w["dt"], True)
    print(f"  {case.id}: cells inside the ramp {min(fractions):.3f} .. {max(fractions):.3f}")
    assert min(fractions) >= 0.25, fractions
    wet = A.Case(case.config, case.hydraulics, case.dtype, case.Nz, case.nsteps, case.columns, heun=case.heun)
    o = A.setup_oracle(wet.workload(), wide=True)
    o.update_state(False)
    paw = o.get("plant_available_water")
    assert not np.any((paw > 0) & (paw < 1))


def _standalone_vegetation(case, model, wide=True, steps=5):
    f, C0, nu0 = case.inputs()
    o = oracle.VegetationOracle(case.n, dtype=np.longdouble if wide else model, model=model)
    for k, v in f.items():
        o.set(k, v)
    o.set("carbon_vegetation", C0)
    o.set("vegetation_area_fraction", nu0)
    for _ in range(steps):
        o.timestep(0.05, True, False)
    return o


def test_wide_vegetation_oracle_restates_the_model_of_its_model_precision():
    """VegetationOracle(dtype=longdouble, model=float32) restates the fp32 MODEL -- parameters, literals and inputs rounded to
    fp32 -- and not the fp64 one: the two wide instances differ by about eps(fp32) on a vegetation field, and the fp32-model one
    agrees with the fp32 oracle to fp32 rounding."""
    case = A.VegetationCase(np.float32, False)
    w32, w64 = _standalone_vegetation(case, np.float32), _standalone_vegetation(case, np.float64)
    o32 = _standalone_vegetation(case, np.float32, wide=False)
    e32 = A.eps(np.float32)
    for name in ("net_assimilation", "canopy_water_conductance", "autotrophic_respiration", "carbon_vegetation"):
        a, b, c = w32.get(name), w64.get(name), o32.get(name).astype(np.longdouble)
        assert a.dtype == b.dtype == np.longdouble
        S = float(np.max(np.abs(a)))
        d_models, d_orc = float(np.max(np.abs(a - b))) / S, float(np.max(np.abs(a - c))) / S
        print(f"  {name:<28} wide(f32 model) - wide(f64 model) {d_models:.3e}   wide(f32 model) - f32 oracle {d_orc:.3e}")
        assert e32 / 64 < d_models < 64 * e32, (name, d_models)      # the models differ by their parameters' and inputs' rounding
        assert d_orc < 64 * e32, (name, d_orc)
    # the Python wrapper refuses a model precision on the plain instances, as Oracle does
    with pytest.raises(AssertionError):
        oracle.VegetationOracle(4, dtype=np.float64, model=np.float32)


@pytest.mark.parametrize("model", [np.float32, np.float64])
def test_conductance_floor_of_the_wide_oracle_is_the_models(model):
    """canopy_evapotranspiration.jl:53 floors the canopy conductance at sqrt(eps(NF)) of the MODEL's number format.  Dark columns
    (no shortwave: no assimilation) over soil at the wilting point (soil moisture limiting factor 0) have conductance 0, so the
    wide transpiration is dq / (ra + 1 / sqrt(eps(model))) to long-double rounding -- with dq recovered from the canopy
    evaporation f_can dq / ra of the same evaluation -- and not dq / (ra + 1 / sqrt(eps(long double)))."""
    n, L = 6, np.longdouble
    thickness = np.array([0.05, 0.1, 0.2, 0.4])
    p = oracle.default_params(flow=1, seb=1, swrc=1, unsat_k=1, vg_alpha=2.0, vg_n=2.0)
    o = oracle.Oracle(n, thickness, p, dtype=L, model=model)
    o.enable_vegetation()
    wind = np.linspace(0.5, 4.0, n)
    o.set("temperature", np.full((4, n), 5.0)); o.set("saturation_water_ice", np.full((4, n), 0.05))
    o.set("skin_temperature", np.linspace(4.0, 9.0, n)); o.set("carbon_vegetation", np.linspace(1.0, 2.0, n))
    o.set("canopy_water", np.linspace(1.0e-5, 6.0e-5, n)); o.set("SAI", np.full(n, 0.5)); o.set("windspeed", wind)
    o.set("surface_shortwave_down", np.zeros(n))
    o.initialize()
    o.update_state(False)
    assert np.all(o.get("soil_moisture_limiting_factor") == 0) and np.all(o.get("canopy_water_conductance") == 0)
    transp, E_can, f_can = o.get("transpiration"), o.get("evaporation_canopy"), o.get("saturation_canopy_water")
    assert np.all(f_can > 0) and np.all(transp > 0)
    ra = 1 / (L(model(p.C_h)) * np.asarray(wind, dtype=model).astype(L))
    floor = L(np.sqrt(model(np.finfo(model).eps)))
    expected = (E_can * ra / f_can) / (ra + 1 / floor)
    err = float(np.max(np.abs(transp - expected) / expected))
    print(f"  model {np.dtype(model).name}: floor {float(floor):.4e}, transpiration against dq / (ra + 1 / floor): {err:.2e} relative")
    assert err <= 16 * float(np.finfo(L).eps), err
    wrong = (E_can * ra / f_can) / (ra + 1 / np.sqrt(np.finfo(L).eps))
    assert np.all(transp > 40 * wrong)              # the arithmetic's epsilon: 45 (fp64 model) and 1e6 (fp32 model) times smaller
    # the scalar entry point of the known-answer tests
    name = "transpiration_wide_f32_model" if model == np.float32 else "transpiration_wide_f64_model"
    assert oracle.veg_scalar(name, 1.0e-3, 100.0, 0.0) == pytest.approx(1.0e-3 / (100.0 + 1.0 / float(floor)), rel=1e-15)


def test_wide_oracle_restates_the_model_of_its_model_precision():
    """The wide instance with the fp32 model restates the fp32 MODEL (its rounded parameters and grid), not the fp64 one: it
    stays within fp32 rounding of the fp32 oracle, and the two wide instances differ from each other by the parameters'
    rounding."""
    case = A.Case("land", "vg", np.float32, 32, 20, A.N72(40))
    w = case.workload()
    orc32, ref32, names, _ = case.references(w)
    w64 = dict(w, dtype=np.dtype(np.float64))
    ref64 = A.setup_oracle(w64, wide=True)
    A.run_oracle(ref64, w["dt"], case.nsteps)
    t32, t64 = ref32["temperature"], ref64.get("temperature")
    d_models = float(np.max(np.abs(t32 - t64)))
    d_orc = float(np.max(np.abs(orc32["temperature"].astype(np.longdouble) - t32)))
    assert 0 < d_models < 1e-4 and d_orc < 1e-3, (d_models, d_orc)


@pytest.mark.parametrize("dtype,factor,tol", [(np.float32, 1.0 + 1.0e-2, 1.0e-4), (np.float64, 1.0 + 1.0e-6, 1.0e-10)])
def test_the_metric_rejects_what_the_tolerance_accepts(dtype, factor, tol):
    """Mutants of the same-precision oracle's own output -- hydraulic_conductivity, evaporation_ground and infiltration scaled
    by 1 + 1e-2 (fp32) / 1 + 1e-6 (fp64; 1 + 5e-7 for the evaporation, see below) -- pass `|x - orc| <= tol * max(1, |orc|)` and fail the metric with M = 8."""
    case = A.Case("land", "vg", dtype, 32 if dtype == np.float64 else 64, 50, A.N72(333))
    w = case.workload()
    orc, ref, names, _ = case.references(w)
    for name in ("hydraulic_conductivity", "evaporation_ground", "infiltration"):
        assert np.any(orc[name] != 0), name
        mutant = dict(orc)
        f = factor
        if name == "evaporation_ground" and dtype == np.float64:
            # the field's maximum here is 1.19e-4, so the 1 + 1e-6 mutant reads 1.19e-10 in the old metric: a hair ABOVE its
            # 1e-10.  Half the mutation is inside the old tolerance, and harder for the new metric to reject.
            assert 1.0e-10 < A.old_metric(orc[name] * factor, orc[name]) < 1.3e-10
            f = 1.0 + 5.0e-7
        mutant[name] = (orc[name].astype(np.longdouble) * np.longdouble(f)).astype(dtype)
        assert A.old_metric(mutant[name], orc[name]) <= tol, name                     # the old assertion accepts it
        rows = A.compare(mutant, orc, ref, names, dtype, label=f"mutant {name}")
        bad = A.violations(rows, dtype, A.M_CAP)
        assert bad and all(b.startswith(name + ":") for b in bad), (name, bad)        # the new one rejects it, and it alone
    assert A.violations(A.compare(orc, orc, ref, names, dtype, label="unmutated"), dtype, A.M_CAP) == []


def test_model_epsilon_of_the_wide_oracle():
    """safediv adds eps(NF) to the denominator (utils.jl:25): that epsilon is the model's, not the arithmetic's.  On a tiny
    denominator the fp32 model gives ~1 / eps(Float32), the fp64 model ~1 / eps(Float64); neither gives 1 / eps(long double)."""
    x, y = 1.0, 1.0e-30
    a32, a64 = oracle.safediv_wide(x, y, np.float32), oracle.safediv_wide(x, y, np.float64)
    assert a32 != a64
    assert abs(float(a32) * np.finfo(np.float32).eps - 1.0) < 1e-6
    assert abs(float(a64) * np.finfo(np.float64).eps - 1.0) < 1e-6
    assert float(a64) == pytest.approx(oracle.scalar("safediv", x, y), rel=1e-15)
    # and through the model's closure: a cell with a vanishing latent content (saturation 1e-12: L theta ~ 1.6e-4 J/m^3), partly
    # frozen -- liquid fraction 1 - U / (-(L theta) + eps)
    thickness = np.array([0.1, 0.2])
    out = {}
    for model in (np.float32, np.float64):
        o = oracle.Oracle(1, thickness, oracle.default_params(), dtype=np.longdouble, model=model)
        o.set("saturation_water_ice", np.full((2, 1), 1.0e-12))
        o.set("internal_energy", np.full((2, 1), -1.0e-5))
        o.closure()
        out[model] = o.get("liquid_water_fraction")[0, 0]
    assert 0 < out[np.float32] < 1 and 0 < out[np.float64] < 1
    assert abs(out[np.float32] - out[np.float64]) > 1e-5          # eps(Float32) against L theta ~ 1.6e-4: a 7e-4 relative shift of U / (L theta)


def test_float_and_double_instances_ignore_the_model_argument():
    with pytest.raises(AssertionError):
        oracle.Oracle(1, np.array([0.1, 0.2]), dtype=np.float64, model=np.float32)


def test_regime_flips_zero_scale_and_nonfinite_cells():
    """The bookkeeping of the metric on made-up fields: a flipped cell is left out and counted, more than 0.1 % of a field
    left out fails, a field whose reference is identically zero must be zero, finite and non-finite cells must coincide."""
    Nz, Nh = 10, 400
    rng = np.random.default_rng(3)
    ref = dict(liquid_water_fraction=np.ones((Nz, Nh), dtype=np.longdouble),
               saturation_water_ice=np.full((Nz, Nh), 0.5, dtype=np.longdouble),
               temperature=rng.uniform(1, 2, (Nz, Nh)).astype(np.longdouble),
               surface_excess_water=np.zeros(Nh, dtype=np.longdouble))
    names = list(ref)
    orc = {k: v.astype(np.float64) for k, v in ref.items()}
    same = lambda: {k: v.copy() for k, v in orc.items()}
    assert A.violations(A.compare(same(), orc, ref, names, np.float64), np.float64, 1) == []
    dev = same()
    dev["liquid_water_fraction"][3, 7] = 0.5            # one cell freezes on the device only: an O(1) difference there
    dev["temperature"][3, 7] = 0.0
    rows = A.compare(dev, orc, ref, names, np.float64)
    assert {q["name"]: q["left_out"] for q in rows} == dict(liquid_water_fraction=1, saturation_water_ice=1, temperature=1, surface_excess_water=1)
    bad = A.violations(rows, np.float64, 1)              # 1 of 4000 cells passes; 1 of 400 columns (the 2-D field) is too many
    assert len(bad) == 1 and bad[0].startswith("surface_excess_water:") and "left out" in bad[0], bad
    assert any("temperature: e_dev" in b for b in A.violations(A.compare(dev, orc, ref, names, np.float64, exclude_flips=False), np.float64, 1))
    for k in range(5):                                   # five cells of 4000: more than 0.1 %
        dev["liquid_water_fraction"][k, 9] = 0.5
    assert any(b.startswith("temperature:") and "left out" in b for b in A.violations(A.compare(dev, orc, ref, names, np.float64), np.float64, 1))
    dev = same()
    dev["surface_excess_water"][5] = 1.0e-300
    assert any("identically zero" in b for b in A.violations(A.compare(dev, orc, ref, names, np.float64), np.float64, A.M_CAP))
    dev = same()
    dev["temperature"][0, 0] = np.nan
    assert any("finite on one side" in b for b in A.violations(A.compare(dev, orc, ref, names, np.float64), np.float64, A.M_CAP))
