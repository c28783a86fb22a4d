"""Accuracy of every device path that is not bit-exact -- all of fp32, fp64 van Genuchten, the LandModel's surface energy
balance, the run-time hydraulics (HYD_GENERIC) with every exponent class of make_pow_spec, the vegetation and canopy
processes (standalone VegetationModel and the vegetation-coupled LandModel) -- measured per field against the
wide oracle (tests/accuracy.py): the device may be at most M times as far from the long-double evaluation of the model as the
same-precision oracle is, plus eps(NF), in units of the field's maximum and, for the fields that span decades, per cell.

M IS TO BE MEASURED, NOT CHOSEN: the worst ratio (e_dev - eps) / e_orc over every case, field and both norms of this module
on its first run on an MI355X, doubled (the max-norm of a second, independently rounded evaluation of the same formulas
fluctuates from case to case) and rounded up to a power of two; it may not exceed 8 (accuracy.M_CAP).  A field that needs more
than the cap is a finding about the device arithmetic, not a reason to widen M.

MEASURED on one MI355X (all 75 tests of this module, DESIGN.md section 2, "Measured accuracy"): the worst ratio is 6.59 --
tend_saturation_water_ice of the fp32 run-time hydraulics with vg_n = 4 -- then 1.77 and 1.57 (the same field, bc_lambda = 0.3,
fp64 and fp32) and at most 1.23 everywhere else; the vegetation cases reach 1.20 (hydraulic_conductivity, fp64, 33 levels) and
1.13 on a vegetation field.  Twice 6.59 rounds up to 16, beyond the cap: M = 8, the cap.

Every test prints S_f, e_orc, e_dev, the ratio and the number of cells left out per field before it asserts (pytest -s)."""
import numpy as np
import pytest

import accuracy as A
import workloads as W
import terrarium_jl_amd as trm

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(A.wide_skip_reason() is not None, reason=str(A.wide_skip_reason()))]

M = 8            # min(16, accuracy.M_CAP): see above
assert M <= A.M_CAP


def device_fields(dev, names, sel):
    """{name: array} of the device state on the selected columns; a tendency field the ABI does not serve after this step
    (TRM_ESTALE) is left out and named"""
    out, stale = {}, []
    for n in names:
        try:
            a = dev.get(n)
        except trm.TerrariumHipError as e:
            if n in A.TENDENCIES and e.code == trm._capi.TRM_ESTALE:
                stale.append(n)
                continue
            raise
        out[n] = a[..., sel] if sel is not None else a
    return out, stale


def run_case(case, steps_per_launch):
    w = case.workload()
    orc, ref, names, sel = case.references(w)
    dev = W.setup_device(w, steps_per_launch=steps_per_launch)
    (dev.step_heun if case.heun else dev.step)(w["dt"], case.nsteps, finalize=True)
    assert dev.status() == 0
    devf, stale = device_fields(dev, names, sel)
    dev.close()
    names = [n for n in names if n not in stale]
    for n in names:
        assert devf[n].dtype == case.dtype, n
    rows = A.compare(devf, orc, ref, names, case.dtype, label=f"{case.id} steps_per_launch={steps_per_launch}")
    if stale:
        print(f"  not served after this step: {', '.join(stale)}")
    worst = max([q["ratio_e"] for q in rows] + [q["ratio_r"] for q in rows if q["ratio_r"] is not None])
    print(f"  worst ratio {worst:.3g}")
    bad = A.violations(rows, case.dtype, M)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("steps_per_launch", [0, 1])
@pytest.mark.parametrize("case", A.FP32_PARITY, ids=lambda c: c.id)
def test_fp32_step_accuracy(case, steps_per_launch):
    """the fp32 rows of test_gpu_parity.CASES, Euler and Heun, the library's default launch grouping and one launch per step"""
    run_case(case, steps_per_launch)


@pytest.mark.parametrize("case", A.FP32_DEEP, ids=lambda c: c.id)
def test_fp32_deep_and_wide_columns_accuracy(case):
    """65-128 levels (two per lane) and 250 levels (four per lane) in fp32"""
    run_case(case, 1)


@pytest.mark.parametrize("case", A.FP32_C5, ids=lambda c: c.id)
def test_fp32_c5_shard_accuracy(case):
    """203 125 columns x 64 levels in fp32 (a quarter of one GPU's C5 share), 10 steps, on about 100 sampled columns that the
    oracles run alone with the full grid's dx (as test_c5_shard_fp32_properties does)"""
    run_case(case, 1)


@pytest.mark.parametrize("case", A.FP64_TOL, ids=lambda c: c.id)
def test_fp64_tolerance_paths_accuracy(case):
    """fp64 through generic pow / exp / roots: van Genuchten and the surface energy balance, Euler and Heun, 32 and 96 levels"""
    run_case(case, 1)


@pytest.mark.parametrize("case", A.FP64_N145, ids=lambda c: c.id)
def test_fp64_n145_full_size_accuracy(case):
    """the N145 LandModel at full size on the column sample of test_n145_full_size_against_sampled_oracle"""
    run_case(case, 1)


@pytest.mark.parametrize("case", A.EXPONENTS, ids=lambda c: c.id)
def test_exponent_classes_of_the_runtime_hydraulics_accuracy(case):
    """INT, HALVES, THIRDS and GENERIC exponents of the run-time hydraulics (accuracy.EXPONENT_SETS), fp64 and fp32"""
    run_case(case, 1)


@pytest.mark.parametrize("case", A.VEG_COUPLED, ids=lambda c: c.id)
def test_coupled_vegetation_accuracy(case):
    """The LandModel coupled to VegetationCarbon ("landveg" of tests/workloads.py): k_surface_veg at level pitch 32 (20 levels) and 64
    (33 levels) and its one-thread-per-column form (70 levels, reference-order soil kernels), Euler and Heun (k_heun_average_0d),
    fp64 and fp32, and the dry variants whose cells sit inside the plant-available-water ramp"""
    run_case(case, 1)


@pytest.mark.parametrize("case", A.VEG_STANDALONE, ids=lambda c: c.id)
def test_standalone_vegetation_accuracy(case):
    """k_vegetation on the VegetationModel of tests/test_gpu_vegetation.py:make_pair, 777 columns, against
    VegetationOracle(dtype=longdouble, model=NF): measured after the last of the 30 steps at which the same-precision oracle is
    finite everywhere (accuracy.VegetationCase); after all 30 the device is finite exactly where that oracle is."""
    from test_gpu_vegetation import make_pair
    orc, ref, names, _ = case.references()
    integ, _ = make_pair(case.n, case.dtype, seed=case.seed, stepper=trm.Heun if case.heun else trm.ForwardEuler)
    for _ in range(case.measured):
        trm.timestep(integ)
    devf = {n: integ.state.get(n) for n in names}
    for n in names:
        assert devf[n].dtype == case.dtype, n
    rows = A.compare(devf, orc, ref, names, case.dtype, label=f"{case.id} after {case.measured} steps")
    worst = max(q["ratio_e"] for q in rows)
    print(f"  worst ratio {worst:.3g}")
    bad = A.violations(rows, case.dtype, M)
    assert not bad, "\n".join(bad)
    for _ in range(case.nsteps - case.measured):
        trm.timestep(integ)
    assert trm.current_time(integ) == case.nsteps * case.dt
    for n in names:
        assert np.array_equal(np.isfinite(integ.state.get(n)), np.isfinite(case.final[n])), n
