"""The reference of tests/test_gpu_vegetation_edges.py, checked without a GPU: the numpy restatement of plant available water
and its column sum (tests/vegetation_edges.py) equals the coupled oracle bit for bit in fp64 and in fp32 at every shape of the
edge suite, and the seeded inputs satisfy the conditions under which a wrong column or level index cannot hide."""
import functools

import numpy as np
import pytest

import oracle
import vegetation_edges as E


@functools.lru_cache(maxsize=None)
def oracle_side(Nz, Nh, dtype):
    """(oracle plant_available_water, oracle soil_moisture_limiting_factor, root_fraction, dz) of a LandModel oracle with vegetation whose
    soil state is the case's saturation and liquid fraction (compute_auxiliary! reads both as they are)"""
    sat, liq = E.inputs(Nz, Nh, dtype)
    o = oracle.Oracle(Nh, E.thickness(Nz), oracle.default_params(flow=1, seb=1, swrc=1, unsat_k=1, vg_alpha=2.0, vg_n=2.0), dtype=dtype)
    o.enable_vegetation()
    o.set("saturation_water_ice", sat)
    o.set("liquid_water_fraction", liq)
    o.compute_auxiliary()
    assert np.array_equal(o.get("saturation_water_ice"), sat) and np.array_equal(o.get("liquid_water_fraction"), liq)
    return o.get("plant_available_water"), o.get("soil_moisture_limiting_factor"), o.get("root_fraction"), o.grid()["dzc"].astype(dtype)


@pytest.mark.parametrize("case", E.CASES, ids=E.case_id)
def test_restatement_equals_the_oracle_bit_for_bit(case):
    Nz, Nh, dtype = case
    sat, liq = E.inputs(*case)
    paw_o, smlf_o, rf, dz = oracle_side(*case)
    assert paw_o.dtype == smlf_o.dtype == rf.dtype == np.dtype(dtype)
    assert np.array_equal(dz.astype(np.float64), oracle.Oracle(1, E.thickness(Nz), dtype=dtype).grid()["dzc"])   # dz is exact in dtype
    paw, terms, smlf = E.restate(sat, liq, rf, dz, dtype)
    assert np.array_equal(E.bits(paw), E.bits(paw_o))
    assert np.array_equal(E.bits(smlf), E.bits(np.atleast_1d(smlf_o)))
    # the per-level table is the per-cell field's column
    assert np.array_equal(E.bits(E.restate(sat, liq, rf[:, 0].copy(), dz, dtype)[2]), E.bits(smlf))


@pytest.mark.parametrize("case", E.CASES, ids=E.case_id)
def test_inputs_make_a_wrong_index_visible(case):
    Nz, Nh, dtype = case
    sat, liq = E.inputs(*case)
    assert sat.dtype == liq.dtype == np.dtype(dtype) and sat.shape == liq.shape == (Nz, Nh)
    assert sat.min() >= 0.05 and sat.max() <= 1 and liq.min() >= 0 and liq.max() <= 1
    if sat.size >= 1000:
        f1, f0 = float(np.mean(liq == 1)), float(np.mean(liq == 0))
        assert 0.6 < f1 < 0.8 and 0.05 < f0 < 0.15 and 0.1 < 1 - f1 - f0 < 0.3, (f1, f0)
    _, _, rf, dz = oracle_side(*case)
    assert np.all(rf > 0) and np.all(np.abs(rf) >= np.finfo(dtype).tiny)            # no subnormal root fraction
    assert np.unique(dz).size == Nz
    paw, terms, smlf = E.restate(sat, liq, rf, dz, dtype)
    assert E.input_conditions(paw, terms, smlf) == []
    # what a wrong index would give differs: the next column's cells, and a sum that stops one level short
    if Nh > 1:
        assert np.all(E.restate(np.roll(sat, -1, axis=1), np.roll(liq, -1, axis=1), rf, dz, dtype)[2] != smlf)
    short = np.zeros(Nh, dtype=dtype)
    for k in range(Nz - 1):
        short = short + terms[k]
    assert np.all(short != smlf)


def test_the_coupled_initial_state_occupies_the_ramp():
    """The coupled cases draw their saturation the same way: with the liquid fraction the model derives from the temperature (1 at
    or above 0 degC, 0 below: temperature_to_energy of initialize!) at least a quarter of the cells start inside the ramp."""
    for case in E.CASES:
        Nz, Nh, dtype = case
        sat, T = E.coupled_initial_state(*case)
        liq = (T >= 0).astype(dtype)
        _, _, rf, dz = oracle_side(*case)
        paw, terms, smlf = E.restate(sat, liq, rf, dz, dtype)
        assert E.input_conditions(paw, terms, smlf) == [], E.case_id(case)
