"""Plant available water and the soil moisture limiting factor on the device at the edges of the block layout of
k_plant_available_water_block / k_surface_veg (64 columns per workgroup, clamped loads, LDS rows of pitch NZP + 1, a partly
filled last workgroup, Nz = NZP) and of the one-thread-per-column kernels beyond 64 levels, bit for bit against the numpy
restatement of tests/vegetation_edges.py (pinned to the oracle in tests/test_vegetation_edges_host.py) with inputs that differ
in every cell -- fp64 and fp32: the quotients are correctly rounded (div_const) and the column sum runs in the sequential
bottom-up order of Oceananigans' Integral, so nothing here is a matter of tolerance.  Then the coupled LandModel at the same
shapes: the fused step against the reference-order kernels, Euler and Heun, bit for bit.

Coupled depths: all of vegetation_edges.DEPTHS (the library refuses none of them for the coupled model)."""
import numpy as np
import pytest

import oracle
import terrarium_jl_amd as trm
import vegetation_edges as E
from test_gpu_coupled_vegetation import CANOPY_AUX, PROG, SURFACE, VEG_AUX, land_with_vegetation

pytestmark = pytest.mark.gpu

DT = 0.5     # as tests/test_gpu_coupled_vegetation.py:make_pair


def grid_of(Nz, Nh, dtype):
    return trm.ColumnGrid(trm.PrescribedSpacing(dz=list(E.thickness(Nz))), Nh, dtype=dtype)


def assert_bits(a, b, what):
    a, b = np.atleast_1d(a), np.atleast_1d(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    differ = E.bits(a) != E.bits(b)
    assert not differ.any(), (what, int(differ.sum()), [tuple(int(x) for x in ix) for ix in np.argwhere(differ)[:5]])


def device_grid(st, dtype):
    """(root_fraction [Nz][Nh], dz [Nz]) of the device's own grid, in dtype"""
    dz = st._grid_arrays()["dzc"]
    assert np.array_equal(dz.astype(dtype).astype(np.float64), dz)
    return st.root_fraction, dz.astype(dtype)


@pytest.mark.parametrize("case", E.CASES, ids=E.case_id)
def test_standalone_plant_available_water_bit_for_bit(case):
    """k_plant_available_water_block<32>, <64> and k_plant_available_water (Nz > 64: reads the per-cell root_fraction field)"""
    Nz, Nh, dtype = case
    sat, liq = E.inputs(*case)
    st = trm.DeviceState(grid_of(*case), trm._capi.default_params())
    st.set_vegetation(trm._capi.default_vegetation_params(), "standalone")
    rf, dz = device_grid(st, dtype)
    o = oracle.Oracle(Nh, E.thickness(Nz), dtype=dtype)
    o.enable_vegetation()
    assert np.allclose(rf, o.get("root_fraction"), rtol=1e-14, atol=0)
    assert np.array_equal(rf, np.broadcast_to(rf[:, :1], rf.shape))          # static: the same table in every column
    st.set("saturation_water_ice", sat)
    st.set("liquid_water_fraction", liq)
    st.compute_plant_available_water()
    paw, _, smlf = E.restate(sat, liq, rf, dz, dtype)
    assert_bits(st.plant_available_water, paw, "plant_available_water")
    assert_bits(st.soil_moisture_limiting_factor, smlf, "soil_moisture_limiting_factor")
    assert np.array_equal(st.get("saturation_water_ice"), sat) and np.array_equal(st.get("liquid_water_fraction"), liq)
    st.close()


def coupled(case, stepper, unfused=False):
    Nz, Nh, dtype = case
    sat, T = E.coupled_initial_state(*case)
    rng = np.random.default_rng([E.SEED + 2, Nz, Nh])
    inits = dict(temperature=T, saturation_water_ice=sat, carbon_vegetation=rng.uniform(1.0, 2.0, Nh),
                 vegetation_area_fraction=rng.uniform(0.05, 0.9, Nh), canopy_water=rng.uniform(0.0, 1.0e-4, Nh))
    inputs = dict(SAI=rng.uniform(0.0, 1.0, Nh), rainfall=rng.uniform(0.0, 2.0e-7, Nh), air_temperature=rng.uniform(2.0, 20.0, Nh),
                  specific_humidity=rng.uniform(1.0e-3, 5.0e-3, Nh), windspeed=rng.uniform(0.0, 4.0, Nh), CO2=rng.uniform(300.0, 500.0, Nh),
                  daily_leaf_respiration=rng.uniform(0.0, 1e-6, Nh))
    integ = trm.initialize(land_with_vegetation(grid_of(*case)), stepper(dt=DT), initializers=inits, inputs=inputs)
    if unfused:
        integ.state.set_option("step_kernel", "unfused")
    return integ


@pytest.mark.parametrize("case", E.CASES, ids=E.case_id)
def test_coupled_surface_kernel_bit_for_bit(case):
    """The two fields k_surface_veg produces in update_state! equal the restatement of the state's own saturation and liquid
    fraction, read back after the call."""
    Nz, Nh, dtype = case
    st = coupled(case, trm.ForwardEuler).state
    st.update_state(True)
    sat, liq = st.get("saturation_water_ice"), st.get("liquid_water_fraction")
    assert np.any(liq == 0) or Nz * Nh < 31
    rf, dz = device_grid(st, dtype)
    paw, terms, smlf = E.restate(sat, liq, rf, dz, dtype)
    assert E.input_conditions(paw, terms, smlf) == []         # the state the kernel saw still occupies the ramp
    assert_bits(st.plant_available_water, paw, "plant_available_water")
    assert_bits(st.soil_moisture_limiting_factor, smlf, "soil_moisture_limiting_factor")
    assert st.status() == 0
    st.close()


@pytest.mark.parametrize("stepper", [trm.ForwardEuler, trm.Heun], ids=["euler", "heun"])
@pytest.mark.parametrize("case", E.CASES, ids=E.case_id)
def test_coupled_fused_equals_reference_order_kernels(case, stepper):
    """4 steps of the fused launches against the reference-order kernels (step_kernel = "unfused"), every field of PROG + SURFACE +
    VEG_AUX + CANOPY_AUX bit for bit; Heun covers k_heun_average_0d and the stage evaluation of k_surface_veg at a tail workgroup."""
    a, b = coupled(case, stepper), coupled(case, stepper, unfused=True)
    for _ in range(4):
        trm.timestep(a)
        trm.timestep(b)
    assert a.state.status() == b.state.status() == 0
    for n in PROG + SURFACE + VEG_AUX + CANOPY_AUX:
        x, y = a.state.get(n), b.state.get(n)
        assert np.all(np.isfinite(x)), n
        assert_bits(x, y, n)
    assert trm.current_time(a) == trm.current_time(b) == 4 * DT
    a.state.close()
    b.state.close()
