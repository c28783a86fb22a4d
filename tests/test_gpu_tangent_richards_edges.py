"""Heat + Richards tangents at the edges of the lane layouts, value by value against an exact Jacobian (tests/linearised_richards.py).

The cases are those of tests/richards_cases.py: Nz in {2, 3, 31, 32, 33, 63, 64} x 13 columns and one column at Nz = 2 and 64, the
three hydraulics instances (default, vg_n2, generic with van Genuchten at n = 1.7), two boundary sets (a temperature Value on top with
fluxes at the bottom; an infiltration flux on the top saturation), and the repair cases at Nz = 3 and 33.  Six steps of 60 s under
steps_per_launch = 4: launches of 4 and 2.

The five tangents of a dense (dU, dsat) seed and of one-hot seeds in U and in sat on levels 0, Nz - 1, 31 and 32 are compared cell by
cell with the extended-precision Jacobian of the restatement: |dev - ref| / S <= 8 x e_ref of the case, S = sum |J_80| |v|, e_ref the same
normalised difference between the float64 and the extended-precision evaluation of the restatement itself -- computed on the CPU, so no
figure of the device enters the bound; 8 is what the project grants a second evaluation order.  A bound above BROKEN is refused as a
broken measurement.  Where S is zero the device's value must be 0.0.  Columns are compared unless the branch mask drops them
(linearised_richards.kept_columns); test_linearised_richards_host.py proves on the CPU that no case loses more than two of 13.

With it: after step_tangent every field, the per-column water fields and the status are those of a twin stepped with trm_step, bit for
bit, and the launch reports the family column_tangent_richards with the case's hydraulics and layout."""
import numpy as np
import pytest

import richards_cases as RC
import terrarium_jl_amd as trm
from richards_cases import DT, DZ, SPL, STEPS, case_id, reference

pytestmark = pytest.mark.gpu

# The ceiling on a case's bound 8 x e_ref.  The largest e_ref test_linearised_richards_host.py measures over the cases is 3.9e-12
# (MEASURED_LARGEST_E_REF there); a case whose e_ref is more than four times that is no measurement of fp64 rounding.
BROKEN = RC.FACTOR * 4.0 * 3.9e-12
TANGENTS = ("internal_energy", "saturation", "temperature", "liquid_water_fraction", "pressure_head")
# every array the finalizing trm_step stores on a Richards context
STATE = ("internal_energy", "saturation_water_ice", "temperature", "liquid_water_fraction", "pressure_head", "hydraulic_conductivity",
         "tend_internal_energy", "tend_saturation_water_ice", "water_table", "surface_excess_water", "tend_surface_excess_water")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def device(case, steps_per_launch=SPL, richards_option=1):
    Nz, Nh = case[0], case[1]
    p, U0, sat, bcs, _ = RC.inputs(case)
    d = trm.DeviceState(trm.ColumnGrid(trm.PrescribedSpacing(dz=[DZ] * Nz), Nh), p)
    d.set_option("steps_per_launch", steps_per_launch)
    d.set_option("derivative_richards", richards_option)
    d.set("saturation_water_ice", sat)
    d.set("internal_energy", U0)
    for (var, side), (kind, value) in bcs.items():
        d.set_bc(var, side, kind, value)
    d.closure()
    d.save_state()
    return d


def stepped_twin(case):
    """the state trm_step leaves, under the library's own choice of program"""
    b = device(case, steps_per_launch=0, richards_option=0)
    b.step(DT, STEPS, finalize=True)
    return {name: bits(b.get(name)) for name in STATE}, b.status(), b.clock()


def tangents(d, seed):
    """the five tangents stacked, of the saved state under the seed [2 Nz][Nh] = (dU, dsat)"""
    Nz = seed.shape[0] // 2
    d.restore_state()
    d.open_tangent()
    d.set_tangent("internal_energy", seed[:Nz])
    d.set_tangent("saturation", seed[Nz:])
    d.step_tangent(DT, STEPS)
    return np.stack([d.tangent(x) for x in TANGENTS])


@pytest.mark.parametrize("case", RC.CASES, ids=case_id)
def test_tangents_match_the_exact_jacobian(case):
    ref = reference(case)
    bound = ref.bound(BROKEN)
    d = device(case)
    figures = {}
    for label, seed in RC.contractions(case).items():
        t = tangents(d, seed)
        if label == "dense":      # the primal is trm_step's, whatever the seed
            state, status, clock = stepped_twin(case)
            for name in STATE:
                assert np.array_equal(bits(d.get(name)), state[name]), (case_id(case), name)
            assert d.status() == status and d.clock() == clock
            prog = d.last_program()
            assert prog["family"] == "column_tangent_richards" and prog["hydraulics"] == case[2], (case_id(case), prog)
            assert prog["lanes_per_column"] == (32 if case[0] <= 32 else 64), (case_id(case), prog)
        figures[label] = ref.error(label, t)
    worst = max(figures.values())
    print(f"{case_id(case)}: e_ref = {ref.e_ref:.3e}, bound = {bound:.3e}, device = {worst:.3e}, kept {int(ref.keep.sum())}/{ref.keep.size}")
    for label, err in figures.items():
        print(f"    {label}: device = {err:.3e}, e_ref = {ref.parts[label]:.3e}")
    over = {label: err for label, err in figures.items() if not err <= bound}
    assert not over, (case_id(case), f"bound {bound:.3e}", over)
