"""Hydraulic-parameter gradients of the heat + Richards adjoint at the edges of the lane layouts, value by value against the parameter
columns of an exact Jacobian (tests/linearised_richards_params.py).

The cases are those of tests/richards_cases.py (test_gpu_tangent_richards_edges.py describes them) with the cotangents of
tests/richards_adjoint_cases.py: Nz in {2, 3, 31, 32, 33, 63, 64} x 13 columns and one column at Nz = 2 and 64, the three hydraulics
instances, two boundary sets, and the repair cases at Nz = 3 and 33.  Six steps of 60 s under steps_per_launch = 4: backward launches of
4 and 2, then the reduction.

For every cotangent all seven per-column gradients are compared with g_ref = J_p^T w on the kept columns: |dev - ref| / S <= the case's
bound, S = sum |J_p| |w|, the bound 8 x the e_ref pooled over the non-repair cases of the same Nz and hydraulics (a repair case: its own)
-- computed on the CPU, so no figure of the device enters it; test_richards_params_host.py holds every bound under the ceiling.  Where
S is zero the device's value must be 0.0: the parameters the case's hydraulics never read, and every gradient of a cotangent that
reaches nothing.  In the repair cases the pressure-head cotangent is zero in the columns whose final state holds a cell at zero
saturation.

With it: gU, gsat and the eleven state arrays are bit for bit those of a twin that runs with the option at 0, and the backward launch
reports the family column_adjoint_richards with hydraulic_parameter_gradient and the case's hydraulics and layout."""
import numpy as np
import pytest

import linearised_richards_params as LP
import terrarium_jl_amd as trm
from linearised_richards_params import DT, STEPS, case_id
from test_gpu_adjoint_richards_edges import adjoint_device, record, sweep
from test_gpu_tangent_richards_edges import STATE, bits

pytestmark = pytest.mark.gpu

PARAMS = tuple(trm._capi.HYDRAULIC_PARAMS)


def params_device(case, steps_per_launch=LP.SPL):
    d = adjoint_device(case, steps_per_launch=steps_per_launch)
    d.set_option("derivative_richards_params", 1)
    return d


def param_sweep(d, w, schedule=((DT, STEPS),)):
    """((gU, gsat), {name: [Nh]}) of the saved state taped under the schedule, with the parameter gradients open"""
    record(d, schedule)
    d.open_param_gradient()
    state = sweep(d, w)
    return state, {name: d.param_gradient(name) for name in PARAMS}


@pytest.mark.parametrize("case", LP.CASES, ids=case_id)
def test_parameter_gradients_match_the_exact_jacobian(case):
    ref = LP.reference(case)
    bound = LP.bound(case)
    d, twin = params_device(case), adjoint_device(case)
    figures = {}
    for label, w in LP.cotangents(case).items():
        (gU, gsat), grads = param_sweep(d, w)
        if label == "dense":
            prog = d.last_program()
            assert prog["family"] == "column_adjoint_richards" and prog["hydraulic_parameter_gradient"] is True, (case_id(case), prog)
            assert prog["hydraulics"] == case[2] and prog["lanes_per_column"] == (32 if case[0] <= 32 else 64), (case_id(case), prog)
        # the state gradients are the bits of the sweep without the parameter gradient, and so is the state
        record(twin)
        tU, tsat = sweep(twin, w)
        assert np.array_equal(bits(gU), bits(tU)) and np.array_equal(bits(gsat), bits(tsat)), (case_id(case), label)
        if label == "dense":
            assert "hydraulic_parameter_gradient" not in twin.last_program()
            for name in STATE:
                assert np.array_equal(bits(d.get(name)), bits(twin.get(name))), (case_id(case), name)
            assert d.status() == twin.status() and d.clock() == twin.clock()
        figures[label] = ref.error(label, grads)
    worst = max(figures.values())
    print(f"{case_id(case)}: e_ref = {ref.e_ref:.3e}, bound = {bound:.3e}, device = {worst:.3e}, ratio = {worst / bound:.3f}, kept {int(ref.keep.sum())}/{ref.keep.size}")
    for label, err in figures.items():
        print(f"    {label}: device = {err:.3e}, e_ref = {ref.parts[label]:.3e}")
    over = {label: err for label, err in figures.items() if not err <= bound}
    assert not over, (case_id(case), f"bound {bound:.3e}", over)
