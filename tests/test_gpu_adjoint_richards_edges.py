"""Heat + Richards gradients at the edges of the lane layouts, value by value against an exact Jacobian (tests/linearised_richards.py).

The cases are those of tests/richards_cases.py (test_gpu_tangent_richards_edges.py describes them): Nz in {2, 3, 31, 32, 33, 63, 64} x 13
columns and one column at Nz = 2 and 64, the three hydraulics instances, two boundary sets, and the repair cases at Nz = 3 and 33.  Six
steps of 60 s under steps_per_launch = 4: record and backward launches of 4 and 2.

gU = dL/dU_0 and gsat = dL/dsat_0 of a dense cotangent on the five final fields and of one-hot cotangents on each of them at levels 0,
Nz - 1, 31 and 32 are compared cell by cell with J_80^T w of the restatement's extended-precision Jacobian
(tests/richards_adjoint_cases.py): |dev - ref| / S <= 8 x e_ref of the case, S = sum |J_80| |w|, e_ref the same normalised difference
between the float64 and the extended-precision evaluation of the restatement itself -- computed on the CPU, so no figure of the device
enters the bound.  A bound above BROKEN is refused as a broken measurement.  Where S is zero the device's value must be 0.0.  Columns are
compared unless the branch mask drops them; test_richards_adjoint_host.py proves on the CPU that no case loses more than two of 13.

With it: after step_record every field, the per-column water fields, the status and the clock are those of a twin stepped with trm_step,
bit for bit, and both launches report the family column_adjoint_richards with the case's hydraulics and layout."""
import numpy as np
import pytest

import richards_adjoint_cases as RA
import terrarium_jl_amd as trm
from richards_adjoint_cases import DT, STEPS, case_id, reference
from test_gpu_tangent_richards_edges import STATE, bits, device, stepped_twin

pytestmark = pytest.mark.gpu

COTANGENTS = tuple(trm._capi.ADJOINT)        # internal_energy, temperature, liquid_water_fraction, saturation, pressure_head
# the cotangent fields in the order of linearised_richards.FIELDS, the order of a cotangent's first axis
BY_FIELD = ("internal_energy", "saturation", "temperature", "liquid_water_fraction", "pressure_head")


def adjoint_device(case, steps_per_launch=RA.SPL):
    d = device(case, steps_per_launch=steps_per_launch, richards_option=0)
    d.set_option("derivative_richards_adjoint", 1)
    return d


def record(d, schedule=((DT, STEPS),)):
    """the saved state taped under the schedule [(dt, steps), ...], one step_record call each, on a fresh tape"""
    d.restore_state()
    d.open_adjoint(sum(steps for _, steps in schedule))
    for dt, steps in schedule:
        d.step_record(dt, steps)


def sweep(d, w):
    """(gU, gsat) of the taped run under the cotangent w [5][Nz][Nh]"""
    for name, field in zip(BY_FIELD, w):
        d.set_cotangent(name, field)
    d.adjoint_backward()
    return d.cotangent("internal_energy"), d.cotangent("saturation")


def gradients(d, w, schedule=((DT, STEPS),)):
    record(d, schedule)
    return sweep(d, w)


@pytest.mark.parametrize("case", RA.CASES, ids=case_id)
def test_gradients_match_the_exact_jacobian(case):
    ref = reference(case)
    bound = ref.bound(RA.BROKEN)
    d = adjoint_device(case)
    figures = {}
    for label, w in RA.cotangents(case).items():
        record(d)
        if label == "dense":      # the primal is trm_step's, whatever the cotangent
            state, status, clock = stepped_twin(case)
            for name in STATE:
                assert np.array_equal(bits(d.get(name)), state[name]), (case_id(case), name)
            assert d.status() == status and d.clock() == clock
            programs = [d.last_program()]
        gU, gsat = sweep(d, w)
        if label == "dense":
            programs.append(d.last_program())
            for prog in programs:
                assert prog["family"] == "column_adjoint_richards" and prog["hydraulics"] == case[2], (case_id(case), prog)
                assert prog["lanes_per_column"] == (32 if case[0] <= 32 else 64), (case_id(case), prog)
            for name in ("temperature", "liquid_water_fraction", "pressure_head"):
                assert np.all(d.cotangent(name) == 0.0), name
        figures[label] = ref.error(label, gU, gsat)
    worst = max(figures.values())
    print(f"{case_id(case)}: e_ref = {ref.e_ref:.3e}, bound = {bound:.3e}, device = {worst:.3e}, ratio = {worst / bound:.3f}, kept {int(ref.keep.sum())}/{ref.keep.size}")
    for label, err in figures.items():
        print(f"    {label}: device = {err:.3e}, e_ref = {ref.parts[label]:.3e}")
    over = {label: err for label, err in figures.items() if not err <= bound}
    assert not over, (case_id(case), f"bound {bound:.3e}", over)
