"""Thermal-parameter derivatives of runs driven by a boundary time series (TRM_OPT_DERIVATIVE_SERIES_PARAMS) at the edges of the lane
layouts, value by value against the exact Jacobian of tests/linearised_heat.py.

The shapes, steps and launches of test_gpu_derivative_edges.py (Nz in 2, 3, 31, 32, 33, 63, 64 x 13 columns, one column at Nz = 2 and
64; six steps in launches of 4 and 2, K = 4): its 36 series cases, the series on the top lane, each with rho_soc 0 and 26.  Per case,
within 8 x e_ref of the case (e_ref computed on the CPU by param_series_derivatives.reference, a bound above 1e-12 refused, exact 0.0
where every reference product is zero):
  tangents    parameter seeds alone; and one joint launch with the state seed, the node seeds, the per-column seeds of the pairs without
              a series and the parameter seeds, against the sum of the reference products -- the one product that shows the blocks do
              not overwrite one another.  The primal after the call is trm_step's with the same series bit for bit (fields, status,
              clock, the written-back boundary values), and the launch reports both families of seeds, the series and the layout.
  gradients   dL/dU_0, the node gradients, the per-column gradients of the other pairs and the ten parameter gradients from ONE sweep
              with the parameter gradient open; the checkpointed tape gives the per-step tape's bit for bit."""
import numpy as np
import pytest

import param_series_derivatives as PS
import terrarium_jl_amd as trm
from boundary_derivatives import PAIRS
from parameter_derivatives import PARAMS
from test_gpu_derivative_edges import DT, K, SERIES_PAIR, STEPS, case_id, device, report
from test_gpu_series_derivative import boundary_values
from test_gpu_tangent import STATE, TANGENTS, bits

pytestmark = pytest.mark.gpu


def param_series_device(case, steps_per_launch=None):
    d = device(case) if steps_per_launch is None else device(case, steps_per_launch=steps_per_launch)
    d.set_option("derivative_series_params", 1)
    return d


def stepped_twin(case):
    """what trm_step leaves with the same series, under the library's own choice of program: state, status, clock, boundary values"""
    b = device(case, steps_per_launch=0)
    b.set_option("derivative_series", 0)                                        # (trm_step does not read it)
    b.step(DT, STEPS, finalize=True)
    out = {name: bits(b.get(name)) for name in STATE}, b.status(), b.clock()
    b.clear_series()
    return out + (bits(boundary_values(b, SERIES_PAIR[case[2]])),)


def tangents(d, case, dU, params, series=None, boundary=None):
    d.restore_state()
    d.open_tangent()
    d.set_tangent("internal_energy", dU)
    if boundary is not None:
        for pair in PS.other_pairs(case):
            d.set_bc_tangent(*pair, boundary[PAIRS.index(pair)])
    d.set_param_tangent(dict(zip(PARAMS, params)))
    if series is not None:
        d.set_bc_series_tangent(*SERIES_PAIR[case[2]], series)
    d.step_tangent(DT, STEPS)
    prog = d.last_program()
    assert prog["family"] == "column_tangent" and prog["boundary_seeds"] and prog["parameter_seeds"], (case_id(case), prog)
    assert prog["series"] == 1 == d.get_option("info_derivative_series"), (case_id(case), prog)
    assert prog["lanes_per_column"] == (32 if case[0] <= 32 else 64), (case_id(case), prog)
    return np.stack([d.tangent(x) for x in TANGENTS])


def gradients(d, case, w, checkpoint_every=None):
    """{input: gradient} from one sweep with the parameter gradient open"""
    pair = SERIES_PAIR[case[2]]
    d.restore_state()
    d.open_adjoint(STEPS, checkpoint_every)
    d.open_param_gradient()
    d.step_record(DT, STEPS)
    recorded = {name: bits(d.get(name)) for name in STATE}, d.status(), d.clock()
    for x, wx in zip(TANGENTS, w):
        d.set_cotangent(x, wx)
    d.adjoint_backward()
    prog = d.last_program()
    assert prog["family"] == "column_adjoint" and prog["backward"] and prog["boundary_gradient"] and prog["parameter_gradient"], (case_id(case), prog)
    assert prog["checkpointed"] == (checkpoint_every is not None) and prog["series"] == 1
    assert prog["lanes_per_column"] == (32 if case[0] <= 32 else 64)
    boundary = np.zeros((len(PAIRS), case[1]))                                  # (the seriesed pair has no per-column gradient: its row stays 0)
    for other in PS.other_pairs(case):
        boundary[PAIRS.index(other)] = d.bc_gradient(*other)
    out = {"state": d.cotangent("internal_energy"), "series": d.bc_series_gradient(*pair), "boundary": boundary,
           "params": np.stack([d.param_gradient(name) for name in PARAMS])}
    d.close_adjoint()
    return out, recorded


@pytest.mark.parametrize("case", PS.CASES, ids=case_id)
def test_tangents_match_the_exact_jacobian(case):
    ref = PS.reference(case)
    v = ref.inputs[5]
    d = param_series_device(case)
    zero = np.zeros((case[0], case[1]))
    figures = {"tangent params": ref.error("tangent params", tangents(d, case, zero, v["params"]))}
    joint = tangents(d, case, v["state"], v["params"], series=v["series"], boundary=v["boundary"])
    figures["tangent joint"] = ref.error("tangent joint", joint)
    # the primal after the joint call is trm_step's with the same series
    state, status, clock, written = stepped_twin(case)
    for name in STATE:
        assert np.array_equal(bits(d.get(name)), state[name]), (case_id(case), name)
    assert d.status() == status and d.clock() == clock
    d.close_tangent()
    d.clear_series()
    assert np.array_equal(bits(boundary_values(d, SERIES_PAIR[case[2]])), written), (case_id(case), "written-back boundary values")
    report(ref, figures)


@pytest.mark.parametrize("case", PS.CASES, ids=case_id)
def test_gradients_match_the_exact_jacobian(case):
    ref = PS.reference(case)
    w = ref.inputs[5]["cotangents"]
    d = param_series_device(case)
    twin = stepped_twin(case)
    per_step, recorded = gradients(d, case, w)
    for name in STATE:                                                          # the recorded primal is trm_step's
        assert np.array_equal(recorded[0][name], twin[0][name]), (case_id(case), name)
    assert recorded[1:] == twin[1:3]
    checkpointed, _ = gradients(d, case, w, checkpoint_every=K)
    figures = {}
    for key, g in per_step.items():
        assert np.array_equal(bits(checkpointed[key]), bits(g)), (case_id(case), key, "checkpointed against per-step")
        figures[f"gradient {key}"] = ref.error(f"gradient {key}", g)
    if case[4] == 26.0:
        assert np.any(per_step["params"][PARAMS.index("k_organic")] != 0.0) and np.any(per_step["params"][PARAMS.index("c_organic")] != 0.0)
    report(ref, figures)
