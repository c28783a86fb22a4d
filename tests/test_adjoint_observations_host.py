"""Adjoint observations without a GPU: the C ABI of trm_adjoint_observe / trm_adjoint_observe_misfit and their getters, the Python
binding, and the reference side of test_gpu_adjoint_observations.py -- for every case the bound FACTOR x e_ref is a measurement of
fp64 rounding (0 < bound <= BROKEN) and the regime mask keeps every column.  Both are conditions on the inputs of the cases; no figure
of the device enters them."""
import ctypes
import inspect

import numpy as np
import pytest

import abi_header
import adjoint_observations as AO
import terrarium_jl_amd as trm
from test_gpu_derivative_edges import BROKEN, FACTOR, case_id

NAMES = ("trm_adjoint_observe", "trm_adjoint_observe_misfit", "trm_adjoint_misfit_download", "trm_adjoint_misfit_device_ptr", "trm_adjoint_observations")


def test_library_exports_the_observation_entry_points():
    lib = ctypes.CDLL(trm._capi.LIB_PATH)
    for name in NAMES:
        assert name in abi_header.functions(), name
        assert hasattr(lib, name) and name in trm._capi.EXPORTS, name


def test_no_context_is_refused_without_a_gpu():
    L = trm._capi.lib()
    levels = np.zeros(1, dtype=np.int32)
    a = np.zeros(1)
    n, b = ctypes.c_int32(0), ctypes.c_int64(0)
    dev = ctypes.c_void_p()
    assert L.trm_adjoint_observe(None, 0, 1, levels.ctypes.data, a.ctypes.data) == trm._capi.TRM_EINVAL
    assert L.trm_adjoint_observe_misfit(None, 1, levels.ctypes.data, a.ctypes.data, None) == trm._capi.TRM_EINVAL
    assert L.trm_adjoint_misfit_download(None, a.ctypes.data) == trm._capi.TRM_EINVAL
    assert L.trm_adjoint_misfit_device_ptr(None, ctypes.byref(dev)) == trm._capi.TRM_EINVAL
    assert L.trm_adjoint_observations(None, ctypes.byref(n), ctypes.byref(b)) == trm._capi.TRM_EINVAL


def test_python_interface():
    def names(f):
        return list(inspect.signature(f).parameters)

    def defaults(f):
        return {k: v.default for k, v in inspect.signature(f).parameters.items() if v.default is not inspect.Parameter.empty}

    assert names(trm.DeviceState.observe) == ["self", "levels", "temperature", "internal_energy", "liquid_water_fraction"]
    assert defaults(trm.DeviceState.observe) == dict(temperature=None, internal_energy=None, liquid_water_fraction=None)
    assert names(trm.DeviceState.observe_misfit) == ["self", "levels", "observed", "weight"] and defaults(trm.DeviceState.observe_misfit) == dict(weight=None)
    assert names(trm.DeviceState.misfit) == ["self"] and names(trm.DeviceState.adjoint_observations) == ["self"]
    assert names(trm.TemperatureRecord.__init__) == ["self", "steps", "levels", "values", "weight"] and defaults(trm.TemperatureRecord.__init__) == dict(weight=None)
    assert names(trm.misfit_gradient) == ["integ", "record", "steps", "checkpoint_every", "wrt_boundary", "wrt_params"]
    assert defaults(trm.misfit_gradient) == dict(steps=None, checkpoint_every=None, wrt_boundary=False, wrt_params=False)
    # the pinned signatures stay as they are
    assert names(trm.vjp) == ["integ", "steps", "temperature", "internal_energy", "liquid_water_fraction", "checkpoint_every", "wrt_boundary", "wrt_params"]
    assert names(trm.DeviceState.open_adjoint) == ["self", "capacity", "checkpoint_every"]


def test_temperature_record_and_tape_sizing():
    from terrarium_jl_amd.derivatives import _tape_slots
    rec = trm.TemperatureRecord([0, 3, 5, 6], [0, 2], np.zeros((4, 2, 5)), weight=2.0)
    assert rec.steps == [0, 3, 5, 6] and rec.levels.dtype == np.int32 and rec.weight.shape == (4, 2, 5)
    with pytest.raises(ValueError):
        trm.TemperatureRecord([3, 0], [0], np.zeros((2, 1, 5)))
    with pytest.raises(ValueError):
        trm.TemperatureRecord([0, 3], [0, 1], np.zeros((2, 1, 5)))
    # per-step: a slot per step; checkpointed: ceil(stretch / K) over the stretches between observed positions
    assert _tape_slots([0, 3, 5, 6], 6, None) == 6
    assert _tape_slots([0, 3, 5, 6], 6, 4) == 3            # 0-3, 3-5, 5-6
    assert _tape_slots([0, 6], 6, 4) == 2                  # 0-4, 4-6: the observations at the ends close nothing
    assert _tape_slots([12, 24], 30, 16) == 3              # 0-12, 12-24, 24-30
    assert _tape_slots([9], 30, 4) == 3 + 6                # 0-9, 9-30
    assert _tape_slots([], 0, 4) == 1


def test_cases_cover_what_the_lane_layouts_can_get_wrong():
    shapes = {(c[0], c[1]) for c in AO.CASES}
    assert shapes == {(2, 13), (3, 13), (32, 13), (33, 13), (64, 13), (64, 1)}
    assert {c[2] for c in AO.CASES} == set(AO.SETS) and {c[4] for c in AO.CASES} == {0.0, 26.0}
    for shape in shapes:
        mine = [c for c in AO.CASES if (c[0], c[1]) == shape]
        assert {c[2] for c in mine if c[5] is None} == set(AO.SETS) and any(c[5] for c in mine)
    assert AO.observed_levels(2) == [0, 1] and AO.observed_levels(32) == [0, 31] and AO.observed_levels(33) == [0, 31, 32]
    assert AO.observed_levels(64) == [0, 31, 32, 63]
    assert AO.POSITIONS == (0, 3, 5, 6) and AO.STEPS == 6 and AO.K == 4


@pytest.mark.parametrize("case", AO.CASES, ids=case_id)
def test_reference_side_of_the_gpu_test(case):
    ref = AO.reference(case)
    assert ref.keep.all(), (case_id(case), "the regime mask drops a column", np.flatnonzero(~ref.keep))
    bound = FACTOR * ref.e_ref
    print(f"{case_id(case)}: e_ref = {ref.e_ref:.3e}, bound = {bound:.3e}")
    for label, err in ref.parts.items():
        print(f"    {label}: e_ref = {err:.3e}")
    assert 0.0 < bound <= BROKEN, (case_id(case), ref.parts)
    # ... and so is the bound of every contraction by itself, unless every product of the contraction is zero
    for label, err in ref.parts.items():
        assert err > 0.0 or np.all(ref.expected[label][1] == 0), (case_id(case), label)
    # T_obs is at least 0.5 K off the model temperature, every weight positive: the residuals keep their digits
    for k, s in enumerate(AO.POSITIONS):
        T = AO.prefix(case, s, np.float64).value("temperature")[ref.record["levels"]]
        assert np.all(np.abs(T - ref.record["observed"][k]) >= 0.5 - 1e-9) and np.all(ref.record["weight"][k] > 0)
    # every input has a part of either kind, and the loss has one
    keys = ["state", "boundary", "params"] + (["series"] if case[5] else [])
    assert set(ref.parts) == {f"{kind} gradient {key}" for kind in AO.KINDS for key in keys} | {"misfit loss"}
    # the misfit's gradient is no accident of zeros: it has weight in S at position 0 and on the top level
    assert np.all(ref.expected["misfit gradient state"][1][ref.record["levels"][-1]] > 0)
