"""Attached temperature records without a GPU: the C ABI of trm_adjoint_observe_record and its six companions, the Python binding, the
stand-alone precondition program, and the reference side of test_gpu_adjoint_record.py -- for every case the bound FACTOR x e_ref is a
measurement of fp64 rounding (0 < bound <= BROKEN) and the regime mask keeps every column.  Both are conditions on the inputs of the
cases; no figure of the device enters them."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

import abi_header
import adjoint_observations as AO
import adjoint_record as AR
import terrarium_jl_amd as trm
from test_gpu_derivative_edges import BROKEN, FACTOR, STEPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("trm_adjoint_observe_record", "trm_adjoint_observe_record_device", "trm_adjoint_record_detach", "trm_adjoint_record_residual_download",
         "trm_adjoint_record_residual_device_ptr", "trm_adjoint_record_misfit_download", "trm_adjoint_record_info")


def test_library_exports_the_record_entry_points():
    lib = ctypes.CDLL(trm._capi.LIB_PATH)
    for name in NAMES:
        assert name in abi_header.functions(), name
        assert hasattr(lib, name) and name in trm._capi.EXPORTS, name
    # additive entries: the option table stays
    assert trm._capi.OPTION["derivative_series_params"] == 15


def test_no_context_is_refused_without_a_gpu():
    L = trm._capi.lib()
    EINVAL = trm._capi.TRM_EINVAL
    idx = np.zeros(1, dtype=np.int32)
    a = np.zeros(1)
    n, m, b = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int64(0)
    dev = ctypes.c_void_p()
    assert L.trm_adjoint_observe_record(None, 1, idx.ctypes.data, 1, idx.ctypes.data, a.ctypes.data, None) == EINVAL
    assert L.trm_adjoint_observe_record_device(None, 1, idx.ctypes.data, 1, idx.ctypes.data, a.ctypes.data, None) == EINVAL
    assert L.trm_adjoint_record_detach(None) == EINVAL
    assert L.trm_adjoint_record_residual_download(None, a.ctypes.data) == EINVAL
    assert L.trm_adjoint_record_residual_device_ptr(None, ctypes.byref(dev)) == EINVAL
    assert L.trm_adjoint_record_misfit_download(None, a.ctypes.data) == EINVAL
    assert L.trm_adjoint_record_info(None, ctypes.byref(n), ctypes.byref(m), ctypes.byref(b)) == EINVAL


def test_python_interface():
    def names(f):
        return list(inspect.signature(f).parameters)

    def defaults(f):
        return {k: v.default for k, v in inspect.signature(f).parameters.items() if v.default is not inspect.Parameter.empty}

    D = trm.DeviceState
    assert names(D.attach_record) == ["self", "positions", "levels", "observed", "weight"] and defaults(D.attach_record) == dict(weight=None)
    for method in (D.detach_record, D.record_residuals, D.record_misfit, D.record_info):
        assert names(method) == ["self"]
    assert names(trm.record_gradient) == ["integ", "record", "steps", "checkpoint_every", "wrt_boundary", "wrt_params"]
    assert defaults(trm.record_gradient) == dict(steps=None, checkpoint_every=None, wrt_boundary=False, wrt_params=False)
    # the pinned ones stay
    assert names(trm.misfit_gradient) == names(trm.record_gradient) and defaults(trm.misfit_gradient) == defaults(trm.record_gradient)
    assert names(trm.TemperatureRecord.__init__) == ["self", "steps", "levels", "values", "weight"]
    assert names(D.observe) == ["self", "levels", "temperature", "internal_energy", "liquid_water_fraction"]
    assert names(D.observe_misfit) == ["self", "levels", "observed", "weight"]
    assert names(trm.vjp) == ["integ", "steps", "temperature", "internal_energy", "liquid_water_fraction", "checkpoint_every", "wrt_boundary", "wrt_params"]
    assert names(D.open_adjoint) == ["self", "capacity", "checkpoint_every"]
    from terrarium_jl_amd.derivatives import _tape_slots
    assert _tape_slots([0, 3, 5, 6], 6, 4) == 3 and _tape_slots([], 6, 4) == 2      # (the per-position path's count, and the attached record's)


def test_record_gradient_wants_one_sample_per_position():
    class Stub:                                                 # (refused before the integrator is touched beyond its timestepper)
        timestepper = trm.ForwardEuler()

        def _has_time_dependence(self):
            return False

        def _windowed(self):
            return False

    twice = trm.TemperatureRecord([0, 3, 3], [0], np.zeros((3, 1, 5)))
    with pytest.raises(ValueError, match="strictly increasing"):
        trm.record_gradient(Stub(), twice)


def test_cases_cover_what_the_lane_layouts_can_get_wrong():
    assert AR.GROUPS["AO"] == AO.CASES and len(AO.CASES) == 48
    dense = AR.GROUPS["dense"]
    assert {(c[0], c[1]) for c in dense} == {(3, 13), (33, 13), (64, 1)} and {c[4] for c in dense} == {26.0}
    for shape in AR.DENSE_SHAPES:
        mine = [c for c in dense if (c[0], c[1]) == shape]
        assert {c[2] for c in mine if c[5] is None} == set(AO.SETS) and sum(1 for c in mine if c[5]) == 1
    assert {(c[0], c[1]) for c in AR.GROUPS["ends"]} == {(2, 13)}
    for rcase in AR.CASES:
        Nz = rcase[1][0]
        positions, levels = AR.positions_of(rcase), AR.levels_of(rcase)
        assert positions[-1] == STEPS and list(positions) == sorted(set(positions)) and list(levels) == sorted(set(levels))
        if rcase[0] == "dense":
            assert positions == tuple(range(STEPS + 1)) and levels == list(range(Nz))
        if rcase[0] == "ends":
            assert positions == (0, STEPS) and len(levels) == 1
        if rcase[0] == "AO":
            assert positions == (0, 3, 5, 6) and levels == AO.observed_levels(Nz)


@pytest.mark.parametrize("rcase", AR.CASES, ids=AR.record_id)
def test_reference_side_of_the_gpu_test(rcase):
    ref = AR.reference(rcase)
    # the cap on columns left out is zero
    assert ref.keep.all(), (AR.record_id(rcase), "the regime mask drops a column", np.flatnonzero(~ref.keep))
    bound = FACTOR * ref.e_ref
    print(f"{AR.record_id(rcase)}: e_ref = {ref.e_ref:.3e}, bound = {bound:.3e}")
    for label, err in ref.parts.items():
        print(f"    {label}: e_ref = {err:.3e}")
    assert 0.0 < bound <= BROKEN, (AR.record_id(rcase), ref.parts)
    for label, err in ref.parts.items():
        assert 0.0 < FACTOR * err <= BROKEN or np.all(ref.expected[label][1] == 0), (AR.record_id(rcase), label, err)
    rec = ref.record
    assert rec["observed"].shape == (len(rec["positions"]), len(rec["levels"]), rcase[1][1]) == rec["weight"].shape
    for k in range(len(rec["positions"])):
        assert np.all(np.abs(ref.T_narrow[k] - rec["observed"][k]) >= 0.5 - 1e-9) and np.all(rec["weight"][k] > 0)
    keys = ["state", "boundary", "params"] + (["series"] if rcase[1][5] else [])
    assert set(ref.parts) == {f"misfit gradient {key}" for key in keys} | {"misfit loss"}
    assert np.all(ref.expected["misfit gradient state"][1][rec["levels"][-1]] > 0) and np.all(ref.identity[1] > 0)
    if rcase[0] == "AO":       # the record, and with it the reference, is the per-position path's
        theirs = AO.reference(rcase[1])
        assert all(np.array_equal(a, b) for a, b in zip(theirs.record["observed"], rec["observed"]))
        for label in ref.parts:
            assert np.array_equal(theirs.expected[label][0], ref.expected[label][0]), label


def test_record_preconditions_hold_under_the_host_sanitizers():
    """tests/record_preconditions.cpp: the position and level tables, slot counting with a record attached and every refusal with its
    text, on contexts built by hand -- a stand-alone program of host code alone, built with the host sanitizers, no GPU call"""
    csrc = os.path.join(ROOT, "terrarium.jl_amd", "csrc")
    r = subprocess.run(["make", "-C", csrc, "-s", "check-preconditions", "PRECONDITIONS=record_preconditions"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "record preconditions ok" in r.stdout
