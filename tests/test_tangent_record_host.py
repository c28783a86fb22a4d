"""Tangent records without a GPU: the C ABI of trm_tangent_record_attach and its five companions, the Python binding, the sums of
trm.record_normal_equations against an explicit restatement, the stand-alone precondition program, and the reference side of
test_gpu_tangent_record.py -- for every case the regime mask keeps every column and 0 < 8 x e_ref <= 1e-12.  Both are conditions on the
inputs of the cases; no figure of the device enters them."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import abi_header
import tangent_record as TR
import terrarium_jl_amd as trm
from terrarium_jl_amd.derivatives import _normal_equation_sums
from test_gpu_derivative_edges import BROKEN, FACTOR, STEPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("trm_tangent_record_attach", "trm_tangent_record_rewind", "trm_tangent_record_detach", "trm_tangent_record_download",
         "trm_tangent_record_device_ptr", "trm_tangent_record_info")


def test_library_exports_the_tangent_record_entry_points():
    lib = ctypes.CDLL(trm._capi.LIB_PATH)
    for name in NAMES:
        assert name in abi_header.functions(), name
        assert hasattr(lib, name) and name in trm._capi.EXPORTS, name
    assert abi_header.table("TRM_TANGENT_RECORD_") == dict(temperature=0, tangent=1) == trm._capi.TANGENT_RECORD


def test_the_five_rides_are_built():
    csrc = os.path.join(ROOT, "terrarium.jl_amd", "csrc")
    rides = {"": "RIDE_NONE", "_bc": "RIDE_BC", "_param": "RIDE_PARAM", "_series": "RIDE_SERIES", "_param_series": "RIDE_PARAM_SERIES"}
    blob = open(trm._capi.LIB_PATH, "rb").read()
    for n, (suffix, ride) in enumerate(rides.items()):
        text = open(os.path.join(csrc, f"trm_launch_column_tangent_record{suffix}.hip")).read()
        assert f"template int tangent_step<{ride}, WITH_RECORD>" in text, suffix
        # the library holds the kernel at this ride in both lane layouts (<HYD, LPC, (trm::Ride)n> is spelled ILi<h>ELi<lpc>ELNS_4RideE<n>E)
        for lpc in (32, 64):
            assert re.search(b"23k_column_tangent_recordILi\\d+ELi%dELNS_4RideE%dE" % (lpc, n), blob), (suffix, lpc)


def test_no_context_is_refused_without_a_gpu():
    L = trm._capi.lib()
    EINVAL = trm._capi.TRM_EINVAL
    idx = np.zeros(1, dtype=np.int32)
    a = np.zeros(1)
    n, m, at, b = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int64(0)
    dev = ctypes.c_void_p()
    assert L.trm_tangent_record_attach(None, 1, idx.ctypes.data, 1, idx.ctypes.data) == EINVAL
    assert L.trm_tangent_record_rewind(None) == EINVAL
    assert L.trm_tangent_record_detach(None) == EINVAL
    assert L.trm_tangent_record_download(None, 0, a.ctypes.data) == EINVAL
    assert L.trm_tangent_record_device_ptr(None, 0, ctypes.byref(dev)) == EINVAL
    assert L.trm_tangent_record_info(None, ctypes.byref(n), ctypes.byref(m), ctypes.byref(at), ctypes.byref(b)) == EINVAL


def test_python_interface():
    def names(f):
        return list(inspect.signature(f).parameters)

    def defaults(f):
        return {k: v.default for k, v in inspect.signature(f).parameters.items() if v.default is not inspect.Parameter.empty}

    D = trm.DeviceState
    assert names(D.attach_tangent_record) == ["self", "positions", "levels"]
    for method in (D.rewind_tangent_record, D.detach_tangent_record, D.tangent_record_info):
        assert names(method) == ["self"]
    assert names(D.tangent_record) == ["self", "which"]
    assert names(trm.record_jvp) == ["integ", "positions", "levels", "d_internal_energy", "d_boundary", "d_params", "steps"]
    assert defaults(trm.record_jvp) == dict(d_internal_energy=0.0, d_boundary=None, d_params=None, steps=None)
    assert names(trm.record_normal_equations) == ["integ", "record", "params"]
    # the pinned ones stay
    assert names(trm.jvp) == ["integ", "d_internal_energy", "steps", "d_boundary", "d_params"]
    assert names(trm.record_gradient) == ["integ", "record", "steps", "checkpoint_every", "wrt_boundary", "wrt_params"]


def test_refusals_before_the_integrator_is_touched():
    class Stub:
        timestepper = trm.ForwardEuler()

        def _has_time_dependence(self):
            return False

        def _windowed(self):
            return False

    for positions in ([], [0, 3, 3], [3, 0], [-1, 2]):
        with pytest.raises(ValueError, match="strictly increasing"):
            trm.record_jvp(Stub(), positions, [0])
    twice = trm.TemperatureRecord([0, 3, 3], [0], np.zeros((3, 1, 5)))
    with pytest.raises(ValueError, match="strictly increasing"):
        trm.record_normal_equations(Stub(), twice, ["k_mineral"])
    with pytest.raises(ValueError, match="no parameter"):
        trm.record_normal_equations(Stub(), trm.TemperatureRecord([0, 3], [0], np.zeros((2, 1, 5))), [])


@pytest.mark.parametrize("weighted", (True, False), ids=("weights", "no-weights"))
def test_normal_equation_sums_are_the_explicit_loops_bit_for_bit(weighted):
    """misfit = sum 1/2 w r r, b_q = sum w s_q r, A_qq' = sum w s_q s_q' with r = T - values: positions ascending, levels in list order,
    one term at a time in float64; a NaN sample and a weight that is not > 0 count for nothing"""
    rng = np.random.default_rng(22)
    npos, nlevels, Nh, nq = 5, 3, 7, 2
    T = rng.normal(0.0, 3.0, (npos, nlevels, Nh))
    S = [rng.normal(0.0, 1e-3, (npos, nlevels, Nh)) * 10.0 ** q for q in range(nq)]
    values = T + rng.normal(0.0, 1.0, T.shape)
    weight = rng.uniform(0.5, 2.0, T.shape) if weighted else None
    values[0, 0, 0] = values[2, 1, 3] = values[4, 2, 6] = np.nan            # gaps in the record
    T[1, 1, 1] = np.nan                                                      # a position the run has not reached
    S[0][1, 1, 1] = S[1][1, 1, 1] = np.nan
    if weighted:
        weight[0, 1, 2] = 0.0
        weight[3, 0, 5] = -1.0
        weight[3, 2, 4] = np.nan
    misfit, b, A = _normal_equation_sums(T, S, values, weight)
    for c in range(Nh):
        L, bc, Ac = 0.0, [0.0] * nq, [[0.0] * nq for _ in range(nq)]
        for k in range(npos):
            for j in range(nlevels):
                w = float(weight[k, j, c]) if weighted else 1.0
                r = float(T[k, j, c]) - float(values[k, j, c])
                if not w > 0.0 or r != r:
                    continue
                L = L + 0.5 * w * r * r
                for q in range(nq):
                    bc[q] = bc[q] + w * float(S[q][k, j, c]) * r
                    for q2 in range(nq):
                        Ac[q][q2] = Ac[q][q2] + w * float(S[q][k, j, c]) * float(S[q2][k, j, c])
        assert misfit[c].tobytes() == np.float64(L).tobytes(), c
        assert b[:, c].tobytes() == np.array(bc).tobytes(), c
        assert np.ascontiguousarray(A[:, :, c]).tobytes() == np.array(Ac).tobytes(), c
    assert np.all(np.isfinite(misfit)) and np.all(np.isfinite(b)) and np.all(np.isfinite(A)) and np.all(misfit > 0)
    # ((w s_q) s_q' rounds once per product: A is symmetric to rounding, not bit for bit)
    assert np.allclose(A, np.swapaxes(A, 0, 1), rtol=1e-14, atol=0.0)


def test_cases_are_those_of_the_attached_adjoint_record():
    import adjoint_record as AR
    assert TR.CASES is AR.CASES and len(TR.CASES) == 48 + 12 + 4
    assert {rc[1][0] for rc in TR.CASES} == {2, 3, 32, 33, 64} and {rc[1][1] for rc in TR.CASES} == {13, 1}
    assert len({rc[1][3] for rc in TR.CASES}) == 2                           # (both halo policies)
    assert any(rc[1][5] for rc in TR.CASES) and any(rc[1][5] is None for rc in TR.CASES)
    for rcase in TR.CASES:
        assert TR.positions_of(rcase)[-1] == STEPS
        assert TR.seed_keys(rcase[1]) == (("state", "series", "params") if rcase[1][5] else ("state", "boundary", "params"))


@pytest.mark.parametrize("rcase", TR.CASES, ids=TR.record_id)
def test_reference_side_of_the_gpu_test(rcase):
    ref = TR.reference(rcase)
    assert ref.keep.all(), (TR.record_id(rcase), "the regime mask drops a column", np.flatnonzero(~ref.keep))
    bound = FACTOR * ref.e_ref
    print(f"{TR.record_id(rcase)}: e_ref = {ref.e_ref:.3e}, bound = {bound:.3e}")
    for label, err in ref.parts.items():
        print(f"    {label}: e_ref = {err:.3e}")
    assert 0.0 < bound <= BROKEN, (TR.record_id(rcase), ref.parts)
    keys = TR.seed_keys(rcase[1])
    assert set(ref.parts) == {f"dT {key}" for key in keys} | {f"identity {key}" for key in keys} | {"temperature"}
    npos, nlevels = len(TR.positions_of(rcase)), len(TR.levels_of(rcase))
    for key in keys:
        assert ref.expected[f"dT {key}"][0].shape == (npos, nlevels, rcase[1][1]) and ref.expected[f"identity {key}"][0].shape == (rcase[1][1],)
    # the state seed moves every sample but those in phase change, position 0 included (the entry closure's tangent)
    assert np.any(ref.expected["dT state"][1][0] > 0) and np.any(ref.expected["dT state"][1][-1] > 0)


def test_tangent_record_preconditions_hold_under_the_host_sanitizers():
    """tests/tangent_record_preconditions.cpp: the tables, the attach refusals with their text, the cut of the launches at the last
    position and the launcher's preconditions, on contexts built by hand -- a stand-alone program of host code alone, built with the
    host sanitizers, no GPU call"""
    csrc = os.path.join(ROOT, "terrarium.jl_amd", "csrc")
    r = subprocess.run(["make", "-C", csrc, "-s", "check-preconditions", "PRECONDITIONS=tangent_record_preconditions"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "tangent record preconditions ok" in r.stdout
