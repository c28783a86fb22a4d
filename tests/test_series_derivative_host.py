"""Derivatives through boundary time series without a GPU: the C ABI of trm_tangent_bc_series_upload / trm_adjoint_bc_series_*, the option
TRM_OPT_DERIVATIVE_SERIES, the Python binding, and the oracle-side half of the central-difference check of
test_gpu_series_derivative.py -- its inputs are proved here, on the CPU: enough columns stay clear of a regime boundary, and the central
difference with respect to every node has converged at the step sizes it uses."""
import ctypes
import inspect

import numpy as np
import pytest

import abi_header
import terrarium_jl_amd as trm
import boundary_derivatives as B
import series_derivatives as S

NAMES = ("trm_tangent_bc_series_upload", "trm_adjoint_bc_series_download", "trm_adjoint_bc_series_device_ptr")


def test_library_exports_the_series_entry_points():
    lib = ctypes.CDLL(trm._capi.LIB_PATH)
    for name in NAMES:
        assert name in abi_header.functions(), name
        assert hasattr(lib, name) and name in trm._capi.EXPORTS, name


def test_no_context_is_refused_without_a_gpu():
    L = trm._capi.lib()
    E = trm._capi.TRM_EINVAL
    buf = (ctypes.c_double * 8)()
    dev, nt = ctypes.c_void_p(), ctypes.c_int32()
    T = trm._capi.BC_VAR["temperature"]
    assert L.trm_tangent_bc_series_upload(None, T, 1, 2, buf) == E
    assert L.trm_adjoint_bc_series_download(None, T, 1, 2, buf) == E
    assert L.trm_adjoint_bc_series_device_ptr(None, T, 1, ctypes.byref(dev), ctypes.byref(nt)) == E


def test_option_and_info_ids_agree_with_the_header():
    capi = trm._capi
    assert abi_header.enums()["TRM_OPT_DERIVATIVE_SERIES"] == 14 == capi.OPTION["derivative_series"]
    assert abi_header.enums()["TRM_INFO_DERIVATIVE_SERIES"] == 109 == capi.OPTION["info_derivative_series"]
    # no bit of TRM_INFO_LAST_PROGRAM was taken: the decoder is what it was
    assert set(capi.decode_program(14 | 1 << 26)) == set(capi.decode_program(14)) and "series" not in capi.decode_program(15 | 1 << 26 | 1 << 30)


def test_python_interface_exists():
    for m in ("set_bc_series_tangent", "bc_series_gradient"):
        assert callable(getattr(trm.DeviceState, m)), m
    assert list(inspect.signature(trm.DeviceState.set_bc_series_tangent).parameters) == ["self", "var", "side", "values"]
    assert list(inspect.signature(trm.DeviceState.bc_series_gradient).parameters) == ["self", "var", "side"]
    jvp, vjp = inspect.signature(trm.jvp).parameters, inspect.signature(trm.vjp).parameters
    assert jvp["d_boundary"].default is None and vjp["wrt_boundary"].default is False


def test_series_brackets_cover_the_cases():
    """what the shapes are chosen for: with 8 steps in launches of 3, 3, 2 the bracket changes inside a launch and between launches, a
    step lands exactly on a node, clamp starts before its first node and the cyclical run wraps"""
    t = np.arange(S.STEPS) * S.DT
    lin = S.node_times("linear")
    left = np.searchsorted(lin, t, side="right") - 1
    assert np.any(np.isin(t, lin[1:])) and left[2] != left[3] and left[4] != left[5]
    assert np.sum(t < S.node_times("clamp")[0]) == 2
    cyc = S.node_times("cyclical")
    assert t[-1] > cyc[-1] + (cyc[-1] - cyc[-2])


@pytest.mark.parametrize("bcset,pair,indexing,halo", S.fd_cases())
def test_central_differences_of_the_oracle_have_converged(bcset, pair, indexing, halo):
    """the input condition of test_gpu_series_derivative.py's central-difference check: at least FD_KEEP_SHARE of the columns kept, and in
    each of them the central differences of the loss at h and at h / 2 agree to 1e-8 of S = sum |w| |fd|, for every node"""
    p, U0, sat, bcs, w = S.fd_inputs(bcset, halo)
    series = S.series_on(bcs, [pair], indexing, B.FD_NH)
    keep = S.fd_kept_columns(p, U0, sat, bcs, series)
    print(f"{bcset} {pair} {indexing} {halo}: kept share {keep.mean():.4f}")
    assert keep.mean() >= S.FD_KEEP_SHARE
    h = B.FD_H[bcs[pair][0]]
    for node in range(S.NT):
        _, _, fd, Ssum = S.fd_central(p, U0, sat, bcs, series, pair, node, w, h)
        _, _, fd_half, _ = S.fd_central(p, U0, sat, bcs, series, pair, node, w, 0.5 * h)
        assert np.all(Ssum[keep] > 0), node
        err = float(np.max(np.abs(fd - fd_half)[keep] / Ssum[keep]))
        print(f"    node {node}: h = {h:g}, max |fd(h) - fd(h / 2)| / S = {err:.3e}")
        assert err <= 1e-8
