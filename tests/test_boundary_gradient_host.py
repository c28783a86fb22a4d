"""Boundary seeds and boundary gradients without a GPU: the C ABI of trm_tangent_bc_upload / trm_adjoint_bc_*, its Python binding, and
the oracle-side half of the central-difference check of test_gpu_boundary_gradient.py -- the inputs of that check are proved here, on
the CPU: enough columns stay clear of a regime boundary, and the central difference has converged at the step sizes it uses."""
import ctypes
import inspect

import numpy as np
import pytest

import abi_header
import terrarium_jl_amd as trm
import boundary_derivatives as B

NAMES = ("trm_tangent_bc_upload", "trm_adjoint_bc_open", "trm_adjoint_bc_download", "trm_adjoint_bc_device_ptr")


def test_library_exports_the_boundary_entry_points():
    lib = ctypes.CDLL(trm._capi.LIB_PATH)
    for name in NAMES:
        assert name in abi_header.functions(), name
        assert hasattr(lib, name) and name in trm._capi.EXPORTS, name


def test_no_context_is_refused_without_a_gpu():
    L = trm._capi.lib()
    E = trm._capi.TRM_EINVAL
    buf = (ctypes.c_double * 4)()
    dev = ctypes.c_void_p()
    T = trm._capi.BC_VAR["temperature"]
    assert L.trm_tangent_bc_upload(None, T, 1, buf) == E
    assert L.trm_adjoint_bc_open(None) == E
    assert L.trm_adjoint_bc_download(None, T, 1, buf) == E
    assert L.trm_adjoint_bc_device_ptr(None, T, 1, ctypes.byref(dev)) == E


def test_decode_program_names_the_boundary_instances():
    decode = trm._capi.decode_program
    assert decode(14 | 1 << 26)["boundary_seeds"] and not decode(14)["boundary_seeds"]
    assert decode(15 | 1 << 30)["boundary_gradient"] and not decode(15)["boundary_gradient"]
    assert not decode(14 | 1 << 30)["boundary_seeds"] and not decode(15 | 1 << 26)["boundary_gradient"]
    for family in range(len(trm._capi.PROGRAM)):
        d = decode(family | 1 << 26 | 1 << 30)
        assert ("boundary_seeds" in d) == (family == 14), family
        assert ("boundary_gradient" in d) == (family == 15), family
    # the existing keys of both families are what they were
    d = decode(15 | 1 << 26)
    assert d["family"] == "column_adjoint" and d["backward"] and not d["generic_boundaries"] and not d["checkpointed"]
    d = decode(15 | 1 << 10 | 1 << 25 | 1 << 26 | 1 << 27 | 1 << 30)
    assert d["lanes_per_column"] == 32 and d["backward"] and d["generic_boundaries"] and d["checkpointed"] and d["boundary_gradient"]
    assert "averages" not in d
    d = decode(14 | 1 << 27)
    assert d["family"] == "column_tangent" and not d["generic_boundaries"] and not d["boundary_seeds"] and "backward" not in d
    d = decode(14 | 2 << 10 | 1 << 25 | 1 << 26)
    assert d["lanes_per_column"] == 64 and d["generic_boundaries"] and d["boundary_seeds"]


def test_python_interface_exists():
    for m in ("set_bc_tangent", "open_bc_gradient", "bc_gradient"):
        assert callable(getattr(trm.DeviceState, m)), m
    jvp, vjp = inspect.signature(trm.jvp).parameters, inspect.signature(trm.vjp).parameters
    assert jvp["d_boundary"].default is None
    assert vjp["wrt_boundary"].default is False
    assert list(jvp)[:3] == ["integ", "d_internal_energy", "steps"] and list(vjp)[:2] == ["integ", "steps"]


@pytest.mark.parametrize("halo", B.HALOS)
@pytest.mark.parametrize("bcset", B.FD_SETS)
def test_central_differences_of_the_oracle_have_converged(bcset, halo):
    """the input condition of test_gpu_boundary_gradient.py's central-difference check: at least FD_KEEP_SHARE of the columns kept, and
    in each of them the central difference of the loss at h and at h / 2 agree to 1e-8 of S = sum |w| |fd|"""
    p, U0, sat, bcs, w = B.fd_inputs(bcset, halo)
    keep = B.fd_kept_columns(p, U0, sat, bcs)
    print(f"{bcset} {halo}: kept share {keep.mean():.4f}")
    assert keep.mean() >= B.FD_KEEP_SHARE
    pairs = B.active_pairs(bcs)
    assert len(pairs) == 2
    for pair in pairs:
        h = B.FD_H[bcs[pair][0]]
        _, _, fd, S = B.fd_central(p, U0, sat, bcs, pair, w, h)
        _, _, fd_half, _ = B.fd_central(p, U0, sat, bcs, pair, w, 0.5 * h)
        assert np.all(S[keep] > 0)
        err = float(np.max(np.abs(fd - fd_half)[keep] / S[keep]))
        print(f"{bcset} {halo} {pair}: h = {h:g}, max |fd(h) - fd(h / 2)| / S = {err:.3e}")
        assert err <= 1e-8
