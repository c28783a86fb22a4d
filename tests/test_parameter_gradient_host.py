"""Parameter seeds and parameter gradients without a GPU: the C ABI of trm_tangent_param_set / trm_adjoint_param_*, its Python binding,
and the oracle-side half of the central-difference check of test_gpu_parameter_gradient.py -- the reference of that check is proved
here, on the CPU: enough columns stay clear of a regime boundary, and the Richardson-extrapolated central difference has converged at
the step sizes it uses."""
import ctypes
import inspect

import numpy as np
import pytest

import abi_header
import terrarium_jl_amd as trm
import parameter_derivatives as P

NAMES = ("trm_tangent_param_set", "trm_adjoint_param_open", "trm_adjoint_param_download", "trm_adjoint_param_device_ptr")


def test_library_exports_the_parameter_entry_points():
    lib = ctypes.CDLL(trm._capi.LIB_PATH)
    for name in NAMES:
        assert name in abi_header.functions(), name
        assert hasattr(lib, name) and name in trm._capi.EXPORTS, name
    # the enum is the order of trm_params
    assert abi_header.table("TRM_THERMAL_PARAM_") == {**{name: q for q, name in enumerate(P.PARAMS)}, "count": 10}
    assert trm._capi.THERMAL_PARAMS == P.PARAMS
    fields = [n for n, _ in trm._capi.default_params()._fields_]
    at = fields.index("k_water")
    assert tuple(fields[at:at + 10]) == P.PARAMS


def test_no_context_is_refused_without_a_gpu():
    L = trm._capi.lib()
    E = trm._capi.TRM_EINVAL
    seed = (ctypes.c_double * 10)()
    buf = (ctypes.c_double * 4)()
    dev = ctypes.c_void_p()
    assert L.trm_tangent_param_set(None, seed) == E
    assert L.trm_adjoint_param_open(None) == E
    assert L.trm_adjoint_param_download(None, 0, buf) == E
    assert L.trm_adjoint_param_device_ptr(None, 0, ctypes.byref(dev)) == E


def test_decode_program_names_the_parameter_instances():
    decode = trm._capi.decode_program
    bit = trm._capi.PROGRAM_PARAMETERS
    assert bit == 1 << 31 and abi_header.enums()["TRM_PROGRAM_PARAMETERS"] == -2147483647 - 1
    assert decode(14 | 1 << 26 | bit)["parameter_seeds"] and not decode(14 | 1 << 26)["parameter_seeds"]
    assert decode(15 | 1 << 26 | 1 << 30 | bit)["parameter_gradient"] and not decode(15 | 1 << 26 | 1 << 30)["parameter_gradient"]
    # the id is a C int: with bit 31 it arrives as a negative number
    as_int = ctypes.c_int32(15 | 1 << 10 | 1 << 26 | 1 << 27 | 1 << 30 | bit).value
    assert as_int < 0
    d = decode(as_int)
    assert d["parameter_gradient"] and d["boundary_gradient"] and d["backward"] and d["checkpointed"] and not d["generic_boundaries"]
    assert d["family"] == "column_adjoint" and d["lanes_per_column"] == 32 and "averages" not in d
    for family in range(len(trm._capi.PROGRAM)):
        d = decode(family | bit)
        assert ("parameter_seeds" in d) == (family == 14), family
        assert ("parameter_gradient" in d) == (family == 15), family
    # every old key keeps its value, with the bit and without
    for pid in (14, 14 | 2 << 10 | 1 << 25 | 1 << 26, 15 | 1 << 26, 15 | 1 << 10 | 1 << 25 | 1 << 26 | 1 << 27 | 1 << 30, 3 | 1 << 25 | 1 << 28):
        new = ("parameter_seeds", "parameter_gradient")
        plain = {k: v for k, v in decode(pid).items() if k not in new}
        assert plain == {k: v for k, v in decode(pid | bit).items() if k not in new}, pid
        assert all(not decode(pid)[k] for k in new if k in decode(pid)), pid
    d = decode(14 | 2 << 10 | 1 << 25 | 1 << 26)
    assert d["lanes_per_column"] == 64 and d["generic_boundaries"] and d["boundary_seeds"] and d["hydraulics"] == "default"


def test_python_interface_exists():
    for m in ("set_param_tangent", "open_param_gradient", "param_gradient"):
        assert callable(getattr(trm.DeviceState, m)), m
    jvp, vjp = inspect.signature(trm.jvp).parameters, inspect.signature(trm.vjp).parameters
    assert jvp["d_params"].default is None and jvp["d_boundary"].default is None
    assert vjp["wrt_params"].default is False and vjp["wrt_boundary"].default is False
    assert list(jvp)[:3] == ["integ", "d_internal_energy", "steps"] and list(vjp)[:2] == ["integ", "steps"]


@pytest.mark.parametrize("bcset,halo,rho_soc", P.FD_CASES)
def test_central_differences_of_the_oracle_have_converged(bcset, halo, rho_soc):
    """the input condition of test_gpu_parameter_gradient.py's central-difference check: at least FD_KEEP_SHARE of the columns stay clear
    of a regime boundary, and in each of them the Richardson extrapolations of the loss at (h, h / 2) and at (h / 2, h / 4) agree to
    1e-8 of S = sum |w| |fd|.  (Measured with these inputs: worst 2.1e-9, smallest kept share 0.875.)"""
    (p, U0, sat, bcs, w), keep, ref = P.fd_reference(bcset, halo, rho_soc, levels=3)
    print(f"{bcset} {halo} rho_soc={rho_soc:g}: kept share {keep.mean():.4f}")
    assert keep.mean() >= P.FD_KEEP_SHARE
    for name in P.PARAMS:
        (fd, S), (fd_fine, _) = P.loss_and_scale(ref[name][0], w), P.loss_and_scale(ref[name][1], w)
        if rho_soc == 0.0 and name.endswith("organic"):
            assert np.all(S == 0) and np.all(fd == 0) and np.all(fd_fine == 0), name     # no organic matter: no dependence at all
            continue
        cols = keep & (S > 0)
        assert cols.sum() >= P.FD_KEEP_SHARE * keep.sum(), name
        err = float(np.max(np.abs(fd - fd_fine)[cols] / S[cols]))
        print(f"{bcset} {halo} rho_soc={rho_soc:g} {name}: h = {P.fd_step(p, name):g}, {int(cols.sum())} columns, "
              f"max |R(h, h/2) - R(h/2, h/4)| / S = {err:.3e}")
        assert err <= 1e-8, name
