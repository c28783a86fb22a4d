"""The checkpointed adjoint tape without a GPU: the C ABI of trm_adjoint_open_checkpointed / trm_adjoint_checkpoints and its Python binding."""
import ctypes
import inspect

import abi_header
import terrarium_jl_amd as trm

NAMES = ("trm_adjoint_open_checkpointed", "trm_adjoint_checkpoints")


def test_library_exports_the_checkpoint_entry_points():
    """(the two interval #defines against the binding, and the ABI version: tests/test_abi_tables.py)"""
    lib = ctypes.CDLL(trm._capi.LIB_PATH)
    for name in NAMES:
        assert name in abi_header.functions(), name
        assert hasattr(lib, name) and name in trm._capi.EXPORTS, name


def test_no_context_is_refused_without_a_gpu():
    L = trm._capi.lib()
    k, n, cap = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
    assert L.trm_adjoint_open_checkpointed(None, 4, 16) == trm._capi.TRM_EINVAL
    assert L.trm_adjoint_checkpoints(None, ctypes.byref(k), ctypes.byref(n), ctypes.byref(cap)) == trm._capi.TRM_EINVAL


def test_decode_program_names_the_checkpointed_launches():
    d = trm._capi.decode_program(15 | (1 << 27))
    assert d["family"] == "column_adjoint" and d["checkpointed"] is True and not d["backward"] and not d["generic_boundaries"]
    d = trm._capi.decode_program(15 | (1 << 10) | (1 << 25) | (1 << 26) | (1 << 27))
    assert d["checkpointed"] and d["backward"] and d["generic_boundaries"] and d["lanes_per_column"] == 32
    assert trm._capi.decode_program(15)["checkpointed"] is False
    assert trm._capi.decode_program(15 | (1 << 26))["checkpointed"] is False
    # the tangent family, and the families that use bit 27 themselves, decode as before
    assert "checkpointed" not in trm._capi.decode_program(14 | (1 << 27))
    assert "checkpointed" not in trm._capi.decode_program(8 | (1 << 27))


def test_python_interface_exists():
    assert callable(trm.DeviceState.adjoint_checkpoints)
    assert inspect.signature(trm.DeviceState.open_adjoint).parameters["checkpoint_every"].default is None
    assert inspect.signature(trm.vjp).parameters["checkpoint_every"].default is None
    # the first argument keeps its place: open_adjoint(capacity) is today's call
    assert list(inspect.signature(trm.DeviceState.open_adjoint).parameters)[:2] == ["self", "capacity"]
