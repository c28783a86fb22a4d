"""Reverse-mode gradients without a GPU: the C ABI of trm_adjoint_* / trm_step_record and its Python binding."""
import ctypes

import abi_header
import terrarium_jl_amd as trm

NAMES = ("trm_adjoint_open", "trm_adjoint_close", "trm_adjoint_upload", "trm_adjoint_download", "trm_adjoint_device_ptr",
         "trm_adjoint_tape", "trm_step_record", "trm_adjoint_backward")


def test_library_exports_the_adjoint_entry_points():
    lib = ctypes.CDLL(trm._capi.LIB_PATH)
    for name in NAMES:
        assert name in abi_header.functions(), name
        assert hasattr(lib, name) and name in trm._capi.EXPORTS, name
    enum = abi_header.enums()
    # the cotangent fields take the tangent's field codes
    for field in ("INTERNAL_ENERGY", "TEMPERATURE", "LIQUID_WATER_FRACTION"):
        assert enum["TRM_ADJOINT_" + field] == enum["TRM_TANGENT_" + field] == trm._capi.ADJOINT[field.lower()], field
    assert enum["TRM_PROGRAM_COLUMN_ADJOINT"] == 15 == trm._capi.PROGRAM.index("column_adjoint")
    assert enum["TRM_PROGRAM_COLUMN_TANGENT"] == 14


def test_no_context_is_refused_without_a_gpu():
    L = trm._capi.lib()
    E = trm._capi.TRM_EINVAL
    buf = (ctypes.c_double * 4)()
    n, cap = ctypes.c_int32(0), ctypes.c_int32(0)
    assert L.trm_adjoint_open(None, 4) == E
    assert L.trm_adjoint_close(None) == E
    assert L.trm_adjoint_upload(None, 0, buf) == E
    assert L.trm_adjoint_download(None, 0, buf) == E
    assert L.trm_adjoint_device_ptr(None, 0, None, None) == E
    assert L.trm_adjoint_tape(None, ctypes.byref(n), ctypes.byref(cap)) == E
    assert L.trm_step_record(None, 300.0, 1) == E
    assert L.trm_adjoint_backward(None) == E


def test_decode_program_names_the_adjoint_family():
    d = trm._capi.decode_program(15)
    assert d["family"] == "column_adjoint" and not d["generic_boundaries"] and not d["backward"]
    d = trm._capi.decode_program(15 | (1 << 10) | (1 << 25))
    assert d["lanes_per_column"] == 32 and d["generic_boundaries"] and not d["backward"]
    d = trm._capi.decode_program(15 | (2 << 10) | (1 << 26))
    assert d["lanes_per_column"] == 64 and not d["generic_boundaries"] and d["backward"]
    # the tangent family decodes as before
    assert "backward" not in trm._capi.decode_program(14 | (1 << 25))


def test_python_interface_exists():
    for m in ("open_adjoint", "close_adjoint", "set_cotangent", "cotangent", "step_record", "adjoint_backward", "adjoint_tape"):
        assert callable(getattr(trm.DeviceState, m)), m
    assert callable(trm.vjp)
