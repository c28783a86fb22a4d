"""Forward-mode tangents without a GPU: the C ABI of trm_tangent_* / trm_step_tangent and its Python binding."""
import ctypes

import abi_header
import terrarium_jl_amd as trm

NAMES = ("trm_tangent_open", "trm_tangent_close", "trm_tangent_upload", "trm_tangent_download", "trm_tangent_device_ptr",
         "trm_tangent_closure", "trm_step_tangent")


def test_library_exports_the_tangent_entry_points():
    lib = ctypes.CDLL(trm._capi.LIB_PATH)
    for name in NAMES:
        assert name in abi_header.functions(), name
        assert hasattr(lib, name) and name in trm._capi.EXPORTS, name
    # (the tangent field ids, TANGENT as a whole table: tests/test_abi_tables.py)
    assert abi_header.enums()["TRM_PROGRAM_COLUMN_TANGENT"] == 14 == trm._capi.PROGRAM.index("column_tangent")
    # (k_closure_tangent is a template: no translation unit carries a renamed copy of it)
    assert b"k_closure_tangent_in_" not in open(trm._capi.LIB_PATH, "rb").read()


def test_no_context_is_refused_without_a_gpu():
    L = trm._capi.lib()
    E = trm._capi.TRM_EINVAL
    buf = (ctypes.c_double * 4)()
    assert L.trm_tangent_open(None) == E
    assert L.trm_tangent_close(None) == E
    assert L.trm_tangent_upload(None, 0, buf) == E
    assert L.trm_tangent_download(None, 0, buf) == E
    assert L.trm_tangent_device_ptr(None, 0, None, None) == E
    assert L.trm_tangent_closure(None) == E
    assert L.trm_step_tangent(None, 300.0, 1) == E


def test_decode_program_names_the_tangent_family():
    d = trm._capi.decode_program(14)
    assert d["family"] == "column_tangent" and not d["generic_boundaries"]
    d = trm._capi.decode_program(14 | (1 << 10) | (1 << 25))
    assert d["lanes_per_column"] == 32 and d["generic_boundaries"]


def test_python_interface_exists():
    for m in ("open_tangent", "close_tangent", "set_tangent", "tangent", "tangent_closure", "step_tangent"):
        assert callable(getattr(trm.DeviceState, m)), m
    assert callable(trm.jvp)
