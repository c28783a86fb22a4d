"""The heat + Richards tangent without a GPU: the option, the two `which` values and the program family in the header and in the Python
tables, and the Python interface."""
import inspect
import os
import re

import pytest

import terrarium_jl_amd as trm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPI = trm._capi


def header_enum():
    header = open(os.path.join(ROOT, "include", "terrarium_hip.h")).read()
    return header, {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(TRM_[A-Z0-9_]+)\s*=\s*(\d+)", header)}


def test_header_and_tables_agree():
    header, enum = header_enum()
    assert enum["TRM_OPT_DERIVATIVE_RICHARDS"] == 16 == CAPI.option_id("derivative_richards")
    assert CAPI.TANGENT_RICHARDS == dict(saturation=enum["TRM_TANGENT_SATURATION"], pressure_head=enum["TRM_TANGENT_PRESSURE_HEAD"]) == dict(saturation=3, pressure_head=4)
    assert [CAPI.tangent_id(x) for x in ("internal_energy", "temperature", "liquid_water_fraction", "saturation", "pressure_head")] == [0, 1, 2, 3, 4]
    with pytest.raises(KeyError):
        CAPI.tangent_id("hydraulic_conductivity")
    assert enum["TRM_PROGRAM_COLUMN_TANGENT_RICHARDS"] == 16 == CAPI.PROGRAM.index("column_tangent_richards")
    assert re.search(r"#define\s+TRM_ABI_VERSION\s+20\b", header)          # (no new entry point)
    assert "on a Richards context: state seeds only" in header


def test_decode_program_names_the_family():
    d = CAPI.decode_program(16 | 2 << 8 | 2 << 10)
    assert d["family"] == "column_tangent_richards" and d["hydraulics"] == "generic" and d["lanes_per_column"] == 64
    d = CAPI.decode_program(16 | 1 << 10)
    assert d["hydraulics"] == "default" and d["lanes_per_column"] == 32
    assert "parameter_seeds" not in d and "boundary_seeds" not in d
    # no existing id decodes differently
    assert CAPI.decode_program(14)["family"] == "column_tangent" and CAPI.decode_program(15)["family"] == "column_adjoint"


def test_python_interface():
    # (the signature of jvp is pinned by earlier tests: the saturation seed travels in a dict of state seeds)
    assert list(inspect.signature(trm.jvp).parameters) == ["integ", "d_internal_energy", "steps", "d_boundary", "d_params"]
    assert "derivative_richards" in trm.jvp.__doc__ and '"saturation"' in trm.jvp.__doc__
    for doc in (trm.DeviceState.set_tangent.__doc__, trm.DeviceState.tangent.__doc__):
        assert "saturation" in doc
