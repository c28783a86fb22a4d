"""The heat + Richards tangent without a GPU: the option, the two `which` values and the program family in the header and in the Python
tables, and the Python interface."""
import inspect

import pytest

import abi_header
import terrarium_jl_amd as trm

CAPI = trm._capi


def test_header_and_tables_agree():
    """(the whole tables and the ABI version: tests/test_abi_tables.py)"""
    enum = abi_header.enums()
    assert enum["TRM_OPT_DERIVATIVE_RICHARDS"] == 16 == CAPI.OPTION["derivative_richards"]
    assert enum["TRM_TANGENT_SATURATION"] == 3 == CAPI.TANGENT["saturation"] and enum["TRM_TANGENT_PRESSURE_HEAD"] == 4 == CAPI.TANGENT["pressure_head"]
    assert [CAPI.TANGENT[x] for x in ("internal_energy", "temperature", "liquid_water_fraction", "saturation", "pressure_head")] == [0, 1, 2, 3, 4]
    with pytest.raises(KeyError):
        CAPI.TANGENT["hydraulic_conductivity"]
    family = "column_tangent_richards"
    assert enum["TRM_PROGRAM_" + family.upper()] == 16 == CAPI.PROGRAM.index(family)
    assert "on a Richards context: state seeds only" in abi_header.text()


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
