"""Thermal-parameter derivatives of runs driven by boundary time series, without a GPU: the option TRM_OPT_DERIVATIVE_SERIES_PARAMS in the
header and the binding, the three translation units of the ride RIDE_PARAM_SERIES in the build, and the CPU reference of
test_gpu_param_series_edges.py -- properties of the reference alone (tests/param_series_derivatives.py, tests/linearised_heat.py): every
column is kept, 8 x e_ref stays under the ceiling 1e-12 above which the GPU module refuses a bound, the joint tangent's e_ref does not
exceed its largest part, and the organic parameters have non-zero blocks at rho_soc = 26."""
import ctypes
import glob
import inspect
import os
import re

import numpy as np
import pytest

import abi_header
import terrarium_jl_amd as trm
import param_series_derivatives as PS
from test_gpu_derivative_edges import BROKEN, FACTOR, SERIES_CASES, case_id

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "terrarium.jl_amd", "csrc")
UNITS = ("trm_launch_column_tangent_param_series", "trm_launch_column_adjoint_param_series", "trm_launch_column_adjoint_ckpt_param_series")


def test_option_agrees_with_the_header():
    """(the whole table, its one id space and the ABI version: tests/test_abi_tables.py)"""
    capi = trm._capi
    assert abi_header.enums()["TRM_OPT_DERIVATIVE_SERIES_PARAMS"] == 15 == capi.OPTION["derivative_series_params"]
    assert (capi.OPTION["derivative_series"], capi.OPTION["info_derivative_series"]) == (14, 109)
    # a launch of the ride reports the bits both families have: nothing new to decode
    prog = capi.decode_program(14 | 1 << 26 | capi.PROGRAM_PARAMETERS)
    assert prog["boundary_seeds"] and prog["parameter_seeds"]
    prog = capi.decode_program(15 | 1 << 26 | 1 << 30 | capi.PROGRAM_PARAMETERS)
    assert prog["backward"] and prog["boundary_gradient"] and prog["parameter_gradient"]


def test_the_ride_is_built_and_the_exports_are_what_they_were():
    sources = {os.path.splitext(os.path.basename(f))[0] for f in glob.glob(os.path.join(CSRC, "*.hip"))}
    assert set(UNITS) <= sources                                            # (the Makefile compiles every *.hip of the directory)
    assert "$(wildcard *.hip)" in open(os.path.join(CSRC, "Makefile")).read()
    instance = {UNITS[0]: r"template int tangent_step<RIDE_PARAM_SERIES, NO_RECORD>", UNITS[1]: r"template int adjoint_backward<false, RIDE_PARAM_SERIES, NO_RECORD>",
                UNITS[2]: r"template int adjoint_backward<true, RIDE_PARAM_SERIES, NO_RECORD>"}
    for unit, pattern in instance.items():
        assert re.search(pattern, open(os.path.join(CSRC, unit + ".hip")).read()), unit
    # the library holds the kernels of the three units: the three families instantiated at RIDE_PARAM_SERIES (the fifth value of
    # trm::Ride: a mangled name spells the template arguments <HYD, LPC, (trm::Ride)4> as ILi<h>ELi<lpc>ELNS_4RideE4E) ...
    blob = open(trm._capi.LIB_PATH, "rb").read()
    for family in (b"k_column_tangent", b"k_column_adjoint", b"k_column_adjoint_ckpt"):
        kernel = b"%d%sILi\\d+ELi(32|64)ELNS_4RideE4E" % (len(family), family)
        assert re.search(kernel, blob), family
    # ... and exports what it exported: every name of EXPORTS, no trm_ symbol for the new ride
    lib = ctypes.CDLL(trm._capi.LIB_PATH)
    for name in trm._capi.EXPORTS:
        assert hasattr(lib, name), name
    assert not any("param_series" in name or "series_param" in name for name in trm._capi.EXPORTS)
    assert set(abi_header.functions()) == set(trm._capi.EXPORTS)


def test_python_signatures_are_unchanged():
    jvp, vjp = inspect.signature(trm.jvp).parameters, inspect.signature(trm.vjp).parameters
    assert list(jvp) == ["integ", "d_internal_energy", "steps", "d_boundary", "d_params"] and jvp["d_params"].default is None
    assert list(vjp) == ["integ", "steps", "temperature", "internal_energy", "liquid_water_fraction", "checkpoint_every", "wrt_boundary", "wrt_params"]
    assert vjp["wrt_params"].default is False and vjp["wrt_boundary"].default is False
    assert "derivative_series_params" in trm.jvp.__doc__ and "derivative_series_params" in trm.vjp.__doc__


def test_cases_are_the_series_cases_with_both_organic_contents():
    assert len(SERIES_CASES) == 36 and len(PS.CASES) == 72
    assert {c[:4] + c[5:] for c in PS.CASES} == {c[:4] + c[5:] for c in SERIES_CASES}
    assert {c[4] for c in PS.CASES} == {0.0, 26.0}


@pytest.mark.parametrize("case", PS.CASES, ids=case_id)
def test_reference_holds(case):
    ref = PS.reference(case)
    print(f"{case_id(case)}: kept {int(ref.keep.sum())}/{ref.keep.size}, e_ref = {ref.e_ref:.3e}, 8 x = {FACTOR * ref.e_ref:.3e}, "
          f"joint = {ref.parts['tangent joint']:.3e} (ceiling {ref.joint_ceiling:.3e}), organic blocks max |J| = {ref.organic:.3e}")
    for label, err in ref.parts.items():
        print(f"    {label}: e_ref = {err:.3e}")
    assert ref.keep.all()
    assert 0.0 < FACTOR * ref.e_ref <= BROKEN
    assert ref.parts["tangent joint"] <= ref.joint_ceiling
    assert set(PS.contractions(case, ref.inputs[5])) | {"tangent joint"} == set(ref.parts)
    if case[4] == 26.0:
        assert ref.organic > 0.0
    else:
        assert ref.organic == 0.0
