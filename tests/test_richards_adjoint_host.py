"""The heat + Richards adjoint without a GPU: the option, the two cotangent ids and the program family in the header and in the Python
tables; the reference of the GPU tests (tests/richards_adjoint_cases.py) held to its own conditions on every case; its consistency with
the tangent side; and the refusals of trm.vjp that need no device."""
import inspect
import types

import numpy as np
import pytest

import abi_header as H
import linearised_richards as LR
import richards_adjoint_cases as RA
import richards_cases as RC
import terrarium_jl_amd as trm

CAPI = trm._capi
LD = np.longdouble
TAPE_ONLY = "on a Richards context: final-state cotangents on a per-step tape only"
# the shapes whose reference was measured when the helper was written: Nz 3, 33 and 64 with 13 columns, all hydraulics and boundary sets,
# both repair cases -- largest e_ref 2.26e-12 (Nz33 default), 13 of 13 columns kept
MEASURED_LARGEST_E_REF = 2.26e-12


def test_header_and_tables_agree():
    enum = H.enums()
    assert enum["TRM_OPT_DERIVATIVE_RICHARDS_ADJOINT"] == 17 == CAPI.OPTION["derivative_richards_adjoint"]
    assert enum["TRM_ADJOINT_SATURATION"] == 3 == CAPI.ADJOINT["saturation"] and enum["TRM_ADJOINT_PRESSURE_HEAD"] == 4 == CAPI.ADJOINT["pressure_head"]
    for field in ("INTERNAL_ENERGY", "TEMPERATURE", "LIQUID_WATER_FRACTION", "SATURATION", "PRESSURE_HEAD"):
        assert enum["TRM_ADJOINT_" + field] == enum["TRM_TANGENT_" + field] == CAPI.ADJOINT[field.lower()] == CAPI.TANGENT[field.lower()], field
    family = "column_adjoint_richards"
    assert enum["TRM_PROGRAM_" + family.upper()] == 17 == CAPI.PROGRAM.index(family)
    assert H.defines()["TRM_ABI_VERSION"] == 20
    assert len(H.functions()) == len(CAPI.EXPORTS) == 122
    assert TAPE_ONLY in H.text() and "on a Richards context: state seeds only" in H.text()


def test_decode_program_names_the_family():
    d = CAPI.decode_program(17 | 1 << 8 | 2 << 10)
    assert d["family"] == "column_adjoint_richards" and d["hydraulics"] == "vg_n2" and d["lanes_per_column"] == 64
    d = CAPI.decode_program(17 | 2 << 8 | 1 << 10)
    assert d["hydraulics"] == "generic" and d["lanes_per_column"] == 32
    assert "backward" not in d and "boundary_gradient" not in d and "parameter_gradient" not in d
    # no existing id decodes differently
    assert CAPI.decode_program(15)["family"] == "column_adjoint" and CAPI.decode_program(16)["family"] == "column_tangent_richards"


@pytest.mark.parametrize("case", RA.CASES, ids=RA.case_id)
def test_reference_conditions(case):
    """what the GPU tests rely on: the bound 8 x e_ref of the case lies in (0, BROKEN], and all but two of 13 columns are compared"""
    ref = RA.reference(case)
    bound = ref.bound(RA.BROKEN)
    dense = ref.parts["dense"]
    print(f"{RA.case_id(case)}: e_ref = {ref.e_ref:.3e}, bound = {bound:.3e}, dense = {dense:.3e}, kept {int(ref.keep.sum())}/{ref.keep.size}")
    assert 0.0 < bound <= RA.BROKEN == 8.0 * 4.0 * 3.9e-12
    assert ref.keep.sum() >= ref.keep.size - 2 and ref.keep.any()
    assert len(ref.parts) == 1 + 5 * len(RA.one_hot_levels(case[0])) <= 21
    for label, (g, S) in ref.expected.items():
        assert g.shape == S.shape == (2 * case[0], int(ref.keep.sum())), label
        assert np.all(np.isfinite(g.astype(np.float64))) and np.all(S >= 0), label


def test_the_measured_cases_keep_their_figures():
    """the figures the helper was written with (an e_ref far above them would be a changed reference, not rounding)"""
    worst = max(RA.reference(case).e_ref for case in RA.CASES if case[0] in (3, 33, 64) and case[1] == 13)
    assert worst <= 4.0 * MEASURED_LARGEST_E_REF, worst


@pytest.mark.parametrize("case", [(3, 13, "default", "repair"), (33, 13, "generic", "T_top+flux_bottom"), (2, 1, "vg_n2", "infiltration_top")], ids=RA.case_id)
def test_consistent_with_the_tangent_side(case):
    """g_ref of a one-hot cotangent is the matching row of J, and <w, J v> = <g_ref, v> in extended precision for the dense pair"""
    ref = RA.Reference(case, jacobian=True)
    Nz = case[0]
    for x, name in enumerate(LR.FIELDS):
        for i in RA.one_hot_levels(Nz):
            g, _ = ref.expected[f"one-hot {name} {i}"]
            assert np.array_equal(g, ref.J[x, i]), (name, i)
    w = RA.cotangents(case)["dense"][..., ref.keep].astype(LD)
    v = RC.inputs(case)[4][:, ref.keep].astype(LD)
    Jv = np.einsum(RC.AXES, ref.J, v)
    g, S = ref.expected["dense"]
    left, right = np.sum(w * Jv, axis=(0, 1)), np.sum(g * v, axis=0)
    scale = np.sum(S * np.abs(v), axis=0)
    assert np.all(np.abs(left - right) <= 64 * np.finfo(LD).eps * scale), (left, right)
    assert np.all(scale > 0)


def test_a_schedule_of_one_stretch_is_the_plain_run():
    case = (3, 13, "default", "infiltration_top")
    a, b = RA.reference(case), RA.Reference(case, schedule=[(RA.DT, 2), (RA.DT, RA.STEPS - 2)])
    assert np.array_equal(a.keep, b.keep) and a.e_ref == b.e_ref
    for label in a.expected:
        assert np.array_equal(a.expected[label][0], b.expected[label][0]), label


def _integrator(richards):
    """what vjp reads of an integrator before it touches the device"""
    flow = trm.RichardsEq() if richards else object()
    model = types.SimpleNamespace(soil=types.SimpleNamespace(hydrology=types.SimpleNamespace(vertical_flow=flow)))
    return types.SimpleNamespace(model=model, timestepper=trm.ForwardEuler(dt=60.0), state=None, boundary_conditions={},
                                 _has_time_dependence=lambda: False, _windowed=lambda: False)


def test_vjp_refusals_that_need_no_device():
    # (the signature of vjp is pinned by earlier tests: the two new cotangents travel in a dict of cotangents, as jvp's saturation seed does)
    assert list(inspect.signature(trm.vjp).parameters)[:5] == ["integ", "steps", "temperature", "internal_energy", "liquid_water_fraction"]
    assert "derivative_richards_adjoint" in trm.vjp.__doc__ and '"saturation"' in trm.vjp.__doc__ and '"pressure_head"' in trm.vjp.__doc__
    for doc in (trm.DeviceState.set_cotangent.__doc__, trm.DeviceState.cotangent.__doc__):
        assert "saturation" in doc
    heat, rich = _integrator(False), _integrator(True)
    for name in ("saturation", "pressure_head"):
        with pytest.raises(ValueError, match="need an integrator with RichardsEq"):
            trm.vjp(heat, 1, internal_energy={name: 1.0})
    with pytest.raises(KeyError, match="hydraulic_conductivity"):
        trm.vjp(heat, 1, internal_energy={"hydraulic_conductivity": 1.0})
    with pytest.raises(ValueError, match="given twice"):
        trm.vjp(rich, 1, temperature=1.0, internal_energy={"temperature": 1.0})
    for kwargs in (dict(wrt_params=True), dict(wrt_boundary=True), dict(checkpoint_every=2)):
        with pytest.raises(ValueError, match="on an integrator with RichardsEq"):
            trm.vjp(rich, 1, internal_energy={"saturation": 1.0}, **kwargs)
