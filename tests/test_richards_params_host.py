"""The hydraulic-parameter gradients of the heat + Richards adjoint without a GPU: the option, the seven ids and the Python tables against
the header; the reference of the GPU tests (tests/linearised_richards_params.py) held to its own conditions on every case -- the state
block of its Jacobian is linearised_richards' bit for bit, every non-repair case keeps all its columns, every bound lies under the
ceiling, the parameters the hydraulics never read have exactly zero columns -- and its parameter columns against Richardson-extrapolated
finite differences of the unseeded extended-precision restatement."""
import numpy as np
import pytest

import abi_header as H
import linearised_richards as LR
import linearised_richards_params as LP
import richards_cases as RC
import terrarium_jl_amd as trm

CAPI = trm._capi
LD = np.longdouble


def test_header_and_tables_agree():
    enum = H.enums()
    assert enum["TRM_OPT_DERIVATIVE_RICHARDS_PARAMS"] == 18 == CAPI.OPTION["derivative_richards_params"]
    assert H.table("TRM_HYDRAULIC_PARAM_") == {**{name.lower(): which for name, which in CAPI.HYDRAULIC_PARAMS.items()}, "count": len(CAPI.HYDRAULIC_PARAMS)}
    assert tuple(CAPI.HYDRAULIC_PARAMS) == LP.PARAMS == ("K_sat", "theta_res", "bc_psi_s", "bc_lambda", "vg_alpha", "vg_n", "impedance")
    # one id space with the thermal ids, in the order of trm_params' hydraulics line
    assert list(CAPI.HYDRAULIC_PARAMS.values()) == list(range(enum["TRM_THERMAL_PARAM_COUNT"], enum["TRM_THERMAL_PARAM_COUNT"] + enum["TRM_HYDRAULIC_PARAM_COUNT"]))
    assert enum["TRM_HYDRAULIC_PARAM_K_SAT"] == 10 and enum["TRM_HYDRAULIC_PARAM_IMPEDANCE"] == 16 and enum["TRM_HYDRAULIC_PARAM_COUNT"] == 7
    fields = [name for name, *_ in CAPI.default_params()._fields_]
    at = [fields.index(name) for name in LP.PARAMS]
    assert at == sorted(at), "the ids follow the order of trm_params"
    assert H.defines()["TRM_ABI_VERSION"] == 20
    assert len(H.functions()) == len(CAPI.EXPORTS) == 122
    for text in ("TRM_OPT_DERIVATIVE_RICHARDS_PARAMS", "does NOT imply", "Kcbar dKc/dp + psibar dpsi/dp", "on a Richards context: final-state cotangents on a per-step tape only"):
        assert text in H.text(), text


def test_decode_program_reports_the_bit_under_its_own_key():
    bit = CAPI.PROGRAM_PARAMETERS
    d = CAPI.decode_program(17 | 1 << 8 | 2 << 10 | bit)
    assert d["family"] == "column_adjoint_richards" and d["hydraulics"] == "vg_n2" and d["lanes_per_column"] == 64
    assert d["hydraulic_parameter_gradient"] is True and "parameter_gradient" not in d
    # (the id arrives as a C int: negative with bit 31)
    assert CAPI.decode_program((17 | 2 << 8 | 1 << 10 | bit) - (1 << 32)) == {**CAPI.decode_program(17 | 2 << 8 | 1 << 10), "hydraulic_parameter_gradient": True}
    for family in range(len(CAPI.PROGRAM)):
        assert "hydraulic_parameter_gradient" not in CAPI.decode_program(family | 1 << 10), family
        assert ("hydraulic_parameter_gradient" in CAPI.decode_program(family | 1 << 10 | bit)) == (family == 17), family


def test_python_surface():
    assert trm.hydraulic_parameter_gradient.__doc__ and "derivative_richards_params" in trm.hydraulic_parameter_gradient.__doc__
    for doc in (trm.DeviceState.open_param_gradient.__doc__, trm.DeviceState.param_gradient.__doc__):
        assert "HYDRAULIC_PARAMS" in doc


def _same_state_block(case, ref):
    """the state block of the Jacobian with the parameter seeds present is linearised_richards' own, bit for bit; the pressure-head rows of
    a repair case's dry columns, where the head is infinite, are non-finite here and stay out"""
    own, _ = LP.split(ref.J, case[0])
    theirs = RC.restatement(case, LD).jacobian()
    out = ~np.isfinite(own.astype(np.float64))
    if case[3] != "repair" and out.any():
        return False
    x, _, _, col = np.nonzero(out)
    return np.array_equal(own[~out], theirs[~out]) and set(x) <= {LR.FIELDS.index("pressure_head")} and set(col) <= set(range(7, 13))


@pytest.mark.parametrize("case", LP.CASES, ids=LP.case_id)
def test_reference_conditions(case):
    """what the GPU tests rely on"""
    ref = LP.reference(case)
    bound = LP.bound(case)
    print(f"{LP.case_id(case)}: e_ref = {ref.e_ref:.3e}, bound = {bound:.3e}, dense = {ref.parts['dense']:.3e}, kept {int(ref.keep.sum())}/{ref.keep.size}")
    assert 0.0 < bound <= LP.CEILING == 8.0 * 4.0 * 3.5e-11
    assert 0.0 < ref.e_ref <= LP.LARGEST_E_REF[0], "LARGEST_E_REF is the largest this module gives"
    if case[3] != "repair":
        assert ref.keep.all(), "every non-repair case keeps all its columns"
        assert not ref.nonfinite.any()
        assert bound >= 8.0 * 2e-14, "a pooled e_ref samples more than one column"
    else:
        assert ref.keep.sum() >= ref.keep.size - 2
        assert bound == 8.0 * ref.e_ref, "a repair case is the only one of its boundary set: its own e_ref"
        # exactly the pressure-head rows of exactly the dry columns are non-finite
        x, _, _, col = np.nonzero(ref.nonfinite)
        assert set(x) == {LR.FIELDS.index("pressure_head")} and set(np.arange(case[1])[ref.keep][col]) == set(range(7, 13)) & set(np.arange(case[1])[ref.keep])
    for label, (g, S) in ref.expected.items():
        assert g.shape == S.shape == (len(LP.PARAMS), int(ref.keep.sum())), label
        assert np.all(np.isfinite(g.astype(np.float64))) and np.all(S >= 0), label
        # a parameter the hydraulics never read: exact zeros
        for name in LP.unread(case[2]):
            q = LP.PARAMS.index(name)
            assert np.all(g[q] == 0) and np.all(S[q] == 0), (label, name)
        # ... and one they read reaches the dense cotangent (13 columns: every regime occurs; impedance needs a cell with ice)
        for name in set(LP.PARAMS) - set(LP.unread(case[2])) if case[1] == RC.NH else ():
            assert np.any(ref.expected["dense"][1][LP.PARAMS.index(name)] > 0), name


def test_the_largest_e_ref_is_the_stated_one():
    worst = max(LP.CASES, key=lambda case: LP.reference(case).e_ref)
    e = LP.reference(worst).e_ref
    print(f"largest parameter e_ref: {e:.3e} ({LP.case_id(worst)})")
    assert LP.case_id(worst) == LP.LARGEST_E_REF[1] and e <= LP.LARGEST_E_REF[0] < 1.1 * e


FD_CASES = [(3, 13, "default", "T_top+flux_bottom"), (3, 13, "generic", "T_top+flux_bottom"), (33, 13, "vg_n2", "infiltration_top"), (33, 13, "default", "repair")]


def _fd(case, name, step):
    """(F(p + step) - F(p - step)) / (2 step) of the five final fields, the parameter carried as a longdouble: [5][Nz][Nh]"""
    p, U0, sat, bcs, _ = RC.inputs(case)
    out = []
    for sign in (1, -1):
        q = LP.carried(p, name, LD(getattr(p, name)) + sign * step)
        r = LR.run([RC.DZ] * case[0], U0, sat, bcs, q, RC.DT, RC.STEPS, dtype=LD, seeded=False)
        out.append(np.stack([r.final[field].x for field in LR.FIELDS]))
    with np.errstate(invalid="ignore"):
        return (out[0] - out[1]) / (2 * step)


@pytest.mark.parametrize("case", FD_CASES, ids=LP.case_id)
def test_parameter_columns_match_finite_differences(case):
    """J_p against (4 fd(h/2) - fd(h)) / 3 of the unseeded extended-precision restatement, h = 1e-3 x the parameter (5e-5 for
    theta_res = 0): within 1e-8 of the field's largest entry.  Worst with this module: 5.4e-10 (Nz33 repair), 2.8e-11 elsewhere (Nz3 generic)."""
    ref = LP.Reference(case, jacobian=True)
    assert _same_state_block(case, ref)
    _, Jp = LP.split(ref.J, case[0])
    p = RC.inputs(case)[0]
    worst = 0.0
    for q, name in enumerate(LP.PARAMS):
        if name in LP.unread(case[2]):
            column = Jp[:, :, q]
            assert np.all(column[np.isfinite(column.astype(np.float64))] == 0), name
            continue
        value = LD(getattr(p, name))
        h = LD(1e-3) * value if value != 0 else LD(5e-5)
        fd = (4 * _fd(case, name, h / 2) - _fd(case, name, h)) / 3
        for x, field in enumerate(LR.FIELDS):
            own, other = Jp[x, :, q], fd[x]
            finite = np.isfinite(own.astype(np.float64))
            assert finite.all() or (case[3] == "repair" and field == "pressure_head")
            scale = np.max(np.abs(own[finite]))
            if scale == 0:
                assert np.all(other[finite] == 0), (name, field)
                continue
            err = float(np.max(np.abs(own[finite] - other[finite])) / scale)
            worst = max(worst, err)
            assert err <= 1e-8, (LP.case_id(case), name, field, err)
    print(f"{LP.case_id(case)}: worst finite-difference disagreement {worst:.2e}")


@pytest.mark.parametrize("case", [(2, 1, "vg_n2", "infiltration_top"), (64, 13, "generic", "T_top+flux_bottom")], ids=LP.case_id)
def test_state_block_is_the_state_restatement(case):
    assert _same_state_block(case, LP.Reference(case, jacobian=True))
