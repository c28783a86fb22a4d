"""Soil-moisture records on the heat + Richards adjoint without a GPU: the option against the header and the binding, the reference of
the GPU tests (tests/richards_record.py) held to its own conditions on every case -- every column kept, every bound derived and under
its ceiling -- a one-sample record against the matching row of the Jacobian, the adjoint identity in extended precision, the parameter
part against Richardson-extrapolated finite differences of the extended-precision misfit, and the Python surface."""
import numpy as np
import pytest

import abi_header as H
import linearised_richards as LR
import linearised_richards_params as LRP
import richards_adjoint_cases as RA
import richards_cases as RC
import richards_record as RR
import terrarium_jl_amd as trm

CAPI = trm._capi
LD = np.longdouble


def test_header_and_tables_agree():
    enum = H.enums()
    assert enum["TRM_OPT_DERIVATIVE_RICHARDS_RECORD"] == 19 == CAPI.OPTION["derivative_richards_record"]
    assert enum["TRM_OPT_DERIVATIVE_RICHARDS_ADJOINT"] == 17 and enum["TRM_OPT_DERIVATIVE_RICHARDS_PARAMS"] == 18
    assert H.defines()["TRM_ABI_VERSION"] == 20
    assert len(H.functions()) == len(CAPI.EXPORTS) == 122
    for text in ("TRM_OPT_DERIVATIVE_RICHARDS_RECORD", "saturation_water_ice", "sat_{p_k}[level_j] - sat_obs", "not even the sign of a zero",
                 "on a Richards context: final-state cotangents on a per-step tape only"):
        assert text in H.text(), text


def test_the_cases_are_the_stated_ones():
    assert len(RR.GROUPS["edges"]) == 6 * 3 * 2 + 2 and len(RR.GROUPS["dense"]) == 2 * 3 + 2 and len(RR.GROUPS["ends"]) == 6
    assert {(c[0], c[1]) for c in RR.GROUPS["edges"]} == set(RR.EDGE_SHAPES)
    assert sum(c[3] == "repair" for c in RR.GROUPS["edges"]) == 2 and sum(c[3] == "repair" for c in RR.GROUPS["dense"]) == 2
    assert {(c[0], c[1], c[2]) for c in RR.GROUPS["dense"]} == {(3, 13, "default"), (33, 13, "default"), (64, 1, "generic")}
    # six steps in launches of 4 and 2: positions 3 and 5 inside a launch, 0 the last launch's last step, 6 the fold's
    assert (RR.STEPS, RR.SPL, RR.POSITIONS) == (6, 4, (0, 3, 5, 6))
    for rcase in RR.CASES:
        assert RR.positions_of(rcase)[-1] == RR.STEPS and RR.levels_of(rcase)[-1] == rcase[1][0] - 1


@pytest.mark.parametrize("rcase", RR.CASES, ids=RR.record_id)
def test_reference_conditions(rcase):
    """what the GPU tests rely on"""
    ref = RR.reference(rcase)
    case = rcase[1]
    Nz, kept = case[0], int(ref.keep.sum())
    figures = ", ".join(f"{part} {ref.e_ref[part]:.2e} (bound {RR.bound(rcase, part):.2e})" for part in RR.PARTS)
    print(f"{RR.record_id(rcase)}: e_ref {figures}, kept {kept}/{ref.keep.size}")
    assert ref.keep.all(), "every case keeps all its columns"
    rec = ref.record
    npos, nlevels = len(RR.positions_of(rcase)), len(RR.levels_of(rcase))
    assert rec["observed"].shape == rec["weight"].shape == (npos, nlevels, case[1])
    moved = np.abs(rec["observed"] - np.stack(ref.sat_narrow))
    assert np.all((moved > 0.02 - 1e-12) & (moved < 0.08 + 1e-12)) and np.all((rec["weight"] >= 0.5) & (rec["weight"] <= 2.0))
    for part in RR.PARTS:
        b = RR.bound(rcase, part)
        assert 0.0 < b <= RR.ceiling(part), part
        existing = LRP.bound(case) if part == "params" else RA.reference(case).bound()
        assert b >= existing and b >= RR.FACTOR * ref.e_ref[part], "the larger of the two e_ref"
        for variant in RR.VARIANTS:
            g, S = ref.expected[(part, variant)]
            assert g.shape == S.shape == {"state": (2 * Nz, kept), "params": (len(RR.PARAMS), kept), "misfit loss": (kept,)}[part]
            assert np.all(np.isfinite(g.astype(np.float64))) and np.all(S >= 0)
    assert RR.ceiling("state") == RA.BROKEN and RR.ceiling("params") == LRP.CEILING
    # the loss does not depend on the final cotangents, and it is positive: every sample is off by 0.02 or more
    a, b = (ref.expected[("misfit loss", variant)][0] for variant in RR.VARIANTS)
    assert np.array_equal(a, b) and np.all(a > 0)
    # a parameter the hydraulics never read: exact zeros; one they read reaches the record (13 columns)
    for variant in RR.VARIANTS:
        g, S = ref.expected[("params", variant)]
        for name in LRP.unread(case[2]):
            q = RR.PARAMS.index(name)
            assert np.all(g[q] == 0) and np.all(S[q] == 0), name
    assert np.any(ref.expected[("params", "record")][1][RR.PARAMS.index("K_sat")] > 0) or case[1] == 1
    assert np.any(ref.expected[("state", "record")][1][Nz:] > 0), "the record reaches the initial saturation"


ONE_SAMPLE = [("edges", (3, 13, "generic", "infiltration_top")), ("edges", (33, 13, "default", "repair")), ("ends", (2, 13, "vg_n2", "T_top+flux_bottom"))]


@pytest.mark.parametrize("rcase", ONE_SAMPLE, ids=RR.record_id)
def test_one_sample_gives_the_matching_row_of_the_jacobian(rcase):
    drawn = RR.reference(rcase).record
    Nz = rcase[1][0]
    for k, j in ((0, 0), (len(drawn["positions"]) - 1, len(drawn["levels"]) - 1), (len(drawn["positions"]) // 2, 0)):
        weight = np.zeros_like(drawn["weight"])
        weight[k, j] = drawn["weight"][k, j]
        observed = drawn["observed"].copy()
        observed[0, -1] = np.nan if (k, j) != (0, len(drawn["levels"]) - 1) else observed[0, -1]        # (a gap beside it changes nothing)
        ref = RR.RecordReference(rcase, jacobians=True, record=dict(drawn, weight=weight, observed=observed))
        row = ref.J[k][RR.SAT][drawn["levels"][j]][..., ref.keep]                                     # [2 Nz + 7][kept]
        expected = row * ref.cot_wide[k][j][ref.keep]
        state, params = ref.expected[("state", "record")][0], ref.expected[("params", "record")][0]
        assert np.array_equal(state, expected[:2 * Nz]) and np.array_equal(params, expected[2 * Nz:]), (k, j)
        assert np.any(state != 0)


@pytest.mark.parametrize("rcase", ONE_SAMPLE + [("dense", (3, 13, "default", "T_top+flux_bottom"))], ids=RR.record_id)
def test_adjoint_identity_in_extended_precision(rcase):
    """sum_k <w_k r_k, J_s v> + <final, J_n v> = <g_ref, v> for the dense state seed of the case: the two orders of one triple sum, equal
    to the rounding of np.longdouble (1.1e-19) times the number of terms -- 1e-16 S is far above that and far below fp64 rounding"""
    ref = RR.RecordReference(rcase, jacobians=True, record=RR.reference(rcase).record)
    case = rcase[1]
    Nz, keep, levels = case[0], ref.keep, ref.record["levels"]
    v = RC.inputs(case)[4][:, keep].astype(LD)
    for variant in RR.VARIANTS:
        final = RR.final_cotangent(case, variant)[..., keep].astype(LD)
        Jn = np.where(np.isfinite(ref.J[-1].astype(np.float64)), ref.J[-1], LD(0))
        forward = np.einsum("xic,xijc,jc->c", final, Jn[:, :, :2 * Nz][..., keep], v)
        for k in range(len(ref.record["positions"])):
            forward = forward + np.einsum("ic,ijc,jc->c", ref.cot_wide[k][:, keep], ref.J[k][RR.SAT][levels][:, :2 * Nz][..., keep], v)
        backward, S = ref.identity[variant]
        assert np.all(S > 0) and np.all(np.abs(forward - backward) <= LD(1e-16) * S), (variant, float(np.max(np.abs(forward - backward) / S)))


FD_CASES = [("edges", (3, 13, "default", "T_top+flux_bottom")), ("edges", (33, 13, "vg_n2", "infiltration_top")), ("dense", (3, 13, "default", "repair"))]


def _misfit(rcase, record, name, value):
    """the extended-precision misfit per column with the parameter `name` carried as `value`"""
    case = rcase[1]
    p, U0, sat, bcs, _ = RC.inputs(case)
    q = LRP.carried(p, name, value)
    total = 0
    for k, s in enumerate(record["positions"]):
        r = LR.run([RC.DZ] * case[0], U0, sat, bcs, q, RC.DT, s, dtype=LD, seeded=False)
        total = total + np.sum(LD(0.5) * record["weight"][k].astype(LD) * (r.final["saturation"].x[record["levels"]] - record["observed"][k].astype(LD)) ** 2, axis=0)
    return total


@pytest.mark.parametrize("rcase", FD_CASES, ids=RR.record_id)
def test_parameter_part_matches_finite_differences_of_the_misfit(rcase):
    """g_ref of the record alone against (4 fd(h/2) - fd(h)) / 3 of the unseeded extended-precision misfit, h = 1e-3 x the parameter (5e-5
    for theta_res = 0), the scheme and the tolerance rule of test_richards_params_host.py: within 1e-8 of the gradient's largest entry.
    Worst with this module: 1.2e-10 (dense Nz3 repair), 2.5e-12 elsewhere (edges Nz33 vg_n2)."""
    ref = RR.reference(rcase)
    case, rec = rcase[1], ref.record
    p = RC.inputs(case)[0]
    g = ref.expected[("params", "record")][0]
    worst = 0.0
    for q, name in enumerate(RR.PARAMS):
        if name in LRP.unread(case[2]):
            assert np.all(g[q] == 0), name
            continue
        value = LD(getattr(p, name))
        h = LD(1e-3) * value if value != 0 else LD(5e-5)
        fd = lambda step: (_misfit(rcase, rec, name, value + step) - _misfit(rcase, rec, name, value - step)) / (2 * step)
        other = ((4 * fd(h / 2) - fd(h)) / 3)[ref.keep]
        scale = np.max(np.abs(g[q]))
        assert scale > 0, name
        err = float(np.max(np.abs(g[q] - other)) / scale)
        worst = max(worst, err)
        assert err <= 1e-8, (RR.record_id(rcase), name, err)
    print(f"{RR.record_id(rcase)}: worst finite-difference disagreement {worst:.2e}")


def test_soil_moisture_record_validation():
    values = np.full((2, 3, 4), 0.5)
    rec = trm.SoilMoistureRecord([0, 6], [0, 1, 5], values, weight=2.0)
    assert isinstance(rec, trm.TemperatureRecord) and rec.steps == [0, 6] and rec.levels.dtype == np.int32 and rec.weight.shape == values.shape
    assert trm.SoilMoistureRecord([3], [2], np.zeros((1, 1, 7))).weight is None
    with pytest.raises(ValueError, match=r"SoilMoistureRecord: values must be \[len\(steps\)\]\[len\(levels\)\]\[Nh\]"):
        trm.SoilMoistureRecord([0, 6], [0, 1], values)
    with pytest.raises(ValueError, match="SoilMoistureRecord: values must be"):
        trm.SoilMoistureRecord([0, 6], [0, 1, 5], values[0])
    with pytest.raises(ValueError, match="SoilMoistureRecord: steps must be >= 0 and non-decreasing"):
        trm.SoilMoistureRecord([6, 0], [0, 1, 5], values)
    with pytest.raises(ValueError, match="SoilMoistureRecord: steps must be >= 0"):
        trm.SoilMoistureRecord([-1, 0], [0, 1, 5], values)


def test_python_surface():
    for thing in (trm.soil_moisture_gradient, trm.SoilMoistureRecord, trm.DeviceState.attach_record, trm.DeviceState.detach_record,
                  trm.DeviceState.record_misfit, trm.DeviceState.record_residuals):
        assert thing.__doc__ and "derivative_richards_record" in thing.__doc__, thing
    assert "derivative_richards_adjoint" in trm.soil_moisture_gradient.__doc__ and "derivative_richards_params" in trm.soil_moisture_gradient.__doc__
    # the drivers that were there keep their words
    assert "derivative_richards_record" not in trm.record_gradient.__doc__ and "derivative_richards_record" not in trm.vjp.__doc__
