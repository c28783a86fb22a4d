"""The reference of the heat + Richards tangent tests, pinned on the CPU: tests/linearised_richards.py against the wide oracle (its primal,
at every step of every case, field by field), against Richardson-extrapolated central differences of the fp64 oracle on the reference's
own shape (its Jacobian), against the reference's two analytic answers, its own fp64 rounding e_ref per case (what the GPU test takes its
bound from), the branch mask of every case, and what the repair cases are for."""
import functools

import numpy as np
import pytest

import linearised_richards as LR
import richards_cases as RC
import terrarium_jl_amd as trm
from richards_cases import DT, DZ, LD, STEPS, case_id

# The largest difference between the restatement and oracle.Oracle(dtype = np.longdouble), both in np.longdouble, per field and relative to
# the field's largest value, over every case of the GPU test and every step -- measured with this test (pytest -s prints the figures): one
# unit in the last place of np.longdouble on the saturation and the pressure head, 0 on the other fields.  The two evaluate the same
# expressions (no organic matter: the conductivity and heat-capacity sums associate alike) and both take their powers from the C
# library's powl; the sums of the repair associate differently.  The bound is 16 x the measurement (bit for bit where that is 0).
MEASURED_PRIMAL_DIFFERENCE = dict(dict.fromkeys(LR.FIELDS + ("water_table", "surface_excess_water"), 0.0), saturation=5.43e-20, pressure_head=2.96e-20)
# The largest e_ref over the cases, measured with test_every_case_has_a_bound_and_keeps_its_columns (Nz31-Nh13-default-infiltration_top);
# the GPU test's ceiling on a bound (BROKEN) is set from it.
MEASURED_LARGEST_E_REF = 3.9e-12
ORACLE_NAME = dict(saturation="saturation_water_ice")


def oracle_on(dz, Nh, p, U0, sat, bcs, dtype=np.float64):
    import oracle
    o = oracle.Oracle(Nh, np.asarray(dz, dtype=np.float64), oracle.default_params(flow=1, swrc=p.swrc, unsat_k=p.unsat_k, vg_n=p.vg_n, K_sat=p.K_sat,
                                                                                   por_mineral=p.por_mineral), dtype=dtype)
    o.set("saturation_water_ice", sat)
    o.set("internal_energy", U0)
    for (var, side), (kind, value) in bcs.items():
        o.set_bc(var, side, kind, value)
    o.closure()
    return o


def test_primal_is_the_wide_oracles():
    import oracle
    if not oracle.wide_available():
        pytest.skip("np.longdouble is not wider than float64 here")
    worst = dict.fromkeys(MEASURED_PRIMAL_DIFFERENCE, 0.0)
    for case in RC.CASES:
        p, U0, sat, bcs, _ = RC.inputs(case)
        mine = RC.restatement(case, LD, seeded=False)
        o = oracle_on([DZ] * case[0], case[1], p, U0, sat, bcs, dtype=LD)
        for step in range(STEPS + 1):
            for x in worst:
                a, b = o.get(ORACLE_NAME.get(x, x)), mine.trajectory[step][x]
                finite = np.isfinite(a)            # (the head of a cell the last step of a repair case drained to zero is -inf in both)
                assert np.array_equal(finite, np.isfinite(b)) and np.array_equal(a[~finite], b[~finite]), (case_id(case), x, step)
                if np.any(a[finite] != 0):
                    worst[x] = max(worst[x], float(np.max(np.abs(a - b)[finite]) / np.max(np.abs(a[finite]))))
            if step < STEPS:
                o.timestep(DT)
    for x in worst:
        print(f"restatement against the wide oracle, {x}: largest difference / field maximum = {worst[x]:.3e} (bound {16.0 * MEASURED_PRIMAL_DIFFERENCE[x]:.3e})")
    for x in worst:
        assert worst[x] <= 16.0 * MEASURED_PRIMAL_DIFFERENCE[x], x


# ---- central differences of the fp64 oracle on the reference's shape: ExponentialSpacing(N = 10), dt = 60 ------------------------------
FD_NH, FD_STEPS = 13, 6
# the largest step per direction (times a direction of 1e3 J/m3 or 1e-3 of saturation per cell): small enough that no cell changes a branch
# between -h and h -- a saturation moved by 1e-3 switches a face minimum of the van Genuchten conductivity in one of the 13 columns
FD_H = {"U": 1.0, "sat": 0.25}


@functools.lru_cache(maxsize=None)
def fd_inputs(hyd):
    """a column that is smooth in the saturation (the top layers are 5 and 12 cm thick: a rough profile is stiff there), mixed in the regimes"""
    dz = np.asarray(trm.ExponentialSpacing(N=10).get_spacing(), dtype=np.float64)
    p = RC.params(hyd)
    rng = np.random.default_rng(11)
    U0, _ = RC.mixed_state(10, FD_NH, p, 11)
    sat = 0.75 + 0.1 * np.sin(np.linspace(0.0, 3.0, 10))[:, None] + rng.uniform(-0.01, 0.01, (10, FD_NH))
    bcs = {pair: (kind, np.broadcast_to(np.asarray(v, dtype=np.float64), (FD_NH,)).copy()) for pair, (kind, v) in RC.boundary_sets(FD_NH)["T_top+flux_bottom"].items()}
    w = {x: rng.normal(0.0, 1.0, (10, FD_NH)) for x in LR.FIELDS}
    directions = {"U": np.concatenate([rng.normal(0.0, 1e3, (10, FD_NH)), np.zeros((10, FD_NH))]),
                  "sat": np.concatenate([np.zeros((10, FD_NH)), rng.normal(0.0, 1e-3, (10, FD_NH))])}
    return dz, p, U0, sat, bcs, w, directions


def fd_central(hyd, v, h):
    dz, p, U0, sat, bcs, _, _ = fd_inputs(hyd)

    def final(sign):
        o = oracle_on(dz, FD_NH, p, U0 + sign * h * v[:10], sat + sign * h * v[10:], bcs)
        for _ in range(FD_STEPS):
            o.timestep(DT)
        return {x: o.get(ORACLE_NAME.get(x, x)).astype(LD) for x in LR.FIELDS}
    plus, minus = final(1.0), final(-1.0)
    return {x: (plus[x] - minus[x]) / (2.0 * LD(h)) for x in LR.FIELDS}


@pytest.mark.parametrize("hyd", RC.HYDRAULICS)
def test_jacobian_matches_central_differences_of_the_oracle(hyd):
    """the method of test_parameter_gradient_host.py: the Richardson extrapolations at (h, h / 2) and (h / 2, h / 4) of the loss
    sum w . field must agree to 1e-8 of S = sum |w| |fd| first; then the restatement's J v is within 1e-6 of S of the finer one"""
    dz, p, U0, sat, bcs, w, directions = fd_inputs(hyd)
    wide = LR.run(dz, U0, sat, bcs, p, DT, FD_STEPS, dtype=LD)
    keep = LR.kept_columns(wide, LR.run(dz, U0, sat, bcs, p, DT, FD_STEPS, dtype=np.float64))
    assert keep.sum() >= FD_NH - 2
    J = wide.jacobian()
    for name, v in directions.items():
        c = [fd_central(hyd, v, FD_H[name] / 2 ** i) for i in range(3)]
        R = [{x: (4.0 * c[i + 1][x] - c[i][x]) / 3.0 for x in LR.FIELDS} for i in range(2)]
        loss = [sum(np.sum(w[x].astype(LD) * r[x], axis=0) for x in LR.FIELDS) for r in R]
        S = sum(np.sum(np.abs(w[x]).astype(LD) * np.abs(R[1][x]), axis=0) for x in LR.FIELDS)
        converged = float(np.max(np.abs(loss[0] - loss[1])[keep] / S[keep]))
        Jv = np.einsum(RC.AXES, J, v.astype(LD))
        mine = sum(np.sum(w[x].astype(LD) * Jv[n], axis=0) for n, x in enumerate(LR.FIELDS))
        err = float(np.max(np.abs(mine - loss[1])[keep] / S[keep]))
        print(f"{hyd} d/d{name}: |R(h, h/2) - R(h/2, h/4)| / S = {converged:.3e}, |J v - R| / S = {err:.3e}, {int(keep.sum())} columns")
        assert converged <= 1e-8, name
        assert err <= 1e-6, name
        # field by field, against the field's own scale per column; the floor is the rounding of the differences themselves: the oracle's
        # fields carry eps |X|, divided by the smallest step (h / 4) and weighted by the extrapolations (4 / 3 + 1 / 3 twice): 64 eps |X| / h
        for n, x in enumerate(LR.FIELDS):
            scale = np.max(np.abs(R[1][x]), axis=0)[keep]
            floor = 64 * np.finfo(np.float64).eps / FD_H[name] * np.max(np.abs(wide.trajectory[-1][x]), axis=0)[keep]
            assert np.all(np.max(np.abs(Jv[n] - R[1][x]), axis=0)[keep] <= 1e-6 * scale + floor), (name, x)


# ---- the reference's two analytic answers (test/differentiability/soil_hydrology_diff.jl) -------------------------------------------------
@pytest.mark.parametrize("hyd", ("default", "vg_n2"))
def test_pressure_slope_is_the_inverse_function_theorems(hyd):
    """at por = 0.5, sat = 0.5: dpsi / dsat = por / swrc'(psi_m), for both retention curves"""
    p = RC.params(hyd)
    p.por_mineral = 0.5
    r = LR.run([DZ] * 4, np.full((4, 2), 1e6), np.full((4, 2), 0.5), {}, p, DT, 0, dtype=LD)
    J = r.jacobian()[LR.FIELDS.index("pressure_head")]
    slope = RC.analytic_slope(p, 0.5)
    for i in range(4):
        assert np.all(np.abs(J[i, 4 + i] - slope) <= 64 * np.finfo(LD).eps * abs(slope)), (i, J[i, 4 + i], slope)
        assert np.all(np.delete(J[i], 4 + i, axis=0) == 0)
    # ... and the oracle's curve has that slope: a central difference of swrc_psi
    import oracle
    op = oracle.default_params(swrc=p.swrc, unsat_k=p.unsat_k, vg_n=p.vg_n)
    h = 1e-5
    fd = (oracle.scalar("swrc_psi", op, 0.5 * (0.5 + h), 0.5) - oracle.scalar("swrc_psi", op, 0.5 * (0.5 - h), 0.5)) / (2 * h)
    assert abs(fd - float(slope)) <= 1e-7 * abs(float(slope))


def test_van_genuchten_conductivity_slopes():
    """the van Genuchten conductivity (alpha = 1, n = 2) at (por, sat, liq) = (0.5, 0.75, 0.9) against central differences in sat and liq"""
    import oracle
    from linearised_heat import Dual
    p = RC.params("vg_n2")
    p.por_mineral = 0.5
    c = dict(por=LD(0.5))
    h = LR.hydraulics(p, LD)
    one = np.ones((1, 1), dtype=LD)
    sat = Dual(0.75 * one, np.array([[[1.0, 0.0]]], dtype=LD))
    liq = Dual(0.9 * one, np.array([[[0.0, 1.0]]], dtype=LD))
    K = LR.cell_conductivity(c, h, sat, liq)
    op = oracle.default_params(swrc=1, unsat_k=1, vg_n=2.0, vg_alpha=1.0, por_mineral=0.5)
    f = lambda s, l: oracle.scalar("hydraulic_conductivity", op, 0.5, s, l, 0.0)
    assert abs(f(0.75, 0.9) - float(K.x[0, 0])) <= 4 * np.finfo(np.float64).eps * float(K.x[0, 0])
    e = 1e-5
    fd_sat = (f(0.75 + e, 0.9) - f(0.75 - e, 0.9)) / (2 * e)
    fd_liq = (f(0.75, 0.9 + e) - f(0.75, 0.9 - e)) / (2 * e)
    print(f"dK/dsat = {float(K.d[0, 0, 0]):.9e} (central difference {fd_sat:.9e}), dK/dliq = {float(K.d[0, 0, 1]):.9e} ({fd_liq:.9e})")
    # (a central difference of step 1e-5 on a smooth function: truncation ~ e^2 = 1e-10 relative, rounding ~ eps / e = 2e-11)
    assert abs(fd_sat - float(K.d[0, 0, 0])) <= 1e-8 * abs(fd_sat) and abs(fd_liq - float(K.d[0, 0, 1])) <= 1e-8 * abs(fd_liq)


# ---- e_ref, the branch mask and the repair cases --------------------------------------------------------------------------------------------
def test_every_case_has_a_bound_and_keeps_its_columns():
    """e_ref of every case (printed) as |J_64 v - J_80 v| / sum |J_80| |v| over every product the GPU test asks for; the branch mask: at most
    2 columns in 13 lost, none of a one-column case -- with the state seeds of richards_cases.STATE_SEEDS, properties of the reference alone"""
    from test_gpu_tangent_richards_edges import BROKEN
    lost_total, largest = 0, (0.0, None)
    for case in RC.CASES:
        ref = RC.reference(case)
        lost = int((~ref.keep).sum())
        lost_total += lost
        worst = max(ref.parts, key=ref.parts.get)
        print(f"{case_id(case)}: e_ref = {ref.e_ref:.3e} ({worst}), bound = {ref.bound(BROKEN):.3e}, lost {lost} of {case[1]} columns")
        assert lost <= (2 if case[1] == RC.NH else 0), case_id(case)
        largest = max(largest, (ref.e_ref, case_id(case)))
        for label, (_, Ssum) in ref.expected.items():
            assert np.any(Ssum > 0), (case_id(case), label)
    print(f"columns lost over all cases: {lost_total}; largest e_ref = {largest[0]:.3e} ({largest[1]})")
    assert largest[0] <= 1.5 * MEASURED_LARGEST_E_REF and BROKEN == RC.FACTOR * 4.0 * MEASURED_LARGEST_E_REF


def test_the_repair_cases_run_what_they_are_for():
    """in the kept columns the upward pass, the downward pass, the top overflow and the bottom clamp each occur at least once"""
    for case in RC.CASES:
        if case[3] != "repair":
            continue
        ref = RC.reference(case)
        for name in ("upward pass", "downward pass", "top overflow", "bottom clamp"):
            assert LR.occurred(ref.wide, name, ref.keep), (case_id(case), name)
