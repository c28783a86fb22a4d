"""The reference of test_gpu_derivative_edges.py, pinned on the CPU: tests/linearised_heat.py against the wide oracle (its primal, at
every step of every case), against the central differences the derivative tests already trust (its Jacobian), its own fp64 rounding
e_ref per case (what the GPU test takes its bound from), and the regime mask of every case."""
import numpy as np
import pytest

import boundary_derivatives as B
import linearised_heat as LH
import series_derivatives as S
import test_gpu_derivative_edges as E
from boundary_derivatives import LD
from test_gpu_tangent import DT, TANGENTS, assert_close_by_column

# The largest difference between the restatement and oracle.Oracle(dtype = np.longdouble), both in np.longdouble, per field and relative
# to the field's largest value, over every case of test_gpu_derivative_edges.py and every step -- measured with this test (pytest -s
# prints the figures).  The two evaluate the same expressions; only the association of the mineral and organic terms of the
# conductivity and heat-capacity sums differs, so the cases without organic matter (rho_soc = 0) agree bit for bit and the figures are
# those of rho_soc = 26.  The bound is 16 x the measurement.
MEASURED_PRIMAL_DIFFERENCE = {"internal_energy": 7.48e-20, "temperature": 1.78e-18, "liquid_water_fraction": 1.09e-19}


def wide_oracle(case):
    import oracle
    Nz, Nh = case[0], case[1]
    p, U0, sat, bcs, series, _ = E.inputs(case)
    over = {name: getattr(p, name) for name in LH.PARAMS}
    o = oracle.Oracle(Nh, np.full(Nz, E.DZ), oracle.default_params(halo_policy=p.halo_policy, rho_soc=p.rho_soc, **over), dtype=np.longdouble)
    o.set("saturation_water_ice", sat)
    o.set("internal_energy", U0)
    for (var, side), (kind, value) in bcs.items():
        o.set_bc(var, side, kind, value)
    S.attach(o, series)
    o.closure()
    return o


def test_primal_is_the_wide_oracles():
    import oracle
    if not oracle.wide_available():
        pytest.skip("np.longdouble is not wider than float64 here")
    worst = dict.fromkeys(TANGENTS, 0.0)
    for case in E.CASES:
        p, U0, sat, bcs, series, _ = E.inputs(case)
        mine = LH.run([E.DZ] * case[0], U0, sat, bcs, p, DT, E.STEPS, dtype=LD, mirror=case[3] == "mirror", series=series, seed=())
        o = wide_oracle(case)
        for step in range(E.STEPS + 1):
            for x in TANGENTS:
                a, b = o.get(x), mine.trajectory[step][x]
                worst[x] = max(worst[x], float(np.max(np.abs(a - b)) / np.max(np.abs(a))))
            if step < E.STEPS:
                o.timestep(DT)
    for x in TANGENTS:
        print(f"restatement against the wide oracle, {x}: largest difference / field maximum = {worst[x]:.3e} "
              f"(bound {16.0 * MEASURED_PRIMAL_DIFFERENCE[x]:.3e})")
    for x in TANGENTS:
        assert worst[x] <= 16.0 * MEASURED_PRIMAL_DIFFERENCE[x], x


def test_closure_without_latent_heat():
    """L_theta = 0 (a dry cell): no phase change regime, liq is 1 at U >= 0 and 0 below, T = U / C on both sides"""
    p = E.thermal_params()
    U0 = np.array([[1e6, -1e6, 0.0]])
    sat = np.zeros((1, 3))
    r = LH.run([E.DZ], U0, sat, {}, p, DT, 0, dtype=LD, seed=("state",))
    assert np.array_equal(r.value("liquid_water_fraction"), [[1.0, 0.0, 1.0]])
    assert np.array_equal(r.regimes[0], [[LH.THAWED, LH.FROZEN, LH.THAWED]])
    J = r.block("state")
    assert np.all(J["liquid_water_fraction"] == 0.0)
    slope = J["temperature"][0, 0]
    assert np.all(slope > 0) and np.allclose((r.value("temperature")[0] / slope)[:2], U0[0, :2], rtol=1e-15)


def loss_gradient(J, w):
    """sum_X sum_i w_X[i] dX_n[i] / d(input), per column"""
    return sum(np.sum(w[x].astype(LD) * J[x], axis=0) for x in TANGENTS)


@pytest.mark.parametrize("halo", B.HALOS)
@pytest.mark.parametrize("bcset", B.FD_SETS)
def test_boundary_blocks_match_central_differences_of_the_oracle(bcset, halo):
    p, U0, sat, bcs, w = B.fd_inputs(bcset, halo)
    keep = B.fd_kept_columns(p, U0, sat, bcs)
    r = LH.run(B.FD_DZ, U0, sat, bcs, p, DT, B.FD_STEPS, dtype=LD, mirror=halo == "mirror", seed=("boundary",))
    for pair in B.active_pairs(bcs):
        h = B.FD_H[bcs[pair][0]]
        plus, minus, fd, Ssum = B.fd_central(p, U0, sat, bcs, pair, w, h)
        J = r.block(("boundary", pair))
        err = np.abs(fd - loss_gradient(J, w))[keep]
        print(f"{bcset} {halo} {pair}: max err / S = {float(np.max(err / Ssum[keep])):.3e}")
        assert np.all(err <= 1e-6 * Ssum[keep] + 1e-9 * np.max(Ssum[keep])), pair
        for x in TANGENTS:
            assert_close_by_column(plus[x], minus[x], h, J[x].astype(np.float64), keep, 1e-6, (x, pair))


@pytest.mark.parametrize("bcset,pair,indexing,halo", S.fd_cases())
def test_series_blocks_match_central_differences_of_the_oracle(bcset, pair, indexing, halo):
    p, U0, sat, bcs, w = S.fd_inputs(bcset, halo)
    series = S.series_on(bcs, [pair], indexing, B.FD_NH)
    keep = S.fd_kept_columns(p, U0, sat, bcs, series)
    r = LH.run(B.FD_DZ, U0, sat, bcs, p, DT, S.STEPS, dtype=LD, mirror=halo == "mirror", series=series, seed=("series",))
    J = r.block(("series", pair))
    h = B.FD_H[bcs[pair][0]]
    for node in range(S.NT):
        plus, minus, fd, Ssum = S.fd_central(p, U0, sat, bcs, series, pair, node, w, h)
        Jn = {x: J[x][:, node, :] for x in TANGENTS}
        err = np.abs(fd - loss_gradient(Jn, w))[keep]
        print(f"{bcset} {pair} {indexing} {halo} node {node}: max err / S = {float(np.max(err / Ssum[keep])):.3e}")
        assert np.all(err <= 1e-6 * Ssum[keep] + 1e-9 * np.max(Ssum[keep])), node
        for x in TANGENTS:
            assert_close_by_column(plus[x], minus[x], h, Jn[x].astype(np.float64), keep, 1e-6, (x, pair, node))


def test_every_case_has_a_bound_and_keeps_its_columns():
    """e_ref of every case (printed), the bound the GPU test derives from it, and the regime mask: at most 1 column in 13 lost, none of
    a one-column case, and all three regimes among the kept columns (both of the two a column of two cells starts in)"""
    lost_total = 0
    for case in E.CASES:
        ref = E.reference(case)
        lost = int((~ref.keep).sum())
        lost_total += lost
        worst = max(ref.parts, key=ref.parts.get)
        print(f"{E.case_id(case)}: e_ref = {ref.e_ref:.3e} ({worst}), bound = {ref.bound():.3e}, lost {lost} of {case[1]} columns")
        assert lost <= (1 if case[1] == E.NH else 0), E.case_id(case)
        kept = ref.regimes[:, :, ref.keep]
        present = sum(bool((kept == regime).any()) for regime in (LH.THAWED, LH.PHASE_CHANGE, LH.FROZEN))
        assert present == min(3, case[0] * case[1]), E.case_id(case)          # (two cells cannot hold more than two at a time)
        for label, (_, Ssum) in ref.expected.items():
            assert np.any(Ssum > 0), (E.case_id(case), label)
    print(f"columns lost over all cases: {lost_total}")
