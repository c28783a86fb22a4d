"""The reference of the heat + Richards adjoint tests, shared by test_richards_adjoint_host.py (which pins it on the CPU) and the two GPU
tests: the cases of tests/richards_cases.py, pulled back instead of pushed forward.  Everything here is computed on the CPU from
tests/linearised_richards.py; no figure of the device enters.

The expected gradient of a cotangent w [5][Nz][Nh] (the fields in the order of linearised_richards.FIELDS) is
g_ref[j, c] = sum_{x, i} J[x, i, j, c] w[x, i, c], J the extended-precision Jacobian of the restatement and j running over the Nz
internal-energy seeds, then the Nz saturation seeds; S = sum |J| |w| normalises a difference cell by cell, and e_ref of a contraction is the
same normalised difference between the float64 and the extended-precision restatement.  Contractions: one dense cotangent and one-hot
cotangents on each of the five fields at one_hot_levels(Nz)."""
import functools

import numpy as np

import linearised_heat as LH
import linearised_richards as LR
import richards_cases as RC
from richards_cases import CASES, DT, DZ, FACTOR, SPL, STEPS, case_id, one_hot_levels     # noqa: F401  (re-exported to the tests)

LD = np.longdouble
AXES = "xijc,xic->jc"
# the dense cotangent: standard normal numbers scaled per field to the size of a unit change of it (J/m3, saturation, K, fraction, m)
SCALES = (1e-6, 1.0, 1e-1, 1.0, 1e-2)
# The seed of the dense cotangent per shape, should one put e_ref of a case above the ceiling (as richards_cases.STATE_SEEDS does for the
# state): none has needed another so far
COTANGENT_SEED = 41
COTANGENT_SEEDS = {}
# The ceiling on a case's bound 8 x e_ref: BROKEN of test_gpu_tangent_richards_edges.py
BROKEN = FACTOR * 4.0 * 3.9e-12


def cotangents(case):
    """{label: w [5][Nz][Nh]}: every product J^T w the device is asked for"""
    Nz, Nh = case[0], case[1]
    rng = np.random.default_rng(COTANGENT_SEEDS.get((Nz, Nh), COTANGENT_SEED))
    out = {"dense": rng.normal(size=(len(LR.FIELDS), Nz, Nh)) * np.asarray(SCALES)[:, None, None]}
    for x, name in enumerate(LR.FIELDS):
        for j in one_hot_levels(Nz):
            w = np.zeros((len(LR.FIELDS), Nz, Nh))
            w[x, j] = 1.0
            out[f"one-hot {name} {j}"] = w
    return out


def run_schedule(dz, U0, sat0, bcs, p, schedule, dtype=LD):
    """linearised_richards.run under a schedule [(dt, steps), ...]: the same loop over the same functions, the dt changing between the
    stretches (the two-dt reference of the split tests)"""
    dtype = np.dtype(dtype).type
    U0 = np.asarray(U0, dtype=np.float64)
    Nz, Nh = U0.shape

    def seed(x, first):
        x = np.asarray(x, dtype=np.float64).astype(dtype)
        d = np.zeros(x.shape + (2 * Nz,), dtype=dtype)
        for r in range(Nz):
            d[r, :, first + r] = 1
        return LR.Dual(x, d)

    g = LR.grid(dz, Nh, dtype)
    c = LH.derived(p, dtype, LH.Seeds())
    h = LR.hydraulics(p, dtype)
    bcs = {pair: (kind, np.broadcast_to(np.asarray(value, dtype=np.float64), (Nh,))) for pair, (kind, value) in bcs.items()}
    U, sat = seed(U0, 0), seed(sat0, Nz)
    rec = LR.Branches()
    T, liq, Ltheta = LR.closure(c, U, sat)
    near = lambda: LR._near(U.x, 0.0, np.maximum(1.0, Ltheta)) | LR._near(U.x + Ltheta, 0.0, np.maximum(1.0, Ltheta))
    rec.add("regime", LH.regime_of(U.x, Ltheta), near())
    psi, z0 = LR.pressure_head(c, h, g, sat, rec)
    branches = [rec]
    for dt, steps in schedule:
        for _ in range(steps):
            rec = LR.Branches()
            GU, GS = LR.tendencies(c, h, g, U, sat, T, liq, psi, bcs, rec)
            U = U + GU * dtype(dt)
            sat, _ = LR.repair(g, sat + GS * dtype(dt), rec)
            psi, z0 = LR.pressure_head(c, h, g, sat, rec)
            T, liq, Ltheta = LR.closure(c, U, sat)
            rec.add("regime", LH.regime_of(U.x, Ltheta), near())
            branches.append(rec)
    return LR.Result(dict(zip(LR.FIELDS, (U, sat, T, liq, psi))), None, branches, Nz, Nh)


class Reference:
    """The reference of a case, computed once on the CPU: the kept columns, per contraction (J_80^T w, S) on them and its e_ref, and
    e_ref of the case (the largest).  `schedule`: [(dt, steps), ...] instead of the case's six steps of DT.  `jacobian`: keep J_80 on the
    kept columns (the host test's consistency checks)."""

    def __init__(self, case, schedule=None, jacobian=False):
        self.case = case
        if schedule is None:
            wide, narrow = RC.restatement(case, LD), RC.restatement(case, np.float64)
        else:
            p, U0, sat, bcs, _ = RC.inputs(case)
            wide, narrow = (run_schedule([DZ] * case[0], U0, sat, bcs, p, schedule, dtype) for dtype in (LD, np.float64))
        self.keep = LR.kept_columns(wide, narrow)
        J_wide, J_narrow = wide.jacobian()[..., self.keep], narrow.jacobian()[..., self.keep]
        self.J = J_wide if jacobian else None
        self.expected, self.parts = {}, {}
        if self.keep.any():
            for label, w in cotangents(case).items():
                with np.errstate(invalid="ignore"):
                    err, ref, Ssum = LH.contraction_error(J_narrow, J_wide, w[..., self.keep], AXES)
                self.expected[label], self.parts[label] = (ref, Ssum), err
        self.e_ref = max(self.parts.values(), default=0.0)

    def bound(self, ceiling=BROKEN):
        b = FACTOR * self.e_ref
        assert 0.0 < b <= ceiling, (case_id(self.case), "e_ref is no measurement of fp64 rounding", self.e_ref)
        return b

    def error(self, label, gU, gsat):
        """|dev - ref| / S of the device's (gU, gsat), [Nz][Nh] each, on the kept columns; exact zeros where S is zero"""
        ref, Ssum = self.expected[label]
        dev = np.concatenate([np.asarray(gU), np.asarray(gsat)])[..., self.keep]
        zero = Ssum == 0
        assert np.all(dev[zero] == 0.0), (case_id(self.case), label, "non-zero where the reference is exactly zero")
        return 0.0 if zero.all() else float(np.max(np.abs(dev.astype(LD) - ref)[~zero] / Ssum[~zero]))


@functools.lru_cache(maxsize=None)
def reference(case):
    """shared by the tests of a case; nothing in it is modified later"""
    return Reference(case)
