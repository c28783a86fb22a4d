"""The cases of the heat + Richards tangent tests and their reference, shared by test_linearised_richards_host.py (which pins the
reference on the CPU) and the two GPU tests: shapes at the edges of the lane layouts, the three hydraulics instances, two boundary sets,
and the repair cases.  Everything here is computed on the CPU from tests/linearised_richards.py; no figure of the device enters.

Shapes: Nz in {2, 3, 31, 32, 33, 63, 64} x 13 columns and one column at Nz = 2 and 64 -- the lane positions of the neighbour shifts, of
the two-level reach of the upwinded face and of the top and bottom selects.  Uniform 0.1 m grid, six steps of 60 s in launches of 4 and 2.
The saturation of a state lies in (0.6, 0.95): there six explicit steps of 60 s are stable for all three hydraulics (the Brooks-Corey
head -psi_s r^-5 makes drier columns stiff), and no cell sits on the theta < por threshold."""
import functools

import numpy as np

import linearised_heat as LH
import linearised_richards as LR
import terrarium_jl_amd as trm

CAPI = trm._capi
LD = np.longdouble
EDGE_SIZES = (2, 3, 31, 32, 33, 63, 64)
NH = 13
SHAPES = [(Nz, NH) for Nz in EDGE_SIZES] + [(2, 1), (64, 1)]
DZ, DT, STEPS, SPL = 0.1, 60.0, 6, 4
HYDRAULICS = ("default", "vg_n2", "generic")
SETS = ("T_top+flux_bottom", "infiltration_top")
REPAIR_SIZES = (3, 33)
FACTOR = 8.0
# (Nz, Nh, hydraulics, boundary set); the repair cases carry the set "repair"
CASES = [(Nz, Nh, hyd, bcset) for Nz, Nh in SHAPES for hyd in HYDRAULICS for bcset in SETS] + [(Nz, NH, "default", "repair") for Nz in REPAIR_SIZES]
# K_sat of the repair cases: a cell drained towards zero saturation is stiff under -psi_s r^-5 (its head at r = 0.1 is -1000 m) and its
# neighbours would refill it faster than any flux drains it; with this K_sat the fluxes decide, and the six steps stay finite
REPAIR_K_SAT = 1.0e-9


def case_id(case):
    return "Nz{}-Nh{}-{}-{}".format(*case)


def params(hyd, K_sat=None):
    p = CAPI.default_params()
    p.flow = CAPI.FLOW["richards"]
    if hyd != "default":
        p.swrc = CAPI.SWRC["van_genuchten"]
        p.unsat_k = CAPI.UNSATK["van_genuchten"]
        p.vg_n = 2.0 if hyd == "vg_n2" else 1.7
    if K_sat is not None:
        p.K_sat = K_sat
    return p


def porosity(p):
    org = p.rho_soc / ((1.0 - p.por_organic) * p.rho_org)
    return (1.0 - org) * p.por_mineral + org * p.por_organic


def mixed_state(Nz, Nh, p, seed):
    """(U, sat): saturation in (0.6, 0.95), every cell drawn thawed, in phase change or frozen, 0.2 MJ/m3 or more from the regime boundaries"""
    rng = np.random.default_rng(seed)
    sat = rng.uniform(0.6, 0.95, (Nz, Nh))
    L = p.rho_w * p.Lsl * sat * porosity(p)
    regime = rng.integers(0, 3, (Nz, Nh))
    far = rng.uniform(2e5, 8e6, (Nz, Nh))
    U = np.where(regime == 0, far, np.where(regime == 1, -rng.uniform(0.1, 0.9, (Nz, Nh)) * L, -L - far))
    return U, sat


def boundary_sets(Nh):
    T_top = np.linspace(-4.0, 4.0, Nh)
    return {
        # a temperature Value on top with fluxes at the bottom (energy and water, the water flowing in)
        "T_top+flux_bottom": {("temperature", "top"): ("value", T_top), ("internal_energy", "bottom"): ("flux", 0.05),
                              ("saturation_water_ice", "bottom"): ("flux", 2.0e-5)},
        # an infiltration flux on the top saturation (a top flux enters with a minus sign: negative flows in)
        "infiltration_top": {("saturation_water_ice", "top"): ("flux", np.linspace(-6.0e-5, -1.0e-5, Nh))},
    }


def analytic_slope(p, sat):
    """por / swrc'(psi_m) at theta = sat por, swrc' = d theta / d psi of the retention curve, in extended precision"""
    por, res, theta = LD(porosity(p)), LD(p.theta_res), LD(sat) * LD(porosity(p))
    r = (theta - res) / (por - res)
    if p.swrc == CAPI.SWRC["van_genuchten"]:
        n, alpha = LD(p.vg_n), LD(p.vg_alpha)
        m = 1 - 1 / n
        psi = -1 / alpha * (r ** (-1 / m) - 1) ** (1 / n)
        dtheta = (por - res) * (-m) * (1 + (-alpha * psi) ** n) ** (-m - 1) * n * (-alpha * psi) ** (n - 1) * (-alpha)
    else:
        lam, psi_s = LD(p.bc_lambda), LD(p.bc_psi_s)
        psi = -psi_s * r ** (-1 / lam)
        dtheta = (por - res) * lam * (-psi_s / psi) ** lam * (-1 / psi)
    return por / dtheta


# The repair cases: thawed columns (U > 0) whose fluxes drive the four parts of adjust_saturation_profile!, by column group --
#   0 .. 3    the bottom cell starts at 0.93 and takes +0.05 of saturation a step: oversaturated from the second step on, the upward pass
#             carries the excess into the cell above, which stays below 1 (two saturated cells in a row are in hydrostatic balance: a head
#             gradient of exactly zero, where the upwinding has no derivative)
#   4 .. 6    the top cell starts at 0.9 and takes +0.05 a step: the top overflow into surface_excess_water
#   7 .. 9    the top cell loses 0.17 a step (REPAIR_DRAIN) and falls below zero in the last step alone: the downward pass
#   10 .. 12  the bottom cell does, in the last step alone: the bottom clamp
# (a cell the downward pass or the clamp leaves at zero saturation has an infinite head: a further step would be NaN, so both happen in
# the last step).  The rest of every column sits at REPAIR_REST.
REPAIR_REST, REPAIR_FILL, REPAIR_DRAIN = 0.7, 8.5e-5, 2.83e-4


def repair_state(Nz, Nh, p):
    rng = np.random.default_rng(77)
    sat = np.full((Nz, Nh), REPAIR_REST) + rng.uniform(-0.02, 0.02, (Nz, Nh))
    sat[0, 0:4] = 0.93
    sat[Nz - 1, 4:7] = 0.9
    sat[Nz - 1, 7:10] = 0.95
    sat[0, 10:13] = 0.95
    U = rng.uniform(2e6, 8e6, (Nz, Nh))
    bottom, top = np.zeros(Nh), np.zeros(Nh)
    bottom[0:4] = REPAIR_FILL
    top[4:7] = -REPAIR_FILL
    top[7:10] = REPAIR_DRAIN
    bottom[10:13] = -REPAIR_DRAIN
    bcs = {("saturation_water_ice", "bottom"): ("flux", bottom), ("saturation_water_ice", "top"): ("flux", top)}
    return U, sat, bcs


# The seed of mixed_state per shape: the first from 1 up with which, in every case of the shape, the branch mask keeps all but two of
# the 13 columns (the column of a one-column shape) and no entry of the Jacobian is a cancellation's zero (seed 1 at Nz = 2 has one: the
# upward pass of the last step moves the bottom cell's tangent into the top cell, where mass conservation makes the sum exactly 0 in
# extended precision and a rounding residue in float64).  Properties of the reference alone, asserted in test_linearised_richards_host.py.
STATE_SEEDS = {(2, 13): 2, (32, 13): 2}


def state_seed(case):
    return STATE_SEEDS.get((case[0], case[1]), 1)


def one_hot_levels(Nz):
    return sorted({0, Nz - 1} | ({31, 32} if Nz >= 33 else set()))


def inputs(case):
    """(p, U0, sat, bcs, dense seed [2 Nz][Nh])"""
    Nz, Nh, hyd, bcset = case
    if bcset == "repair":
        p = params(hyd, REPAIR_K_SAT)
        U0, sat, bcs = repair_state(Nz, Nh, p)
    else:
        p = params(hyd)
        U0, sat = mixed_state(Nz, Nh, p, state_seed(case))
        bcs = boundary_sets(Nh)[bcset]
    bcs = {pair: (kind, np.broadcast_to(np.asarray(value, dtype=np.float64), (Nh,)).copy()) for pair, (kind, value) in bcs.items()}
    rng = np.random.default_rng(1000 + state_seed(case))
    dense = np.concatenate([rng.normal(0.0, 1e3, (Nz, Nh)), rng.normal(0.0, 1e-3, (Nz, Nh))])       # J/m3, saturation
    return p, U0, sat, bcs, dense


def restatement(case, dtype, seeded=True):
    p, U0, sat, bcs, _ = inputs(case)
    return LR.run([DZ] * case[0], U0, sat, bcs, p, DT, STEPS, dtype=dtype, seeded=seeded)


def contractions(case):
    """{label: seed [2 Nz][Nh]}: every product J v the device is asked for -- the dense seed, one-hot seeds in U and in sat"""
    Nz, Nh = case[0], case[1]
    out = {"dense": inputs(case)[4]}
    for j in one_hot_levels(Nz):
        for name, first in (("U", 0), ("sat", Nz)):
            e = np.zeros((2 * Nz, Nh))
            e[first + j] = 1.0
            out[f"one-hot {name} {j}"] = e
    return out


AXES = "xijc,jc->xic"


class Reference:
    """The reference of a case, computed once on the CPU: the kept columns, per contraction (J_80 v, S) on them and its e_ref, the
    branches of the wide run, and e_ref of the case (the largest).  The Jacobians are not kept."""

    def __init__(self, case):
        self.case = case
        wide, narrow = restatement(case, LD), restatement(case, np.float64)
        self.keep = LR.kept_columns(wide, narrow)
        self.wide = wide
        J_wide, J_narrow = wide.jacobian()[..., self.keep], narrow.jacobian()[..., self.keep]
        wide.final = narrow.final = None
        self.expected, self.parts = {}, {}
        if self.keep.any():
            for label, v in contractions(case).items():
                with np.errstate(invalid="ignore"):
                    err, ref, Ssum = LH.contraction_error(J_narrow, J_wide, v[:, self.keep], AXES)
                self.expected[label], self.parts[label] = (ref, Ssum), err
        self.e_ref = max(self.parts.values(), default=0.0)

    def bound(self, ceiling):
        b = FACTOR * self.e_ref
        assert 0.0 < b <= ceiling, (case_id(self.case), "e_ref is no measurement of fp64 rounding", self.e_ref)
        return b

    def error(self, label, dev):
        """|dev - ref| / S of the five device tangents [5][Nz][Nh] on the kept columns; exact zeros where S is zero"""
        ref, Ssum = self.expected[label]
        dev = np.asarray(dev)[..., self.keep]
        zero = Ssum == 0
        assert np.all(dev[zero] == 0.0), (case_id(self.case), label, "non-zero where the reference is exactly zero")
        return 0.0 if zero.all() else float(np.max(np.abs(dev.astype(LD) - ref)[~zero] / Ssum[~zero]))


@functools.lru_cache(maxsize=None)
def reference(case):
    """shared by the tests of a case; nothing in it is modified later"""
    return Reference(case)
