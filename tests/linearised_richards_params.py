"""The reference of the hydraulic-parameter gradients of the heat + Richards adjoint, shared by test_richards_params_host.py (which pins
it on the CPU) and the two GPU tests: tests/linearised_richards.py, imported unchanged, driven with the hydraulics dict `h` holding duals
seeded on the seven parameters of trm_params' hydraulics line -- K_sat, theta_res, bc_psi_s, bc_lambda, vg_alpha, vg_n, impedance.  The
same functions run (closure, pressure_head, tendencies, repair); the seed axis is the 2 Nz state seeds of linearised_richards.run, then 7
more.  Everything here is computed on the CPU; no figure of the device enters.

linearised_richards.power takes a constant exponent; with vg_n and bc_lambda seeded the exponents are duals, so `power` below is installed
in its place for the duration of a run: d(x^y)/dy = x^y ln x, and 0 where x^y is 0 (a frozen cell's x = 0 under x^(n/(n+1)); the Mualem
term at x = 1); a zero seed gives 0 whatever the factor.  The base's share is linearised_richards' own.

g_ref[p, c] = sum_{x, i} J_p[x, i, p, c] w[x, i, c] for a cotangent w [5][Nz][Nh] of richards_adjoint_cases.cotangents, J_p the
extended-precision Jacobian's parameter columns; S = sum |J_p| |w|; e_ref of a contraction is the same normalised difference between the
float64 and the extended-precision run (linearised_heat.contraction_error).

The bound of a case is FACTOR (8) times the largest e_ref over the non-repair cases of the same Nz and hydraulics -- both boundary sets,
Nh = 13 and 1: a parameter gradient is one number per column, so a one-column case samples e_ref once (down to 5e-16 there, while every
pooled value is >= 2e-14).  The two repair cases are the only ones of their boundary set and keep their own e_ref.  In a repair case the
final state of the downward-pass and bottom-clamp columns (7 .. 12) holds a cell at zero saturation: its head is infinite and so is its
parameter slope.  There the pressure-head cotangent is zero (`cotangents`), and the non-finite pressure-head rows stay out of the
contraction.

CEILING: FACTOR x 4 x the largest e_ref measured on the CPU with this module, rounded up to two digits -- see LARGEST_E_REF."""
import functools
import types

import numpy as np

import linearised_heat as LH
import linearised_richards as LR
import richards_adjoint_cases as RA
import richards_cases as RC
from linearised_heat import Dual
from richards_cases import CASES, DT, DZ, FACTOR, SPL, STEPS, case_id     # noqa: F401  (re-exported to the tests)

LD = np.longdouble
# the seven names in the order of TRM_HYDRAULIC_PARAM_* (the fields of trm_params), and the key of `h` each is read through
PARAMS = ("K_sat", "theta_res", "bc_psi_s", "bc_lambda", "vg_alpha", "vg_n", "impedance")
H_KEY = dict(K_sat="K_sat", theta_res="theta_res", bc_psi_s="psi_s", bc_lambda="lam", vg_alpha="alpha", vg_n="n", impedance="impedance")
AXES = "xipc,xic->pc"
# the largest parameter e_ref this module gives over the 56 cases, and its case (test_richards_params_host.py prints every one)
LARGEST_E_REF = (3.5e-11, "Nz33-Nh13-default-repair")
CEILING = FACTOR * 4.0 * LARGEST_E_REF[0]
# columns of a repair case whose final state holds a cell at zero saturation (richards_cases.repair_state: the downward pass, the clamp)
DRY_COLUMNS = slice(7, 13)


def unread(hyd):
    """the parameters the hydraulics of a case never read: exact zeros"""
    return ("vg_alpha", "vg_n", "impedance") if hyd == "default" else ("bc_psi_s", "bc_lambda")


def power(a, y):
    """a ^ y for an exponent that may be a dual"""
    if not isinstance(y, Dual) or y.d is None:
        return _constant_power(a, y.x if isinstance(y, Dual) else y)
    with np.errstate(all="ignore"):
        v = np.power(a.x, y.x)
        base = LR._scaled_or_zero(a, y.x * v / a.x)
        slope = np.where(v == 0, np.zeros((), dtype=v.dtype), v * np.log(a.x))
        d = slope[..., None] * y.d
        d = np.where(np.broadcast_to(y.d, d.shape) == 0, np.zeros((), dtype=d.dtype), d)
    return Dual(v, d if base is None else base + d)


_constant_power = LR.power


class _installed:
    """`power` in linearised_richards' namespace for the duration of a run"""

    def __enter__(self):
        LR.power = power

    def __exit__(self, *exc):
        LR.power = _constant_power
        return False


def seeded_hydraulics(p, dtype, ns, first):
    """linearised_richards.hydraulics with the seven parameters as duals: seed first + q on parameter q"""
    h = LR.hydraulics(p, dtype)
    for q, name in enumerate(PARAMS):
        d = np.zeros(ns, dtype=dtype)
        d[first + q] = 1
        h[H_KEY[name]] = Dual(dtype(getattr(p, name)), d)
    h["m"] = dtype(1) - dtype(1) / h["n"]
    return h


def carried(p, name, value):
    """p with the parameter `name` held as `value` (an np.longdouble travels into the restatement unrounded)"""
    q = types.SimpleNamespace(**{field: getattr(p, field) for field, *_ in p._fields_})
    setattr(q, name, value)
    return q


def run(dz, U0, sat0, bcs, p, dt, nsteps, dtype=LD):
    """linearised_richards.run with the parameter seeds behind the state seeds: the same loop over the same functions"""
    dtype = np.dtype(dtype).type
    U0 = np.asarray(U0, dtype=np.float64)
    Nz, Nh = U0.shape
    ns = 2 * Nz + len(PARAMS)

    def seed(x, first):
        x = np.asarray(x, dtype=np.float64).astype(dtype)
        d = np.zeros(x.shape + (ns,), dtype=dtype)
        for r in range(Nz):
            d[r, :, first + r] = 1
        return Dual(x, d)

    g = LR.grid(dz, Nh, dtype)
    c = LH.derived(p, dtype, LH.Seeds())
    h = seeded_hydraulics(p, dtype, ns, 2 * Nz)
    bcs = {pair: (kind, np.broadcast_to(np.asarray(value, dtype=np.float64), (Nh,))) for pair, (kind, value) in bcs.items()}
    U, sat = seed(U0, 0), seed(sat0, Nz)
    near = lambda: LR._near(U.x, 0.0, np.maximum(1.0, Ltheta)) | LR._near(U.x + Ltheta, 0.0, np.maximum(1.0, Ltheta))
    with _installed():
        rec = LR.Branches()
        T, liq, Ltheta = LR.closure(c, U, sat)
        rec.add("regime", LH.regime_of(U.x, Ltheta), near())
        psi, z0 = LR.pressure_head(c, h, g, sat, rec)
        branches = [rec]
        for _ in range(nsteps):
            rec = LR.Branches()
            GU, GS = LR.tendencies(c, h, g, U, sat, T, liq, psi, bcs, rec)
            U = U + GU * dtype(dt)
            sat, _ = LR.repair(g, sat + GS * dtype(dt), rec)
            psi, z0 = LR.pressure_head(c, h, g, sat, rec)
            T, liq, Ltheta = LR.closure(c, U, sat)
            rec.add("regime", LH.regime_of(U.x, Ltheta), near())
            branches.append(rec)
    return LR.Result(dict(zip(LR.FIELDS, (U, sat, T, liq, psi))), None, branches, Nz, Nh)


def restatement(case, dtype, inputs=None):
    p, U0, sat, bcs = RC.inputs(case)[:4] if inputs is None else inputs
    return run([DZ] * case[0], U0, sat, bcs, p, DT, STEPS, dtype=dtype)


def split(J, Nz):
    """(state block [5][Nz][2 Nz][Nh], parameter block [5][Nz][7][Nh]) of a Jacobian over the whole seed axis"""
    return J[:, :, :2 * Nz], J[:, :, 2 * Nz:]


def cotangents(case):
    """richards_adjoint_cases.cotangents; in a repair case the pressure-head cotangent is zero in the columns whose final state holds a
    cell at zero saturation"""
    out = {label: w.copy() for label, w in RA.cotangents(case).items()}
    if case[3] == "repair":
        for w in out.values():
            w[LR.FIELDS.index("pressure_head"), :, DRY_COLUMNS] = 0.0
    return out


class Reference:
    """The reference of a case, computed once on the CPU: the kept columns, per contraction (g_ref [7][kept], S) and its e_ref, and e_ref of
    the case (the largest).  `jacobian`: keep the extended-precision Jacobian over the whole seed axis, all columns.  `inputs`:
    (p, U0, sat, bcs) in place of the case's own, on the case's shape and with its cotangents.  `mask` False: every column is kept
    (K_sat = 0, where every face minimum is a tie at zero in either precision and both sides take the tie's second operand)."""

    def __init__(self, case, jacobian=False, inputs=None, mask=True):
        self.case = case
        Nz = case[0]
        wide, narrow = restatement(case, LD, inputs), restatement(case, np.float64, inputs)
        self.keep = LR.kept_columns(wide, narrow) if mask else np.ones(case[1], dtype=bool)
        J_all = wide.jacobian()
        self.J = J_all if jacobian else None
        J_wide, J_narrow = split(J_all, Nz)[1][..., self.keep], split(narrow.jacobian(), Nz)[1][..., self.keep]
        # the rows no finite arithmetic reaches: a head at zero saturation (repair cases, the pressure-head rows of the dry columns alone)
        self.nonfinite = ~(np.isfinite(J_wide.astype(np.float64)) & np.isfinite(J_narrow))
        J_wide, J_narrow = np.where(self.nonfinite, LD(0), J_wide), np.where(self.nonfinite, 0.0, J_narrow)
        self.expected, self.parts = {}, {}
        if self.keep.any():
            for label, w in cotangents(case).items():
                w = w[..., self.keep]
                assert not np.any(self.nonfinite & (w != 0)[:, :, None, :]), (case_id(case), label, "a cotangent on a non-finite row")
                err, ref, Ssum = LH.contraction_error(J_narrow, J_wide, w, AXES)
                self.expected[label], self.parts[label] = (ref, Ssum), err
        self.e_ref = max(self.parts.values(), default=0.0)

    def error(self, label, grads):
        """|dev - ref| / S of the device's seven per-column gradients {name: [Nh]} on the kept columns; exact zeros where S is zero"""
        ref, Ssum = self.expected[label]
        dev = np.stack([np.asarray(grads[name]) for name in PARAMS])[:, self.keep]
        zero = Ssum == 0
        assert np.all(dev[zero] == 0.0), (case_id(self.case), label, "non-zero where the reference is exactly zero")
        return 0.0 if zero.all() else float(np.max(np.abs(dev.astype(LD) - ref)[~zero] / Ssum[~zero]))


@functools.lru_cache(maxsize=None)
def reference(case):
    """shared by the tests of a case; nothing in it is modified later"""
    return Reference(case)


def pool(case):
    """the cases whose e_ref the bound of `case` is taken over"""
    if case[3] == "repair":
        return [case]
    return [q for q in CASES if q[0] == case[0] and q[2] == case[2] and q[3] != "repair"]


@functools.lru_cache(maxsize=None)
def bound(case):
    """FACTOR x the pooled e_ref, in (0, CEILING]"""
    b = FACTOR * max(reference(q).e_ref for q in pool(case))
    assert 0.0 < b <= CEILING, (case_id(case), "e_ref is no measurement of fp64 rounding", b)
    return b
