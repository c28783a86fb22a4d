"""An exact linearisation of the heat + Richards ForwardEuler step in numpy: the reference of test_linearised_richards_host.py,
test_gpu_tangent_richards.py and test_gpu_tangent_richards_edges.py.

The step is restated from oracle/terrarium_oracle.hpp (update_state, explicit_step, closure with RichardsEq) over the dual type of
linearised_heat.py, in the dtype the caller chooses (np.float64 or np.longdouble): the energy closure, the Brooks-Corey and van Genuchten
retention curves, the linear and the van Genuchten-Mualem conductivity, the face minimum and the upwinding, the Darcy fluxes, the
saturation repair with both passes, the top overflow and the bottom clamp, the water table and the flux boundary terms.  The seeds are the
state's: the initial internal energy (seed j: level j of every column) and the initial saturation (seed Nz + j).  Derivatives come from
operator overloading; `where` on the primal's condition keeps the derivative of the branch taken.  Nothing here is taken from csrc/.

Three conventions, stated because a derivative does not exist there and any choice is one:
  * max(x, 0) passes the derivative where x > 0 and gives 0 elsewhere (a tie: 0); min(x, y) takes y on a tie, as Base.min;
  * a power x^a has the derivative a x^a / x dx, and 0 where dx is 0 whatever the factor (x = 0: a frozen cell's water content under
    sqrt; 1 - x^e1 = 0: a saturated cell in the Mualem term);
  * the water table is piecewise constant in the saturation: no derivative.
Every branch a cell takes at every step is recorded (`Result.branches`), with the distance of the tested value from its threshold
(`Result.near`): kept_columns drops a column only where the two precisions disagree on a branch or a tested value lies within MARGIN
(relative) of its threshold.

Arrays are [Nz][Nh], row 0 the bottom layer."""
import numpy as np

import linearised_heat as LH
from linearised_heat import Dual, stack_levels, where

FIELDS = ("internal_energy", "saturation", "temperature", "liquid_water_fraction", "pressure_head")
MARGIN = 1e-9
LN10 = np.log(np.longdouble(10))


# ---- dual helpers the heat-only restatement does not need --------------------------------------------------------------------------
def _scaled_or_zero(a, factor):
    """a.d * factor, and 0 where a.d is 0 whatever the factor is"""
    if a.d is None:
        return None
    with np.errstate(all="ignore"):
        d = a.d * np.asarray(factor)[..., None]
    return np.where(a.d == 0, np.zeros((), dtype=d.dtype), d)


def power(a, y):
    """a ^ y for a constant exponent"""
    with np.errstate(all="ignore"):
        v = np.power(a.x, y)
        return Dual(v, _scaled_or_zero(a, y * v / a.x))


def exp10(a):
    with np.errstate(all="ignore"):
        v = np.power(a.x.dtype.type(10), a.x)
    return Dual(v, _scaled_or_zero(a, LN10.astype(a.x.dtype) * v))


def absolute(a):
    return Dual(np.abs(a.x), None if a.d is None else a.d * np.where(a.x < 0, -1, 1).astype(a.x.dtype)[..., None])


def rows_of(a):
    """the rows of a [n][Nh] dual as a list of [Nh] duals"""
    return [a[k] for k in range(a.x.shape[0])]


def from_rows(rows):
    x = np.stack([r.x for r in rows])
    if all(r.d is None for r in rows):
        return Dual(x)
    ns = next(r.d for r in rows if r.d is not None).shape[-1]
    return Dual(x, np.stack([np.zeros(r.x.shape + (ns,), dtype=x.dtype) if r.d is None else np.broadcast_to(r.d, r.x.shape + (ns,)) for r in rows]))


class Branches:
    """the branches of one step: name -> (taken [rows][Nh], near [rows][Nh])"""

    def __init__(self):
        self.taken, self.near = {}, {}

    def add(self, name, taken, near):
        self.taken[name] = np.asarray(taken).copy()
        self.near[name] = np.asarray(near).copy()


def _near(value, threshold=0.0, scale=None):
    value = np.abs(np.asarray(value, dtype=np.longdouble) - threshold)
    scale = np.maximum(np.abs(threshold), 0.0) if scale is None else np.asarray(scale, dtype=np.longdouble)
    return value <= MARGIN * np.maximum(scale, np.finfo(np.float64).tiny)


def minimum(x, y, rec, name):
    """Base.min(x, y): x where x < y, else y.  A tie of operands with the same derivatives is no branch."""
    take_x = x.x < y.x
    dx, dy = x.full(), y.full()
    same = (x.x == y.x) & (True if dx is None and dy is None else np.all((0 if dx is None else dx) == (0 if dy is None else dy), axis=-1))
    rec.add(name, np.where(same, False, take_x), _near(x.x - y.x, 0.0, np.maximum(np.abs(x.x), np.abs(y.x))) & ~same)
    return where(take_x, x, y)


def positive_part(x, rec, name, scale=1.0):
    """max(x, 0)"""
    took = x.x > 0
    rec.add(name, took, _near(x.x, 0.0, scale))
    return where(took, x, x.x.dtype.type(0))


# ---- the physics ---------------------------------------------------------------------------------------------------------------------
def hydraulics(p, dtype):
    n = dtype(p.vg_n)
    return dict(swrc=int(p.swrc), unsat_k=int(p.unsat_k), K_sat=dtype(p.K_sat), theta_res=dtype(p.theta_res), psi_s=dtype(p.bc_psi_s),
                lam=dtype(p.bc_lambda), alpha=dtype(p.vg_alpha), n=n, m=dtype(1) - dtype(1) / n, impedance=dtype(p.impedance),
                vwc_forcing=dtype(p.vwc_forcing))


def fractions(c, sat, liq):
    one = sat.x.dtype.type(1)
    water_ice = sat * c["por"]
    return water_ice * liq, water_ice * (one - liq), (one - sat) * c["por"]


def conductivity(c, sat, liq):
    water, ice, air = fractions(c, sat, liq)
    s = c["sk_water"] * water + c["sk_ice"] * ice + c["sk_air"] * air + c["s0"]
    return s * s


def closure(c, U, sat):
    """(T, liq, regime) of the FreeWater energy closure at (U, sat), both duals"""
    dtype = sat.x.dtype.type
    Ltheta = sat * c["L"] * c["por"]
    melting = dtype(1) - U / (-Ltheta + dtype(LH.EPS))
    liq = where(U.x >= 0, dtype(1), where(U.x >= -Ltheta.x, melting, dtype(0)))
    water, ice, air = fractions(c, sat, liq)
    C = c["c_water"] * water + c["c_ice"] * ice + c["c_air"] * air + c["C0"]
    T = where(U.x < -Ltheta.x, (U + Ltheta) / C, where(U.x >= 0, U / C, dtype(0)))
    return T, liq, Ltheta.x


def matric_head(c, h, sat, rec):
    """swrc_psi(theta = sat por, theta_sat = por)"""
    dtype = sat.x.dtype.type
    theta = sat * c["por"]
    unsat = theta.x < c["por"]
    rec.add("unsaturated", unsat, _near(theta.x, c["por"]) & (theta.x != c["por"]))
    r = (theta - h["theta_res"]) / (c["por"] - h["theta_res"])
    if h["swrc"] == 1:
        psi = power(power(r, dtype(-1) / h["m"]) - dtype(1), dtype(1) / h["n"]) * (dtype(-1) / h["alpha"])
        return where(unsat, psi, dtype(0))
    return where(unsat, power(r, dtype(-1) / h["lam"]) * (-h["psi_s"]), -h["psi_s"])


def water_table(g, sat, rec):
    """zF of the first cell from the bottom with sat < 1, the surface if there is none: [Nh], a constant"""
    Nz = g["Nz"]
    below_one = sat.x < 1
    rec.add("water table", below_one, _near(sat.x, 1.0) & (sat.x != 1))
    first = np.where(below_one.any(axis=0), np.argmax(below_one, axis=0), Nz)
    return g["zF"][1 + first]


def pressure_head(c, h, g, sat, rec):
    dtype = sat.x.dtype.type
    Nz = g["Nz"]
    z0 = water_table(g, sat, rec)
    z = g["zC"][1:Nz + 1, None]
    psih = np.maximum(dtype(0), z0[None, :] - z)
    psiz = z - g["zF"][Nz + 1]
    return (matric_head(c, h, sat, rec) + psih) + psiz, z0


def cell_conductivity(c, h, sat, liq):
    dtype = sat.x.dtype.type
    water, ice, air = fractions(c, sat, liq)
    if h["unsat_k"] == 0:
        return water * h["K_sat"] / (water + ice + air)
    n = h["n"]
    x = water / c["por"]
    I_ice = exp10((dtype(1) - liq) * (-h["impedance"]))
    inner = dtype(1) - power(x, n / (n + dtype(1)))
    t = dtype(1) - power(inner, (n - dtype(1)) / n)
    assert np.all((x.x >= 0) & (x.x <= 1)), "an illegal composition: not restated"
    return absolute(I_ice * h["K_sat"] * power(x, dtype(0.5)) * (t * t))


def tendencies(c, h, g, U, sat, T, liq, psi, bc, rec):
    """(dU/dt, dsat/dt) of compute_tendencies plus the Flux terms of explicit_step; bc = {(var, side): (kind, value [Nh])}"""
    Nz = g["Nz"]
    dtype = sat.x.dtype.type
    kind = lambda pair: bc[pair][0] if pair in bc else "noflux"
    value = lambda pair: Dual(np.asarray(bc[pair][1], dtype=np.float64).astype(dtype)) if pair in bc else None
    # ---- energy (the halo cells copy the edge cells: Richards fills the saturation halo)
    Tb = LH.halo_value(kind(("temperature", "bottom")), value(("temperature", "bottom")), T[0], g["dzf"][1], top=False)
    Tt = LH.halo_value(kind(("temperature", "top")), value(("temperature", "top")), T[Nz - 1], g["dzf"][Nz + 1], top=True)
    Th = stack_levels(Tb, T, Tt)
    kap = conductivity(c, stack_levels(sat[0], sat, sat[Nz - 1]), stack_levels(liq[0], liq, liq[Nz - 1]))
    rdzf = g["rdzf"][1:, None]
    q = -((kap[1:] + kap[:-1]) * dtype(0.5)) * ((Th[1:] - Th[:-1]) * rdzf)
    GU = -((q[1:] - q[:-1]) * g["rdzc"][1:Nz + 1, None])
    # ---- water: Kf on faces 0 .. Nz + 2 (0 and Nz + 2 are never written: 0), Darcy fluxes on faces 1 .. Nz + 1
    Kc = rows_of(cell_conductivity(c, h, sat, liq))
    zero = Dual(np.zeros_like(sat.x[0]))
    Kf = [zero, Kc[0]]
    step_rec = Branches()
    for k in range(2, Nz):                                           # (cells 2 .. Nz - 1, one-based)
        Kf.append(minimum(Kc[k - 1], Kc[k - 2], step_rec, f"face {k}"))
    Kf += [Kc[Nz - 1], Kc[Nz - 1], zero]
    rec.add("face minimum", np.stack([step_rec.taken.get(f"face {k}", np.zeros_like(sat.x[0], dtype=bool)) for k in range(2, max(Nz, 3))]),
            np.stack([step_rec.near.get(f"face {k}", np.zeros_like(sat.x[0], dtype=bool)) for k in range(2, max(Nz, 3))]))
    psi_h = stack_levels(psi[0], psi, psi[Nz - 1])
    grad = (psi_h[1:] - psi_h[:-1]) * rdzf                           # faces 1 .. Nz + 1
    down = grad.x < 0
    # (faces 1 and Nz + 1 see psi - psi of the edge cell: exactly 0 in any arithmetic, no branch)
    scale = np.maximum(np.abs(psi_h.x[1:]), np.abs(psi_h.x[:-1]))
    near_grad = _near(psi_h.x[1:] - psi_h.x[:-1], 0.0, scale)
    near_grad[0] = near_grad[Nz] = False
    rec.add("upwind direction", down, near_grad)
    taken, near, Kstar = [], [], []
    for f in range(1, Nz + 2):
        r = Branches()
        lo = minimum(Kf[f - 1], Kf[f], r, "lo")
        hi = minimum(Kf[f], Kf[f + 1], r, "hi")
        Kstar.append(where(down[f - 1], lo, hi))
        taken.append(np.where(down[f - 1], r.taken["lo"], r.taken["hi"]))
        near.append(np.where(down[f - 1], r.near["lo"], r.near["hi"]))
    rec.add("upwind minimum", np.stack(taken), np.stack(near))
    qW = -(from_rows(Kstar) * grad)
    div = (qW[1:] - qW[:-1]) * g["rdzc"][1:Nz + 1, None]
    GS = (-div + dtype(0) + h["vwc_forcing"]) / c["por"]
    # ---- compute_z_bcs!: Flux conditions
    Az = g["dx"]
    bottom = np.arange(Nz)[:, None] == 0
    top = np.arange(Nz)[:, None] == Nz - 1
    for var, G in (("internal_energy", "U"), ("saturation_water_ice", "S")):
        add = Dual(np.zeros_like(sat.x))
        if kind((var, "bottom")) == "flux":
            add = add + where(bottom, value((var, "bottom")) * Az / (Az * g["dzc"][1]), dtype(0))
        if kind((var, "top")) == "flux":
            add = add - where(top, value((var, "top")) * Az / (Az * g["dzc"][Nz]), dtype(0))
        if G == "U":
            GU = GU + add
        else:
            GS = GS + add
    return GU, GS


def repair(g, sat, rec):
    """adjust_saturation_profile!: (sat, overflow into surface_excess_water [Nh])"""
    Nz = g["Nz"]
    dtype = sat.x.dtype.type
    s = rows_of(sat)
    dzc = g["dzc"]                                                   # cell k (one-based) at dzc[k]
    up, down = Branches(), Branches()
    for k in range(0, Nz - 1):
        excess = positive_part(s[k] - dtype(1), up, k)
        s[k] = s[k] - excess
        s[k + 1] = s[k + 1] + excess * dzc[k + 1] / dzc[k + 2]
    for k in range(Nz - 1, 0, -1):
        deficit = positive_part(-s[k], down, k)
        s[k] = s[k] + deficit
        s[k - 1] = s[k - 1] - deficit * dzc[k + 1] / dzc[k]
    rec.add("upward pass", np.stack([up.taken[k] for k in range(Nz - 1)]), np.stack([up.near[k] for k in range(Nz - 1)]))
    rec.add("downward pass", np.stack([down.taken[k] for k in range(1, Nz)]), np.stack([down.near[k] for k in range(1, Nz)]))
    one = Branches()
    excess = positive_part(s[Nz - 1] - dtype(1), one, "top")
    s[Nz - 1] = s[Nz - 1] - excess
    rec.add("top overflow", one.taken["top"][None], one.near["top"][None])
    clamped = ~(s[0].x > 0)
    rec.add("bottom clamp", clamped[None], (_near(s[0].x, 0.0, 1.0) & (s[0].x != 0))[None])
    s[0] = where(clamped, dtype(0), s[0])
    return from_rows(s), excess.x * dzc[Nz]


def grid(dz, Nh, dtype):
    g = LH.grid(dz, Nh, dtype)
    # (faces and centres, which the heat-only restatement does not keep: Grid::build of the oracle)
    dzv = np.asarray(dz, dtype=np.float64)
    Nz = dzv.size
    cs = np.cumsum(dzv)          # (np.cumsum adds left to right, as the oracle's loop)
    zF = np.zeros(Nz + 3, dtype=dtype)
    for k in range(1, Nz + 1):
        zF[k] = dtype(-cs[Nz - k])
    zF[0] = zF[1] - (zF[2] - zF[1])
    zF[Nz + 2] = zF[Nz + 1] + (zF[Nz + 1] - zF[Nz])
    g["zF"] = zF
    g["zC"] = (zF[1:] + zF[:-1]) / dtype(2)
    return g


class Result:
    """final: {field: Dual [Nz][Nh]}; trajectory: per state 0 .. n the primal {field or water_table / surface_excess_water: array};
    branches: per state 0 .. n a Branches (state 0: of the initial closures alone)"""

    def __init__(self, final, trajectory, branches, Nz, Nh):
        self.final, self.trajectory, self.branches, self.Nz, self.Nh = final, trajectory, branches, Nz, Nh

    def jacobian(self):
        """[5][Nz out][2 Nz in][Nh]: d(field) / d(U_0, sat_0)"""
        out = []
        for name in FIELDS:
            q = self.final[name]
            d = q.full()
            out.append(np.zeros(q.x.shape[:1] + (2 * self.Nz,) + q.x.shape[1:], dtype=q.x.dtype) if d is None else np.ascontiguousarray(np.moveaxis(d, -1, 1)))
        return np.stack(out)


def run(dz, U0, sat0, bcs, p, dt, nsteps, dtype=np.longdouble, S0=0.0, seeded=True):
    """`nsteps` ForwardEuler steps of the heat + Richards SoilModel from (U0, sat0) [Nz][Nh] on the thickness `dz` (index 0 the surface
    layer); bcs: {(var, side): (kind, value [Nh] or scalar)} with var among temperature (value), internal_energy and
    saturation_water_ice (flux).  The initial saturation is taken as stored (a legal profile: the initial closure leaves it alone)."""
    dtype = np.dtype(dtype).type
    U0 = np.asarray(U0, dtype=np.float64)
    Nz, Nh = U0.shape
    ns = 2 * Nz

    def seed(x, first):
        x = np.asarray(x, dtype=np.float64).astype(dtype)
        if not seeded:
            return Dual(x)
        d = np.zeros(x.shape + (ns,), dtype=dtype)
        for r in range(Nz):
            d[r, :, first + r] = 1
        return Dual(x, d)

    g = grid(dz, Nh, dtype)
    c = LH.derived(p, dtype, LH.Seeds())
    h = hydraulics(p, dtype)
    bcs = {pair: (kind, np.broadcast_to(np.asarray(value, dtype=np.float64), (Nh,))) for pair, (kind, value) in bcs.items()}
    U, sat = seed(U0, 0), seed(sat0, Nz)
    S = np.broadcast_to(np.asarray(S0, dtype=np.float64), (Nh,)).astype(dtype)
    rec = Branches()
    T, liq, Ltheta = closure(c, U, sat)
    rec.add("regime", LH.regime_of(U.x, Ltheta), _near(U.x, 0.0, np.maximum(1.0, Ltheta)) | _near(U.x + Ltheta, 0.0, np.maximum(1.0, Ltheta)))
    psi, z0 = pressure_head(c, h, g, sat, rec)

    def snapshot():
        return dict(internal_energy=U.x, saturation=sat.x, temperature=T.x, liquid_water_fraction=liq.x, pressure_head=psi.x, water_table=z0,
                    surface_excess_water=S)

    trajectory, branches = [snapshot()], [rec]
    for _ in range(nsteps):
        rec = Branches()
        GU, GS = tendencies(c, h, g, U, sat, T, liq, psi, bcs, rec)
        U = U + GU * dtype(dt)
        sat, over = repair(g, sat + GS * dtype(dt), rec)
        S = (S + np.minimum(dtype(0), S) * dtype(dt)) + over
        psi, z0 = pressure_head(c, h, g, sat, rec)
        T, liq, Ltheta = closure(c, U, sat)
        rec.add("regime", LH.regime_of(U.x, Ltheta), _near(U.x, 0.0, np.maximum(1.0, Ltheta)) | _near(U.x + Ltheta, 0.0, np.maximum(1.0, Ltheta)))
        trajectory.append(snapshot())
        branches.append(rec)
    return Result(dict(zip(FIELDS, (U, sat, T, liq, psi))), trajectory, branches, Nz, Nh)


# ---- what a comparison needs ---------------------------------------------------------------------------------------------------------
def kept_columns(wide, narrow):
    """The branch mask: a column is left out only if at some cell and step the two evaluations (np.longdouble, np.float64) take
    different branches, or a value a branch tests lies within MARGIN (relative) of its threshold in either."""
    keep = np.ones(wide.Nh, dtype=bool)
    for bw, bn in zip(wide.branches, narrow.branches):
        for name in bw.taken:
            differ = bw.taken[name] != bn.taken[name]
            keep &= ~np.any(differ | bw.near[name] | bn.near[name], axis=0)
    return keep


def occurred(result, name, keep):
    """whether branch `name` was taken at some cell and step of a kept column"""
    return any(np.any(b.taken[name][:, keep]) for b in result.branches if name in b.taken)
