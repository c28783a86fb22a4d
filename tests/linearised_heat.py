"""An exact linearisation of the heat-only ForwardEuler step in numpy: the reference of test_linearised_heat_host.py and
test_gpu_derivative_edges.py.

The step is restated once, from oracle/terrarium_oracle.hpp, over the dual type `Dual` = (x, d[..., nseed]): the value
and its derivatives with respect to every seeded input, in the dtype the caller chooses (np.float64 or np.longdouble).  Derivatives
come from operator overloading alone; `where` on the primal's condition keeps the derivative of the branch taken, which is what
Enzyme gives the reference.  Nothing here is taken from the device's hand-written tangent or adjoint.

What can carry a seed: the initial internal energy (one seed per level: columns are independent, so seed j is level j of every
column), the four boundary values, the ten thermal parameters (pushed through the map to the eight numbers the kernels hold: sk_water,
sk_ice, sk_air, s0, c_water, c_ice, c_air, C0), and the nodes of a boundary series (`linear`, `clamp`, `cyclical`).

Arrays are [Nz][Nh], row 0 the bottom layer, as everywhere in the tests."""
import math

import numpy as np

TANGENTS = ("internal_energy", "temperature", "liquid_water_fraction")
PAIRS = (("temperature", "bottom"), ("temperature", "top"), ("internal_energy", "bottom"), ("internal_energy", "top"))
PARAMS = ("k_water", "k_ice", "k_air", "k_mineral", "k_organic", "c_water", "c_ice", "c_air", "c_mineral", "c_organic")
CONSTANTS = ("rho_w", "Lsl", "por_mineral", "por_organic", "rho_soc", "rho_org")
THAWED, PHASE_CHANGE, FROZEN = 0, 1, 2
EPS = float(np.finfo(np.float64).eps)       # safediv's eps(NF) is the model's (Float64) in either arithmetic


# ---- the dual type -----------------------------------------------------------------------------------------------------------------
class Dual:
    """x[...] and d[..., nseed] = dx / d(seed); d is None for a constant"""
    __slots__ = ("x", "d")
    __array_ufunc__ = None      # numpy leaves `array op Dual` to the reflected operators below

    def __init__(self, x, d=None):
        self.x, self.d = np.asarray(x), d

    @staticmethod
    def lift(a):
        return a if isinstance(a, Dual) else Dual(a)

    def _scaled(self, factor):
        """d * factor[..., None]"""
        return None if self.d is None else self.d * np.asarray(factor)[..., None]

    @staticmethod
    def _sum(a, b):
        return b if a is None else a if b is None else a + b

    def __neg__(self):
        return Dual(-self.x, None if self.d is None else -self.d)

    def __add__(self, o):
        o = Dual.lift(o)
        return Dual(self.x + o.x, Dual._sum(self.d, o.d))

    __radd__ = __add__

    def __sub__(self, o):
        return self + (-Dual.lift(o))

    def __rsub__(self, o):
        return Dual.lift(o) + (-self)

    def __mul__(self, o):
        o = Dual.lift(o)
        return Dual(self.x * o.x, Dual._sum(self._scaled(o.x), o._scaled(self.x)))

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Dual.lift(o)
        q = self.x / o.x
        return Dual(q, Dual._sum(self._scaled(1 / o.x), o._scaled(-(q / o.x))))

    def __rtruediv__(self, o):
        return Dual.lift(o) / self

    def sqrt(self):
        r = np.sqrt(self.x)
        return Dual(r, self._scaled(1 / (2 * r)))

    def rounded_to(self, dtype):
        """the value stored in `dtype` (a linear map on the derivative: it keeps its own dtype)"""
        return Dual(self.x.astype(dtype), self.d)

    def full(self):
        """d in the shape x.shape + (nseed,) (a product with a scalar dual leaves it broadcastable only)"""
        return None if self.d is None else np.broadcast_to(self.d, self.x.shape + self.d.shape[-1:])

    def __getitem__(self, key):
        return Dual(self.x[key], None if self.d is None else self.full()[key])


def where(cond, a, b):
    """the branch the primal takes, and that branch's derivative"""
    a, b = Dual.lift(a), Dual.lift(b)
    x = np.where(cond, a.x, b.x)
    if a.d is None and b.d is None:
        return Dual(x)
    ns = (a.d if a.d is not None else b.d).shape[-1]
    zero = np.zeros(ns, dtype=x.dtype)
    da = a.d if a.d is not None else zero
    db = b.d if b.d is not None else zero
    return Dual(x, np.where(np.asarray(cond)[..., None], da, db))


def stack_levels(bottom, interior, top):
    """[1 + Nz + 1][Nh]: the halo rows around a field"""
    parts = [bottom, interior, top]
    rows = [q.x[None] if q.x.ndim == 1 else q.x for q in parts]
    x = np.concatenate(rows, axis=0)
    if all(q.d is None for q in parts):
        return Dual(x)
    ns = next(q.d for q in parts if q.d is not None).shape[-1]
    ds = [np.zeros(r.shape + (ns,), dtype=x.dtype) if q.d is None else np.broadcast_to(q.d, r.shape + (ns,)) for q, r in zip(parts, rows)]
    return Dual(x, np.concatenate(ds, axis=0))


# ---- seeds -------------------------------------------------------------------------------------------------------------------------
class Seeds:
    """which slice of the seed axis belongs to which input: "state" (Nz), ("boundary", pair) (1), "params" (10), ("series", pair) (nt)"""

    def __init__(self):
        self.slices, self.n = {}, 0

    def add(self, key, count):
        self.slices[key] = slice(self.n, self.n + count)
        self.n += count


# ---- the grid (Grid::build of the oracle) --------------------------------------------------------------------------------------------
def grid(dz, Nh, dtype):
    """thickness index 0 is the surface layer, as get_spacing gives it; cells 1..Nz bottom to top, 0 and Nz + 1 the halos"""
    dz = np.asarray(dz, dtype=np.float64)
    Nz = dz.size
    cs = np.zeros(Nz)
    s = dz[0]
    cs[0] = s
    for i in range(1, Nz):
        s = s + dz[i]
        cs[i] = s
    zF = np.zeros(Nz + 3, dtype=dtype)
    for k in range(1, Nz + 1):
        zF[k] = dtype(-cs[Nz - k])
    zF[0] = zF[1] - (zF[2] - zF[1])
    zF[Nz + 2] = zF[Nz + 1] + (zF[Nz + 1] - zF[Nz])
    zC = (zF[1:] + zF[:-1]) / dtype(2)          # 0..Nz+1
    dzc = zF[1:] - zF[:-1]                      # 0..Nz+1
    dzf = np.zeros(Nz + 2, dtype=dtype)
    dzf[1:] = zC[1:] - zC[:-1]                  # 1..Nz+1
    rdzf = np.zeros(Nz + 2, dtype=dtype)
    rdzf[1:] = dtype(1) / dzf[1:]
    return dict(Nz=Nz, dzc=dzc, dzf=dzf, rdzc=dtype(1) / dzc, rdzf=rdzf, dx=dtype(np.float64(1.0 / Nh)))


# ---- time indexing of a series (FieldTimeSeries; interpolating_time_indices of the oracle, in Float64 like the reference) -----------
def find_time_index(times, t):
    low, high = 0, len(times) - 1
    while low + 1 < high:
        mid = (low + high) // 2
        if times[mid] == t:
            return 0.0, mid, mid
        if times[mid] < t:
            low = mid
        else:
            high = mid
    return float(high - low) / (times[high] - times[low]) * (t - times[low]), low, high


def time_indices(times, indexing, t):
    """(f, n1, n2): the value at t is v[n2] f + v[n1] (1 - f), v[n1] alone where n1 == n2"""
    times = [float(x) for x in times]
    Nt = len(times)
    if Nt == 1:
        return 0.0, 0, 0
    if indexing == "cyclical":
        t1, tN = times[0], times[-1]
        T = (tN - t1) + (tN - times[-2])
        mod_tau = math.fmod(t - t1, T)
        if mod_tau < 0:
            mod_tau += T
        mod_t = mod_tau + t1
        if mod_t > tN:
            return 1.0 / (T - (tN - t1)) * (mod_t - tN), Nt - 1, 0
        return find_time_index(times, mod_t)
    if indexing not in ("linear", "clamp"):
        raise ValueError(f"time indexing {indexing!r} is not restated here")
    f, n1, n2 = find_time_index(times, t)
    if indexing == "clamp":
        if t >= times[-1]:
            return 0.0, Nt - 1, Nt - 1
        if t <= times[0]:
            return 0.0, 0, 0
    return f, n1, n2


def series_value(nodes, times, indexing, t, dtype):
    """the boundary value of a step from the node values `nodes` [nt][Nh]: the products are formed in Float64 for every arithmetic, as
    the reference (and the oracle's update_inputs) forms them, then stored in the arithmetic's type"""
    f, n1, n2 = time_indices(times, indexing, t)
    if n1 == n2:
        return nodes[n1]
    v1, v2 = nodes[n1].rounded_to(np.float64), nodes[n2].rounded_to(np.float64)
    return (v2 * np.float64(f) + v1 * np.float64(1.0 - f)).rounded_to(dtype)


# ---- the physics ---------------------------------------------------------------------------------------------------------------------
def derived(p, dtype, seeds):
    """The constants of a run: organic fraction, porosity, L = rho_w Lsl, and the eight numbers the ten thermal parameters reach the
    step through -- sk_water, sk_ice, sk_air, s0 = sqrt(k_mineral) frac_mineral + sqrt(k_organic) frac_organic, c_water, c_ice, c_air,
    C0 = c_mineral frac_mineral + c_organic frac_organic -- as duals seeded on the ten parameters themselves."""
    c = {name: dtype(getattr(p, name)) for name in CONSTANTS}
    org = c["rho_soc"] / ((dtype(1) - c["por_organic"]) * c["rho_org"])
    por = (dtype(1) - org) * c["por_mineral"] + org * c["por_organic"]
    solid = dtype(1) - por
    frac_organic, frac_mineral = solid * org, solid * (dtype(1) - org)
    q = {}
    for n, name in enumerate(PARAMS):
        d = None
        if "params" in seeds.slices:
            d = np.zeros(seeds.n, dtype=dtype)
            d[seeds.slices["params"].start + n] = 1
        q[name] = Dual(dtype(getattr(p, name)), d)
    return dict(por=por, L=c["rho_w"] * c["Lsl"],
                sk_water=q["k_water"].sqrt(), sk_ice=q["k_ice"].sqrt(), sk_air=q["k_air"].sqrt(),
                s0=q["k_mineral"].sqrt() * frac_mineral + q["k_organic"].sqrt() * frac_organic,
                c_water=q["c_water"], c_ice=q["c_ice"], c_air=q["c_air"],
                C0=q["c_mineral"] * frac_mineral + q["c_organic"] * frac_organic)


def fractions(c, sat, liq):
    """volumetric_fractions: (water, ice, air); the mineral and organic shares are in s0 and C0"""
    one = sat.dtype.type(1)
    water_ice = sat * c["por"]
    return liq * water_ice, (one - liq) * water_ice, (one - sat) * c["por"]


def conductivity(c, sat, liq):
    """kappa = s^2 (InverseQuadratic)"""
    water, ice, air = fractions(c, sat, liq)
    s = c["sk_water"] * water + c["sk_ice"] * ice + c["sk_air"] * air + c["s0"]
    return s * s


def regime_of(U, Ltheta):
    """per cell: THAWED (U >= 0), PHASE_CHANGE (-L_theta <= U < 0), FROZEN (U < -L_theta)"""
    return np.where(U >= 0, THAWED, np.where(U >= -Ltheta, PHASE_CHANGE, FROZEN))


def closure(c, U, sat):
    """(T, liq) of the FreeWater energy closure: liquid_water_fraction, heat_capacity, energy_to_temperature"""
    dtype = sat.dtype.type
    Ltheta = c["L"] * sat * c["por"]
    melting = dtype(1) - U / (-Ltheta + dtype(EPS))            # safediv(U, -L_theta); with L_theta = 0 no U < 0 passes U >= -L_theta
    liq = where(U.x >= 0, dtype(1), where(U.x >= -Ltheta, melting, dtype(0)))
    water, ice, air = fractions(c, sat, liq)
    C = c["c_water"] * water + c["c_ice"] * ice + c["c_air"] * air + c["C0"]
    T = where(U.x < -Ltheta, (U + Ltheta) / C, where(U.x >= 0, U / C, dtype(0)))
    return T, liq


def halo_value(kind, value, edge, spacing, top):
    """fill_halo of a centred field: Value extrapolates through the boundary value, Gradient adds g * spacing, everything else copies"""
    dtype = spacing.dtype.type
    if kind == "value":
        grad = (value - edge) / (spacing / dtype(2)) if top else (edge - value) / (spacing / dtype(2))
        return edge + grad * (spacing if top else -spacing)
    if kind == "gradient":
        return edge + value * (spacing if top else -spacing)
    return edge


def tendency(c, g, U, T, liq, sat, bc, mirror):
    """dU/dt of compute_tendencies plus the Flux terms of explicit_step; bc = {pair: (kind, value)}"""
    Nz = g["Nz"]
    dtype = sat.dtype.type
    kind = {pair: bc[pair][0] if pair in bc else "noflux" for pair in PAIRS}
    value = {pair: bc[pair][1] if pair in bc else None for pair in PAIRS}
    Tb = halo_value(kind[PAIRS[0]], value[PAIRS[0]], T[0], g["dzf"][1], top=False)
    Tt = halo_value(kind[PAIRS[1]], value[PAIRS[1]], T[Nz - 1], g["dzf"][Nz + 1], top=True)
    Th = stack_levels(Tb, T, Tt)
    # the halo cells: liq copies the edge; sat is the edge's under the mirror policy and stays 0 (a dry cell) under reference_zero
    dry = np.zeros_like(sat[0])
    sat_h = np.concatenate([(sat[0] if mirror else dry)[None], sat, (sat[Nz - 1] if mirror else dry)[None]], axis=0)
    liq_h = stack_levels(liq[0], liq, liq[Nz - 1])
    kap = conductivity(c, sat_h, liq_h)
    rdzf = g["rdzf"][1:, None]                                        # faces 1..Nz+1
    q = -((kap[1:] + kap[:-1]) * dtype(0.5)) * ((Th[1:] - Th[:-1]) * rdzf)
    G = -((q[1:] - q[:-1]) * g["rdzc"][1:Nz + 1, None])
    Az = g["dx"]
    bottom = np.arange(Nz)[:, None] == 0
    top = np.arange(Nz)[:, None] == Nz - 1
    if kind[PAIRS[2]] == "flux":
        G = G + where(bottom, value[PAIRS[2]] * Az / (Az * g["dzc"][1]), dtype(0))
    if kind[PAIRS[3]] == "flux":
        G = G - where(top, value[PAIRS[3]] * Az / (Az * g["dzc"][Nz]), dtype(0))
    return G


class Result:
    """final: {field: Dual [Nz][Nh]}; trajectory: per state 0..n the primal {field: [Nz][Nh]}; regimes: per state [Nz][Nh]; L_theta;
    seeds: the Seeds of the run"""

    def __init__(self, final, trajectory, regimes, Ltheta, seeds, Nh):
        self.final, self.trajectory, self.regimes, self.Ltheta, self.seeds, self.Nh = final, trajectory, regimes, Ltheta, seeds, Nh

    def value(self, name):
        return self.final[name].x

    def block(self, key):
        """{field: dX_n / d(input)}: "state" -> [Nz out][Nz in][Nh]; ("boundary", pair) -> [Nz][Nh]; "params" -> [Nz][10][Nh];
        ("series", pair) -> [Nz][nt][Nh].  Zeros for an input that carries no seed (a pair the boundary set does not hold)."""
        out = {}
        boundary = isinstance(key, tuple) and key[0] == "boundary"
        for name in TANGENTS:
            q = self.final[name]
            if key not in self.seeds.slices:
                assert boundary, key
                out[name] = np.zeros(q.x.shape, dtype=q.x.dtype)
                continue
            d = q.full()[..., self.seeds.slices[key]]
            out[name] = d[..., 0].copy() if boundary else np.ascontiguousarray(np.moveaxis(d, -1, 1))
        return out


def run(dz, U0, sat, bcs, p, dt, nsteps, dtype=np.longdouble, mirror=False, series=None, seed=("state", "boundary", "params", "series")):
    """`nsteps` ForwardEuler steps of the heat-only SoilModel from (U0, sat) [Nz][Nh] on the thickness `dz` (index 0 the surface layer).

    bcs: {(var, side): (kind, value [Nh] or scalar)}; series: {(var, side): (kind, times, node values [nt][Nh], indexing)}, which
    replaces that pair's constant value from t = 0 on; p: anything with the ten thermal parameters and CONSTANTS as attributes; mirror:
    the halo policy.  `seed` names the inputs that carry seeds."""
    dtype = np.dtype(dtype).type
    series = series or {}
    U0 = np.asarray(U0, dtype=np.float64)
    Nz, Nh = U0.shape
    seeds = Seeds()
    if "state" in seed:
        seeds.add("state", Nz)
    if "boundary" in seed:
        for pair in PAIRS:
            if pair in bcs and pair not in series:
                seeds.add(("boundary", pair), 1)
    if "params" in seed:
        seeds.add("params", len(PARAMS))
    if "series" in seed:
        for pair, (_, times, _, _) in series.items():
            seeds.add(("series", pair), len(times))

    def seeded(x, key, rows):
        """x [rows][Nh] (rows = 0: [Nh]) with seed r of `key` on row r of every column"""
        x = np.asarray(x, dtype=np.float64).astype(dtype)
        if key not in seeds.slices:
            return Dual(x)
        d = np.zeros(x.shape + (seeds.n,), dtype=dtype)
        sl = seeds.slices[key]
        if rows == 0:
            d[..., sl.start] = 1
        else:
            for r in range(rows):
                d[r, :, sl.start + r] = 1
        return Dual(x, d)

    g = grid(dz, Nh, dtype)
    c = derived(p, dtype, seeds)
    sat = np.asarray(sat, dtype=np.float64).astype(dtype)
    Ltheta = c["L"] * sat * c["por"]
    constant = {pair: (kind, seeded(np.broadcast_to(np.asarray(value, dtype=np.float64), (Nh,)), ("boundary", pair), 0)) for pair, (kind, value) in bcs.items()}
    nodes = {pair: seeded(values, ("series", pair), len(times)) for pair, (_, times, values, _) in series.items()}

    U = seeded(U0, "state", Nz)
    T, liq = closure(c, U, sat)
    trajectory = [dict(zip(TANGENTS, (U.x, T.x, liq.x)))]
    regimes = [regime_of(U.x, Ltheta)]
    time = 0.0
    for _ in range(nsteps):
        bc = dict(constant)
        for pair, (kind, times, _, indexing) in series.items():
            bc[pair] = (kind, series_value(nodes[pair], times, indexing, time, dtype))
        U = U + tendency(c, g, U, T, liq, sat, bc, mirror) * dtype(dt)
        T, liq = closure(c, U, sat)
        time += float(dt)
        trajectory.append(dict(zip(TANGENTS, (U.x, T.x, liq.x))))
        regimes.append(regime_of(U.x, Ltheta))
    return Result(dict(zip(TANGENTS, (U, T, liq))), trajectory, regimes, Ltheta, seeds, Nh)


# ---- what a comparison needs ---------------------------------------------------------------------------------------------------------
def kept_columns(wide, narrow, margin=1e-6):
    """The regime mask: a column is left out only if at some cell and step the two evaluations (np.longdouble, np.float64) take
    different regimes, or the wide internal energy comes within margin * max(1, L_theta) of a regime boundary (U = 0, U = -L_theta)."""
    keep = np.ones(wide.Nh, dtype=bool)
    tol = margin * np.maximum(1.0, wide.Ltheta)
    for state, rw, rn in zip(wide.trajectory, wide.regimes, narrow.regimes):
        U = state["internal_energy"]
        near = (np.abs(U) <= tol) | (np.abs(U + wide.Ltheta) <= tol)
        keep &= ~np.any(near | (rw != rn), axis=0)
    return keep


def contraction_error(J, J_wide, v, axes):
    """(err, ref, S) of the contraction einsum(axes, J, v) against the same contraction of J_wide in extended precision, normalised by
    S = einsum(axes, |J_wide|, |v|); where S is zero the value must be zero too"""
    LD = np.longdouble
    ref = np.einsum(axes, J_wide.astype(LD), np.asarray(v).astype(LD))
    S = np.einsum(axes, np.abs(J_wide).astype(LD), np.abs(np.asarray(v)).astype(LD))
    got = np.einsum(axes, J.astype(LD), np.asarray(v).astype(LD))
    zero = S == 0
    assert np.all(got[zero] == 0), "a non-zero value where every product of the reference is zero"
    err = 0.0 if zero.all() else float(np.max(np.abs(got - ref)[~zero] / S[~zero]))
    return err, ref, S
