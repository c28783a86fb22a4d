"""What the boundary-gradient tests share (test_boundary_gradient_host.py, test_gpu_boundary_gradient.py): which boundary values the
heat-only step reads, and the inputs of the central-difference check of the oracle -- a uniform 0.1 m grid, where a perturbation of a
boundary value moves the internal energy by far more than its rounding (the exponential grid's 100 m bottom cell does not allow that)."""
import numpy as np

from test_gpu_adjoint import cotangents
from test_gpu_tangent import DT, TANGENTS, boundary_sets, latent, mixed_state, params, regime_distance

LD = np.longdouble
PAIRS = (("temperature", "bottom"), ("temperature", "top"), ("internal_energy", "bottom"), ("internal_energy", "top"))
READS = {"temperature": ("value", "gradient"), "internal_energy": ("flux",)}
HALOS = ("reference_zero", "mirror")

FD_NZ, FD_NH, FD_STEPS = 10, 64, 6
FD_DZ = [0.1] * FD_NZ
FD_SETS = ("T_top+flux_bottom", "flux_top+T_bottom", "gradient_top+flux_bottom", "gradient_bottom+T_top", "zero_gradient_bottom+T_top")
FD_H = {"value": 1e-3, "gradient": 1e-2, "flux": 1.0}       # K, K/m, W/m2
FD_KEEP_DISTANCE = 3e4      # J/m3 from a regime boundary over the run; the largest perturbation of U these steps cause is 9e3
FD_KEEP_SHARE = 0.85


def active_pairs(bcs):
    """the (var, side) pairs of a boundary set whose value the heat-only step reads"""
    return [pair for pair in PAIRS if pair in bcs and bcs[pair][0] in READS[pair[0]]]


def oracle_on(dz, Nh, p, U, sat, bcs):
    import oracle
    o = oracle.Oracle(Nh, np.asarray(dz, dtype=np.float64), oracle.default_params(halo_policy=p.halo_policy))
    o.set("saturation_water_ice", sat)
    o.set("internal_energy", U)
    for (var, side), (kind, value) in bcs.items():
        o.set_bc(var, side, kind, value)
    o.closure()
    return o


def fd_inputs(bcset, halo):
    p = params(halo)
    U0, sat = mixed_state(FD_NZ, FD_NH, p, seed=3)
    bcs = {pair: (kind, np.broadcast_to(np.asarray(value, dtype=np.float64), (FD_NH,)).copy()) for pair, (kind, value) in boundary_sets(FD_NH)[bcset].items()}
    return p, U0, sat, bcs, cotangents(FD_NZ, FD_NH, 41)


def fd_kept_columns(p, U0, sat, bcs):
    """the columns whose cells stay more than FD_KEEP_DISTANCE from a regime boundary over the oracle's run"""
    L = latent(p, sat)
    o = oracle_on(FD_DZ, FD_NH, p, U0, sat, bcs)
    dist = regime_distance(o.get("internal_energy"), L)
    for _ in range(FD_STEPS):
        o.timestep(DT)
        dist = np.minimum(dist, regime_distance(o.get("internal_energy"), L))
    return dist > FD_KEEP_DISTANCE


def fd_run(p, U0, sat, bcs, pair, delta):
    """the oracle's final (U, T, liq) with the boundary value of `pair` moved by `delta` in every column"""
    moved = dict(bcs)
    moved[pair] = (bcs[pair][0], bcs[pair][1] + delta)
    o = oracle_on(FD_DZ, FD_NH, p, U0, sat, moved)
    for _ in range(FD_STEPS):
        o.timestep(DT)
    return {name: o.get(name) for name in TANGENTS}


def fd_central(p, U0, sat, bcs, pair, w, h):
    """(plus, minus, fd, S): the runs at +-h, fd[column] = the central difference of the per-column loss sum_X sum_i w_X X_n, and
    S[column] = sum_X sum_i |w_X| |central difference of X_n|"""
    plus, minus = fd_run(p, U0, sat, bcs, pair, h), fd_run(p, U0, sat, bcs, pair, -h)
    fd = sum(np.sum(w[x].astype(LD) * (plus[x].astype(LD) - minus[x].astype(LD)), axis=0) for x in TANGENTS) / (2.0 * h)
    S = sum(np.sum(np.abs(w[x]).astype(LD) * np.abs(plus[x].astype(LD) - minus[x].astype(LD)), axis=0) for x in TANGENTS) / (2.0 * h)
    return plus, minus, fd, S
