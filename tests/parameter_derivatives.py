"""What the parameter-gradient tests share (test_parameter_gradient_host.py, test_gpu_parameter_gradient.py): the ten thermal parameters,
and the reference of the central-difference check -- Richardson-extrapolated central differences of the oracle on the uniform 0.1 m
grid of boundary_derivatives.py, computed once per case and shared."""
import functools

import numpy as np

from boundary_derivatives import FD_DZ, FD_KEEP_DISTANCE, FD_KEEP_SHARE, FD_NH, FD_NZ, FD_STEPS, HALOS, LD
from test_gpu_adjoint import cotangents
from test_gpu_tangent import DT, TANGENTS, boundary_sets, latent, mixed_state, params, regime_distance

PARAMS = ("k_water", "k_ice", "k_air", "k_mineral", "k_organic", "c_water", "c_ice", "c_air", "c_mineral", "c_organic")
CONDUCTIVITIES, CAPACITIES = PARAMS[:5], PARAMS[5:]
FD_SETS = ("T_top+flux_bottom", "flux_top+T_bottom", "gradient_top+flux_bottom")
RHO_SOC = (0.0, 26.0)       # 26 kg/m3: an organic fraction of 0.2
FD_CASES = [(bcset, halo, rho) for bcset in FD_SETS for halo in HALOS for rho in RHO_SOC]
FD_H_CAPACITY = 2e4         # J/m3/K; c_air - h is negative, which the oracle does not mind: C stays above 1e6


def fd_step(p, name):
    """the step of the central difference of parameter `name`"""
    return FD_H_CAPACITY if name in CAPACITIES else 1e-2 * min(1.0, getattr(p, name) / 2.0)


def thermal_params(halo="reference_zero", rho_soc=0.0):
    p = params(halo)
    p.rho_soc = rho_soc
    return p


def fd_inputs(bcset, halo, rho_soc):
    p = thermal_params(halo, rho_soc)
    U0, sat = mixed_state(FD_NZ, FD_NH, p, seed=3)
    bcs = {pair: (kind, np.broadcast_to(np.asarray(value, dtype=np.float64), (FD_NH,)).copy()) for pair, (kind, value) in boundary_sets(FD_NH)[bcset].items()}
    return p, U0, sat, bcs, cotangents(FD_NZ, FD_NH, 41)


def oracle_with(p, U0, sat, bcs, **moved):
    """the oracle of boundary_derivatives.oracle_on under the thermal parameters of `p`, those in `moved` replaced"""
    import oracle
    over = {name: getattr(p, name) for name in PARAMS}
    over.update(moved)
    o = oracle.Oracle(FD_NH, np.asarray(FD_DZ, dtype=np.float64), oracle.default_params(halo_policy=p.halo_policy, rho_soc=p.rho_soc, **over))
    o.set("saturation_water_ice", sat)
    o.set("internal_energy", U0)
    for (var, side), (kind, value) in bcs.items():
        o.set_bc(var, side, kind, value)
    o.closure()
    return o


def fd_run(p, U0, sat, bcs, name, delta):
    """the oracle's final (U, T, liq) with parameter `name` moved by `delta`"""
    o = oracle_with(p, U0, sat, bcs, **{name: getattr(p, name) + delta})
    for _ in range(FD_STEPS):
        o.timestep(DT)
    return {x: o.get(x).astype(LD) for x in TANGENTS}


def fd_kept_columns(p, U0, sat, bcs):
    """the columns whose cells stay more than FD_KEEP_DISTANCE from a regime boundary over the oracle's run"""
    L = latent(p, sat)
    o = oracle_with(p, U0, sat, bcs)
    dist = regime_distance(o.get("internal_energy"), L)
    for _ in range(FD_STEPS):
        o.timestep(DT)
        dist = np.minimum(dist, regime_distance(o.get("internal_energy"), L))
    return dist > FD_KEEP_DISTANCE


def central(p, U0, sat, bcs, name, h):
    plus, minus = fd_run(p, U0, sat, bcs, name, h), fd_run(p, U0, sat, bcs, name, -h)
    return {x: (plus[x] - minus[x]) / (2.0 * LD(h)) for x in TANGENTS}


def richardson(coarse, fine):
    """(4 fd(h / 2) - fd(h)) / 3, field by field"""
    return {x: (4.0 * fine[x] - coarse[x]) / 3.0 for x in TANGENTS}


def loss_and_scale(d, w):
    """(dL, S)[column] of the field derivatives d: sum_X sum_i w_X d_X and sum_X sum_i |w_X| |d_X|"""
    dL = sum(np.sum(w[x].astype(LD) * d[x], axis=0) for x in TANGENTS)
    S = sum(np.sum(np.abs(w[x]).astype(LD) * np.abs(d[x]), axis=0) for x in TANGENTS)
    return dL, S


@functools.lru_cache(maxsize=None)
def fd_reference(bcset, halo, rho_soc, levels=2):
    """The reference of a case, computed once: (inputs, keep, {name: [extrapolation at (h, h/2), at (h/2, h/4) if levels == 3]}), each
    extrapolation the dict of field derivatives dX_n/d(parameter) as [Nz][Nh] in extended precision.  Nothing in it is modified later."""
    p, U0, sat, bcs, w = fd_inputs(bcset, halo, rho_soc)
    keep = fd_kept_columns(p, U0, sat, bcs)
    ref = {}
    for name in PARAMS:
        h = fd_step(p, name)
        c = [central(p, U0, sat, bcs, name, h / 2 ** i) for i in range(levels)]
        ref[name] = [richardson(c[i], c[i + 1]) for i in range(levels - 1)]
    return (p, U0, sat, bcs, w), keep, ref
