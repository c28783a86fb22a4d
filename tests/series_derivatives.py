"""What the tests of the derivatives through boundary time series share (test_series_derivative_host.py, test_gpu_series_derivative.py):
the series -- node times per time indexing, node values around the boundary set's value -- and the inputs of the central-difference
check of the oracle, on the uniform grid of boundary_derivatives.py.

8 steps of DT from t = 0 under steps_per_launch = 3 (launches of 3, 3, 2), 4 nodes:
  linear, raster   [0, 2.5, 5, 7.5] DT     the bracket changes between launches (steps 2 | 3, 5 | 6) and inside one (4 -> 5); step 5 lands
                                           exactly on a node
  clamp            the same + 1.25 DT      the first two steps sit before the first node
  cyclical         [0, 1.5, 3, 4.5] DT     the period is 6 DT: the run wraps, step 5 sits between the last node and the first
"""
import numpy as np

import boundary_derivatives as B
from boundary_derivatives import LD
from test_gpu_tangent import DT, TANGENTS, boundary_sets, latent, regime_distance

NH, STEPS, SPL, NT = 48, 8, 3, 4
SIZES = (10, 32, 50)                # fewer than 32 lanes a column, exactly 32, the 64-lane layout with tail lanes
INDEXINGS = ("linear", "clamp", "cyclical", "raster")
SETS = ("T_top+flux_bottom", "flux_top+T_bottom")
AMPLITUDE = {"value": 2.0, "flux": 5.0}      # K, W/m2

FD_INDEXINGS = ("linear", "clamp", "cyclical")
FD_KEEP_SHARE = 0.80


def node_times(indexing, nt=NT, second=False):
    """the node times of a series; `second`: of the other pair where both pairs of a set carry one (other brackets in the same step)"""
    base = np.array([0.0, 1.5, 3.0, 4.5]) if indexing == "cyclical" else np.array([0.0, 2.5, 5.0, 7.5])
    if indexing == "clamp":
        base = base + 1.25
    if nt != NT:
        step = base[1] - base[0]
        base = base[0] + step * np.arange(nt)
    if second:
        base = base * 0.8 + (0.0 if indexing == "cyclical" else 0.25)
    return base * DT


def node_values(kind, base, Nh, nt=NT):
    """[nt][Nh]: the boundary set's value + A sin(1.3 k + 0.1 i)"""
    k, i = np.arange(nt)[:, None], np.arange(Nh)[None, :]
    return np.broadcast_to(np.asarray(base, dtype=np.float64), (Nh,))[None, :] + AMPLITUDE[kind] * np.sin(1.3 * k + 0.1 * i)


def series_on(bcs, pairs, indexing, Nh, nt=NT):
    """{pair: (kind, times, values, indexing)} for `pairs` of the boundary set `bcs`; the second pair gets other node times"""
    out = {}
    for n, pair in enumerate(pairs):
        kind, base = bcs[pair]
        out[pair] = (kind, node_times(indexing, nt, second=n > 0), node_values(kind, base, Nh, nt), indexing)
    return out


def attach(target, series):
    """the series onto a DeviceState or an Oracle (both: set_bc_series(var, side, kind, times, values, time_indexing))"""
    for (var, side), (kind, times, values, indexing) in series.items():
        target.set_bc_series(var, side, kind, times, values, indexing)


# ---- the central-difference check of the oracle ---------------------------------------------------------------------------------------
def fd_inputs(bcset, halo):
    """(p, U0, sat, bcs, w) on the grid FD_DZ x FD_NH: mixed_state(seed = 3), cotangents(.., 41)"""
    return B.fd_inputs(bcset, halo)


def fd_oracle(p, U0, sat, bcs, series):
    o = B.oracle_on(B.FD_DZ, B.FD_NH, p, U0, sat, bcs)
    attach(o, series)
    return o


def fd_kept_columns(p, U0, sat, bcs, series):
    """the columns whose cells stay more than FD_KEEP_DISTANCE from a regime boundary over the oracle's run of STEPS steps"""
    L = latent(p, sat)
    o = fd_oracle(p, U0, sat, bcs, series)
    dist = regime_distance(o.get("internal_energy"), L)
    for _ in range(STEPS):
        o.timestep(DT)
        dist = np.minimum(dist, regime_distance(o.get("internal_energy"), L))
    return dist > B.FD_KEEP_DISTANCE


def fd_run(p, U0, sat, bcs, series, pair, node, delta):
    """the oracle's final (U, T, liq) with node `node` of the series of `pair` moved by `delta` in every column"""
    kind, times, values, indexing = series[pair]
    moved = values.copy()
    moved[node] += delta
    o = fd_oracle(p, U0, sat, bcs, {**series, pair: (kind, times, moved, indexing)})
    for _ in range(STEPS):
        o.timestep(DT)
    return {name: o.get(name) for name in TANGENTS}


def fd_central(p, U0, sat, bcs, series, pair, node, w, h):
    """(plus, minus, fd, S) as boundary_derivatives.fd_central, for one node of a series"""
    plus, minus = fd_run(p, U0, sat, bcs, series, pair, node, h), fd_run(p, U0, sat, bcs, series, pair, node, -h)
    fd = sum(np.sum(w[x].astype(LD) * (plus[x].astype(LD) - minus[x].astype(LD)), axis=0) for x in TANGENTS) / (2.0 * h)
    S = sum(np.sum(np.abs(w[x]).astype(LD) * np.abs(plus[x].astype(LD) - minus[x].astype(LD)), axis=0) for x in TANGENTS) / (2.0 * h)
    return plus, minus, fd, S


def fd_cases():
    """(bcset, pair, indexing, halo): each of the two pairs of a set seriesed in turn"""
    out = []
    for bcset in SETS:
        for pair in B.active_pairs(boundary_sets(2)[bcset]):
            for indexing in FD_INDEXINGS:
                for halo in B.HALOS:
                    out.append((bcset, pair, indexing, halo))
    return out
