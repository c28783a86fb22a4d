#!/usr/bin/env python3
"""Sensitivity of a soil column to its thermal parameters AND to the history of the surface temperature that drives it, from one
backward sweep: the calibration run of a borehole inversion.  The column of surface_temperature_history_sensitivity.py,

    PrescribedSurfaceTemperature(:T_ub, FieldTimeSeries(times, values)), ForwardEuler, run! for N_t = 200 steps

and the loss L = the mean final temperature of the top five levels.  trm.vjp with `wrt_boundary=True, wrt_params=True` pulls the
cotangent of the final profile back through the checkpointed tape once and returns dL/dU_0, dL/d(node value) for every node of the
record, and dL/d(parameter) for the five conductivities and five heat capacities.  Forward mode answers one parameter per run
(trm.jvp with `d_params`) on the same record; the example checks every parameter gradient against it and prints the figures.

    python examples/thermal_parameter_history_sensitivity.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from surface_temperature_history_sensitivity import N_NODES, N_T, SURFACE, column, profile_weights, record  # noqa: E402
import terrarium_jl_amd as trm  # noqa: E402

PARAMS = trm._capi.THERMAL_PARAMS


def reverse(steps=N_T, nodes=N_NODES, checkpoint_every=16, num_columns=1):
    """(dL/dU_0 [Nz][Nh], dL/d(node value) [nodes][Nh], {parameter: dL/d(parameter) [Nh]}) from one backward sweep"""
    integrator, grid = column(steps, nodes, num_columns)
    w = np.repeat(profile_weights(grid.Nz), num_columns, axis=1)
    g, g_boundary, g_params = trm.vjp(integrator, steps, temperature=w, checkpoint_every=checkpoint_every, wrt_boundary=True, wrt_params=True)
    return g, g_boundary[SURFACE], g_params


def forward(name, steps=N_T, nodes=N_NODES, num_columns=1):
    """(dL/d(parameter `name`), S) per column by one tangent run of the same record: a seed of 1 on that parameter alone;
    S = sum |w| |tangent|, the scale a difference between the two modes is measured in"""
    integrator, grid = column(steps, nodes, num_columns)
    tangents = trm.jvp(integrator, 0.0, steps, d_params={name: 1.0})
    w = profile_weights(grid.Nz)
    return np.sum(w * tangents["temperature"], axis=0), np.sum(np.abs(w) * np.abs(tangents["temperature"]), axis=0)


def main():
    g, g_nodes, g_params = reverse()
    times = record()[0]
    print("  node   time / h   dL/d(T_ub at the node)")
    for k, (t, s) in enumerate(zip(times, g_nodes[:, 0])):
        print(f"  {k:4d}   {t / 3600.0:8.2f}   {s:14.6e}")
    print(f"  |dL/dU_0| summed over the column: {np.sum(np.abs(g)):.6e}")
    print("  parameter    dL/d(parameter) by trm.vjp   by trm.jvp       |difference| / sum |w| |tangent|")
    for name in PARAMS:
        f, scale = forward(name)
        rel = abs(f[0] - g_params[name][0]) / scale[0] if scale[0] != 0.0 else abs(g_params[name][0])
        print(f"  {name:10s}   {g_params[name][0]:14.6e}               {f[0]:14.6e}   {rel:.3e}")


if __name__ == "__main__":
    main()
