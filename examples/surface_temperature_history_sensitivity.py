#!/usr/bin/env python3
"""Sensitivity of a soil column to the HISTORY of the surface temperature that drives it: the column of
surface_temperature_sensitivity.py, its surface temperature now a record

    PrescribedSurfaceTemperature(:T_ub, FieldTimeSeries(times, values)), ForwardEuler, run! for N_t = 200 steps

and the question a borehole inversion asks: how does the final temperature profile respond to each node of the record?

Reverse mode answers it in one backward sweep: the cotangent of the final temperature profile, pulled back through the taped run
(trm.vjp with `wrt_boundary=True`), gives dL/d(node value) for every node of the record at once, in the record's shape.  Forward mode
answers one node per run: a seed of 1 on that node (trm.jvp with `d_boundary`) gives the response of every level to it.  The example
prints the node sensitivities and checks one node against the forward run.

    python examples/surface_temperature_history_sensitivity.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import terrarium_jl_amd as trm  # noqa: E402

N_T = 200
N_NODES = 9
SURFACE = ("temperature", "top")


def record(steps=N_T, nodes=N_NODES):
    """(times, values): a surface-temperature record over the run, a cooling trend with a warm spell"""
    dt = trm.ForwardEuler().dt
    times = np.linspace(0.0, steps * dt, nodes)
    values = 1.0 - 2.0 * times / times[-1] + 1.5 * np.exp(-((times / times[-1] - 0.6) / 0.15) ** 2)
    return times, values


def column(steps=N_T, nodes=N_NODES, num_columns=1):
    grid = trm.ColumnGrid(trm.ExponentialSpacing(), num_columns=num_columns)
    model = trm.SoilModel(grid, initializer=trm.SoilInitializer())
    times, values = record(steps, nodes)
    series = trm.FieldTimeSeries(times, np.repeat(values[:, None], num_columns, axis=1))
    bcs = trm.merge_boundary_conditions(trm.PrescribedSurfaceTemperature("T_ub", series))
    return trm.initialize(model, trm.ForwardEuler(), boundary_conditions=bcs), grid


def profile_weights(Nz):
    """the cotangent of the final temperature profile: L = the mean of the top five levels"""
    w = np.zeros((Nz, 1))
    w[-5:] = 1.0 / 5.0
    return w


def reverse(steps=N_T, nodes=N_NODES, checkpoint_every=16):
    """(dL/d(node value) as [nodes], node times): every node from one backward sweep"""
    integrator, grid = column(steps, nodes)
    _, g_boundary = trm.vjp(integrator, steps, temperature=profile_weights(grid.Nz), checkpoint_every=checkpoint_every, wrt_boundary=True)
    return g_boundary[SURFACE][:, 0], record(steps, nodes)[0]


def forward(node, steps=N_T, nodes=N_NODES):
    """dL/d(value of `node`) by one tangent run: a seed of 1 on that node alone"""
    integrator, grid = column(steps, nodes)
    seed = np.zeros((nodes, 1))
    seed[node] = 1.0
    tangents = trm.jvp(integrator, 0.0, steps, d_boundary={SURFACE: seed})
    return float(np.sum(profile_weights(grid.Nz) * tangents["temperature"]))


def main():
    g, times = reverse()
    print("  node   time / h   dL/d(T_ub at the node) by trm.vjp")
    for k, (t, s) in enumerate(zip(times, g)):
        print(f"  {k:4d}   {t / 3600.0:8.2f}   {s:14.6e}")
    node = int(np.argmax(np.abs(g)))
    f = forward(node)
    print(f"node {node} by trm.jvp: {f:.6e}; difference / sensitivity: {abs(f - g[node]) / abs(f):.3e}")


if __name__ == "__main__":
    main()
