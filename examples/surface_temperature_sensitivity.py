#!/usr/bin/env python3
"""Sensitivity of a soil column to the surface temperature that drives it: the column of differentiating_soil_column.py

    ColumnGrid(ExponentialSpacing()), SoilModel(grid; initializer = SoilInitializer(...)), PrescribedSurfaceTemperature(:T_ub, 1.0),
    ForwardEuler, run! for N_t = 200 steps

and the question a calibration or an assimilation of a forcing asks: how do the final temperatures respond to T_ub?

Forward mode answers it in one run: a seed of 1 on the boundary value, no seed on the state (trm.jvp with `d_boundary`), gives
dT_f[i] / dT_ub for every level i.  Reverse mode answers one level per run: a one-hot cotangent on T_f[i], pulled back through the
taped run (trm.vjp with `wrt_boundary=True`), gives the same number as its boundary gradient.  The example prints both.

    python examples/surface_temperature_sensitivity.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import terrarium_jl_amd as trm  # noqa: E402

N_T = 200
SURFACE = ("temperature", "top")


def column(num_columns=1):
    spacing = trm.ExponentialSpacing()
    grid = trm.ColumnGrid(spacing, num_columns=num_columns)
    model = trm.SoilModel(grid, initializer=trm.SoilInitializer())
    bcs = trm.merge_boundary_conditions(trm.PrescribedSurfaceTemperature("T_ub", 1.0))    # constant surface temperature of 1 degC
    return trm.initialize(model, trm.ForwardEuler(), boundary_conditions=bcs), grid


def forward(steps=N_T):
    """(dT_f / dT_ub as [Nz], z): one tangent run, the seed on the surface temperature alone"""
    integrator, grid = column()
    tangents = trm.jvp(integrator, 0.0, steps, d_boundary={SURFACE: 1.0})
    return tangents["temperature"][:, 0], grid.z_centers()


def reverse(steps=N_T, levels=None, checkpoint_every=None):
    """dT_f[i] / dT_ub for i in `levels` (default: all), one backward sweep each: replica k of the column carries the one-hot cotangent
    of level levels[k], so the sweeps share one launch"""
    Nz = len(trm.ExponentialSpacing().get_spacing())
    levels = list(range(Nz)) if levels is None else list(levels)
    integrator, _ = column(num_columns=len(levels))
    seed = np.zeros((Nz, len(levels)))
    seed[levels, np.arange(len(levels))] = 1.0
    _, g_boundary = trm.vjp(integrator, steps, temperature=seed, checkpoint_every=checkpoint_every, wrt_boundary=True)
    return g_boundary[SURFACE]


def main():
    dT, zs = forward()
    g = reverse()
    print("  depth / m   dT_f/dT_ub by trm.jvp   the same by trm.vjp")
    for z, a, r in zip(zs[::-1], dT[::-1], g[::-1]):
        print(f"  {z:9.3f}   {a:21.6e}   {r:19.6e}")
    scale = np.max(np.abs(dT))
    print(f"largest difference / largest sensitivity: {float(np.max(np.abs(dT - g)) / scale):.3e}")


if __name__ == "__main__":
    main()
