#!/usr/bin/env python3
"""Sensitivity of a soil column to its thermal parameters: the column of differentiating_soil_column.py

    ColumnGrid(ExponentialSpacing()), SoilModel(grid; initializer = SoilInitializer(...)), PrescribedSurfaceTemperature(:T_ub, 1.0),
    ForwardEuler, run! for N_t = 200 steps

and the question a calibration of soil thermal properties against a borehole temperature asks: how does the final temperature of
one level respond to each of the five conductivities and five heat capacities of the soil's constituents?

Reverse mode answers it in one run: a one-hot cotangent on T_f[level], pulled back through the taped run (trm.vjp with
`wrt_params=True`), gives all ten numbers.  Forward mode answers one parameter per run: a unit seed on the parameter, no seed on the
state (trm.jvp with `d_params`), gives dT_f[i] / d(parameter) for every level i.  The example prints both.

    python examples/thermal_parameter_sensitivity.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import terrarium_jl_amd as trm  # noqa: E402

N_T = 200
LEVEL = 3            # counted down from the surface (0: the top level); the fields are stored bottom first
PARAMETERS = trm._capi.THERMAL_PARAMS


def column():
    grid = trm.ColumnGrid(trm.ExponentialSpacing(), num_columns=1)
    model = trm.SoilModel(grid, initializer=trm.SoilInitializer())
    bcs = trm.merge_boundary_conditions(trm.PrescribedSurfaceTemperature("T_ub", 1.0))    # constant surface temperature of 1 degC
    return trm.initialize(model, trm.ForwardEuler(), boundary_conditions=bcs), grid


def reverse(steps=N_T, level=LEVEL, checkpoint_every=None):
    """{parameter: dT_f[level] / d(parameter)}: one backward sweep"""
    integrator, grid = column()
    seed = np.zeros((grid.Nz, 1))
    seed[grid.Nz - 1 - level, 0] = 1.0
    _, g = trm.vjp(integrator, steps, temperature=seed, checkpoint_every=checkpoint_every, wrt_params=True)
    return {name: float(g[name][0]) for name in PARAMETERS}


def forward(steps=N_T, level=LEVEL):
    """the same, one tangent run per parameter"""
    out = {}
    for name in PARAMETERS:
        integrator, grid = column()
        out[name] = float(trm.jvp(integrator, 0.0, steps, d_params={name: 1.0})["temperature"][grid.Nz - 1 - level, 0])
    return out


def main():
    g, t = reverse(), forward()
    _, grid = column()
    print(f"final temperature of level {LEVEL} below the surface (z = {grid.z_centers()[grid.Nz - 1 - LEVEL]:.3f} m) after {N_T} steps")
    print("  parameter    dT_f/d(parameter) by trm.vjp   the same by trm.jvp")
    for name in PARAMETERS:
        print(f"  {name:10s}   {g[name]:28.6e}   {t[name]:19.6e}")


if __name__ == "__main__":
    main()
