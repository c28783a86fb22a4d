#!/usr/bin/env python3
"""Reverse-mode gradient of a soil column with heat AND water -- the call of the reference's test/differentiability/soil_hydrology_diff.jl,
Enzyme.autodiff(Reverse, ...), on the setup of examples/differentiating_soil_water_column.py:

    ColumnGrid(ExponentialSpacing(N = 10)), SoilModel(grid; soil = SoilEnergyWaterCarbon(hydrology = SoilHydrology(RichardsEq())),
    initializer = SoilInitializer()), ForwardEuler, timestep!(integrator, 60.0)

The loss is the saturation of one cell after ten steps of 60 s: a one-hot cotangent on the final saturation.  One backward sweep on the
device (trm.vjp with a dict of cotangents) gives its gradient with respect to the whole initial state, dL/dU_0 and dL/dsat_0.  The same
numbers are one row of the Jacobian that forward mode builds from 2 Nz one-hot tangent runs (trm.jvp on 2 Nz replicas of the column):
both are printed side by side.

    python examples/soil_water_gradient.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import terrarium_jl_amd as trm  # noqa: E402

N, DT, STEPS, CELL = 10, 60.0, 10, 7


def column(num_columns, saturation=0.5):
    grid = trm.ColumnGrid(trm.ExponentialSpacing(N=N), num_columns=num_columns)
    soil = trm.SoilEnergyWaterCarbon(hydrology=trm.SoilHydrology(vertical_flow=trm.RichardsEq()))
    # (an unsaturated column: the default initializer saturates every cell, where the pressure head has no slope)
    model = trm.SoilModel(grid, soil=soil, initializer=trm.SoilInitializer(hydrology=trm.ConstantSaturation(saturation)))
    return trm.initialize(model, trm.ForwardEuler(dt=DT)), grid


def gradient(cell=CELL, steps=STEPS):
    """(dL/dU_0 [Nz], dL/dsat_0 [Nz]) of L = sat_n[cell], from one backward sweep"""
    integrator, _ = column(1)
    w = np.zeros((N, 1))
    w[cell] = 1.0
    g = trm.vjp(integrator, steps, internal_energy={"saturation": w})
    return g["internal_energy"][:, 0], g["saturation"][:, 0]


def jacobian_row(cell=CELL, steps=STEPS):
    """the same row from forward mode: 2 Nz one-hot tangent runs, as replicas of the column in one launch"""
    integrator, grid = column(2 * N)
    d_U = np.concatenate([np.eye(N), np.zeros((N, N))], axis=1)
    d_sat = np.concatenate([np.zeros((N, N)), np.eye(N)], axis=1)
    row = trm.jvp(integrator, {"internal_energy": d_U, "saturation": d_sat}, steps)["saturation"][cell]
    return row[:N], row[N:], grid.z_centers()


def main():
    gU, gsat = gradient()
    jU, jsat, zs = jacobian_row()
    print(f"L = saturation of cell {CELL} (z = {zs[CELL]:.3f} m) after {STEPS} steps of {DT:g} s")
    print("  depth / m    dL/dU_0 (vjp)    row of J (jvp)    dL/dsat_0 (vjp)    row of J (jvp)")
    for k in range(N - 1, -1, -1):
        print(f"  {zs[k]:9.3f}   {gU[k]:14.6e}   {jU[k]:14.6e}   {gsat[k]:16.6e}   {jsat[k]:14.6e}")
    scale = max(np.max(np.abs(jU)), np.max(np.abs(jsat)))
    worst = max(np.max(np.abs(gU - jU)), np.max(np.abs(gsat - jsat)))
    print(f"largest difference between the two modes: {worst:.3e} (largest entry {scale:.3e}); one sweep against {2 * N} tangent runs")


if __name__ == "__main__":
    main()
