#!/usr/bin/env python3
"""Forward-mode sensitivity of a soil column with heat AND water -- the setup of the reference's test/differentiability/soil_hydrology_diff.jl:

    ColumnGrid(ExponentialSpacing(N = 10)), SoilModel(grid; soil = SoilEnergyWaterCarbon(hydrology = SoilHydrology(RichardsEq())),
    initializer = SoilInitializer()), ForwardEuler, timestep!(integrator, 60.0)

The reference takes Enzyme through one `timestep!` of this model.  Here the tangent of the heat + Richards step runs forward on the
device (trm.jvp with a dict of state seeds): the columns of one launch are independent, so 2 Nz replicas of the column -- replica k seeded
one-hot in the internal energy of level k, replica Nz + k one-hot in the saturation of level k -- give every column of the Jacobian of
the final state with respect to the initial (U, sat) at once, for each of the five fields the tangent carries.

    python examples/differentiating_soil_water_column.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import terrarium_jl_amd as trm  # noqa: E402

N, DT, STEPS = 10, 60.0, 10


def jacobian(steps=STEPS, saturation=0.5):
    """({field: J [Nz out][2 Nz in]}, z): J[:, k] = d field_f / d U_0[k], J[:, Nz + k] = d field_f / d sat_0[k] after `steps` steps of 60 s.
    The column starts at a constant saturation of 0.5, as the reference's closure test sets it (the default initializer saturates
    every cell, where the pressure head has no slope)."""
    spacing = trm.ExponentialSpacing(N=N)
    grid = trm.ColumnGrid(spacing, num_columns=2 * N)             # 2 Nz replicas of the one column
    soil = trm.SoilEnergyWaterCarbon(hydrology=trm.SoilHydrology(vertical_flow=trm.RichardsEq()))
    initializer = trm.SoilInitializer(hydrology=trm.ConstantSaturation(saturation))
    model = trm.SoilModel(grid, soil=soil, initializer=initializer)
    integrator = trm.initialize(model, trm.ForwardEuler(dt=DT))
    d_U = np.concatenate([np.eye(N), np.zeros((N, N))], axis=1)   # replica k: dU_0 = e_k
    d_sat = np.concatenate([np.zeros((N, N)), np.eye(N)], axis=1)  # replica Nz + k: dsat_0 = e_k
    tangents = trm.jvp(integrator, {"internal_energy": d_U, "saturation": d_sat}, steps)
    return tangents, grid.z_centers()


def main():
    J, zs = jacobian()
    top = N - 1
    print(f"after {STEPS} steps of {DT:g} s: sensitivities of the top cell's final state to the initial saturation")
    print("  depth / m   dsat_f[top]/dsat_0   dpsi_f[top]/dsat_0   dT_f[top]/dsat_0   dU_f[top]/dsat_0")
    for k in range(N - 1, -1, -1):
        print(f"  {zs[k]:9.3f}   {J['saturation'][top, N + k]:18.6e}   {J['pressure_head'][top, N + k]:18.6e}   "
              f"{J['temperature'][top, N + k]:16.6e}   {J['internal_energy'][top, N + k]:16.6e}")
    finite = all(bool(np.all(np.isfinite(j))) for j in J.values())
    print(f"five Jacobians {J['saturation'].shape}, finite: {finite}")


if __name__ == "__main__":
    main()
