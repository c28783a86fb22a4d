#!/usr/bin/env python3
"""Forward- and reverse-mode sensitivity of a soil column -- the twin of the reference's examples/autodiff/differentiating_terrarium.jl:

    ColumnGrid(ExponentialSpacing()), SoilModel(grid; initializer = SoilInitializer(...)), PrescribedSurfaceTemperature(:T_ub, 1.0),
    ForwardEuler, run! for N_t = 200 steps; sensitivity of the final temperature to the initial internal energy

The reference runs Enzyme in reverse mode with a one-hot seed on the final temperature of the second-lowest layer, which gives one ROW
of the Jacobian J = dT_f / dU_0.  Here the tangent of the step runs forward on the device (trm.jvp): every column of one launch is
independent, so Nz replicas of the column, replica k seeded one-hot at level k, give every COLUMN of J at once -- the whole Jacobian.
Its row 1 (row 0 is the bottom layer) is the vector the reference's autodiff call computes.

`gradient` does what the reference does: one column, a one-hot cotangent on the final temperature of the second-lowest layer, pulled
back through the taped run in one backward sweep (trm.vjp).  It is printed beside row 1 of the Jacobian.

    python examples/differentiating_soil_column.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import terrarium_jl_amd as trm  # noqa: E402

N_T = 200


def jacobian(steps=N_T):
    """(J_T, J_U, z): J_T[i, k] = dT_f[i] / dU_0[k], J_U[i, k] = dU_f[i] / dU_0[k] after `steps` steps; z the layer centres."""
    spacing = trm.ExponentialSpacing()
    Nz = len(spacing.get_spacing())
    grid = trm.ColumnGrid(spacing, num_columns=Nz)                # Nz replicas of the one column
    model = trm.SoilModel(grid, initializer=trm.SoilInitializer())
    bcs = trm.merge_boundary_conditions(trm.PrescribedSurfaceTemperature("T_ub", 1.0))    # constant surface temperature of 1 degC
    integrator = trm.initialize(model, trm.ForwardEuler(), boundary_conditions=bcs)
    tangents = trm.jvp(integrator, np.eye(Nz), steps)             # replica k: dU_0 = e_k
    return tangents["temperature"], tangents["internal_energy"], grid.z_centers()


def gradient(steps=N_T, checkpoint_every=None):
    """dT_f[second-lowest layer] / dU_0 after `steps` steps, [Nz]: the reference's Enzyme.autodiff(Reverse, ...) call.
    `checkpoint_every` = K: the tape keeps every K-th state and the sweep forms the rest again (the reference's Checkpointing.jl
    scheme passed to run!) -- the same gradient bit for bit."""
    spacing = trm.ExponentialSpacing()
    Nz = len(spacing.get_spacing())
    grid = trm.ColumnGrid(spacing, num_columns=1)
    model = trm.SoilModel(grid, initializer=trm.SoilInitializer())
    bcs = trm.merge_boundary_conditions(trm.PrescribedSurfaceTemperature("T_ub", 1.0))
    integrator = trm.initialize(model, trm.ForwardEuler(), boundary_conditions=bcs)
    seed = np.zeros((Nz, 1))
    seed[1] = 1.0                                                  # the final temperature of the second-lowest layer
    return trm.vjp(integrator, steps, temperature=seed, checkpoint_every=checkpoint_every)[:, 0]


def main():
    J_T, J_U, zs = jacobian()
    dT = J_T[1]        # dT_f[second-lowest layer] / dU_0: the reference's reverse-mode gradient
    g = gradient()
    print("  depth / m   dT_f/dU_0 (second-lowest layer)   the same by trm.vjp   dU_f/dU_0 (same layer)")
    for z, a, r, b in zip(zs[::-1], dT[::-1], g[::-1], J_U[1][::-1]):
        print(f"  {z:9.3f}   {a:31.6e}   {r:19.6e}   {b:22.6e}")
    print(f"Jacobian {J_T.shape}, finite: {bool(np.all(np.isfinite(J_T)))}")


if __name__ == "__main__":
    main()
