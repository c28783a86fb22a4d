#!/usr/bin/env python3
"""The calibration of borehole_calibration_dense.py -- 240 samples on four sensor depths, two thermal parameters -- by
Levenberg-Marquardt instead of gradient descent.

A gradient alone allows a descent with a guessed step.  The problem is a small least-squares problem with a zero residual at the truth,
the textbook case for Gauss-Newton: with the sensitivities s_q = dT/d(parameter q) at the samples, the step solves
(A + lambda diag A) delta = -b, A = sum s s^T, b = sum s r.  A tangent record (DeviceState.attach_tangent_record,
trm_tangent_record_attach) gives T and s_q at all 240 samples from ONE tangent run per parameter: positions and levels are attached
once, the samples are stored inside the tangent launches, no sample ends a launch (trm.record_jvp, trm.record_normal_equations).

The synthetic record itself comes from one such run with zero seeds -- the 240 trm.run(steps=1) calls and field downloads of the
sibling example in one call.  The iteration works in the logarithms of the two parameters; two tangent runs per iterate; the damping is
multiplied by 4 on a rejected trial and divided by 3 on an accepted one.

    python examples/borehole_calibration_gauss_newton.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import borehole_calibration as base  # noqa: E402
import terrarium_jl_amd as trm  # noqa: E402

N_T = base.N_T
TRUTH, GUESS, NAMES = base.TRUTH, base.GUESS, base.NAMES
UP, DOWN = 4.0, 3.0


def synthetic_record():
    """(record, U_0): what the true column shows at the sensors after every step, from one tangent run with zero seeds"""
    integrator, grid = base.column(TRUTH)
    U0 = integrator.state.get("internal_energy")
    levels = base.sensor_levels(grid.Nz)
    positions = list(range(1, N_T + 1))
    T, _ = trm.record_jvp(integrator, positions, levels)
    return trm.TemperatureRecord(positions, levels, T), U0


def normal_equations(params, record, U0):
    """(L, b, A) in the logarithms of the parameters: one tangent run per parameter on this parameter set's column"""
    integrator, _ = base.column(params, U0)
    L, b, A = trm.record_normal_equations(integrator, record, NAMES)
    scale = np.array([params[name] for name in NAMES])          # d/d log(p) = p d/dp
    return float(np.sum(L)), scale * np.sum(b, axis=1), scale[:, None] * scale[None, :] * np.sum(A, axis=2)


def main(iterations=8):
    record, U0 = synthetic_record()
    params, damping = dict(GUESS), 1e-2
    L, b, A = normal_equations(params, record, U0)
    print(f"  {len(record.steps)} samples on {record.levels.size} levels, {len(NAMES)} tangent runs per iterate")
    print("  iteration   misfit / K^2     k_mineral      c_mineral   damping")
    print(f"  {0:9d}   {L:12.6e}   {params['k_mineral']:9.4f}   {params['c_mineral']:12.5e}")
    history = [(L, dict(params), True)]
    for it in range(1, iterations + 1):
        if not np.any(b):
            break
        delta = np.linalg.solve(A + damping * np.diag(np.diag(A)), -b)
        trial = {name: params[name] * float(np.exp(d)) for name, d in zip(NAMES, delta)}
        L_trial, b_trial, A_trial = normal_equations(trial, record, U0)
        accepted = L_trial < L
        if accepted:
            params, L, b, A, damping = trial, L_trial, b_trial, A_trial, damping / DOWN
        else:
            damping = damping * UP
        print(f"  {it:9d}   {L:12.6e}   {params['k_mineral']:9.4f}   {params['c_mineral']:12.5e}   {damping:.2e}" + ("" if accepted else "   (rejected)"))
        history.append((L, dict(params), accepted))
    print(f"  truth                      {TRUTH['k_mineral']:9.4f}   {TRUTH['c_mineral']:12.5e}")
    return history


if __name__ == "__main__":
    main()
