#!/usr/bin/env python3
"""The calibration of borehole_calibration.py against a logger that samples at EVERY step: 240 samples on four sensor depths, on a
checkpointed tape of 240 / 16 = 15 slots.

Registered position by position (trm.misfit_gradient) such a record makes every step a launch boundary and a checkpoint slot -- the
checkpointed tape degenerates into a per-step tape of 240 slots.  Attached (DeviceState.attach_record, trm_adjoint_observe_record_device)
the record is read inside the backward launches: no sample ends a launch, none takes a slot.

The record goes to the device ONCE, outside the descent loop, as two torch tensors (the observed temperatures; no weights).  The two
calibrated numbers are parameters of the model, and a model with other parameters is another context; every iteration's context
attaches the same device arrays by pointer -- no copy, no per-sample call -- records the 240 steps in one call and sweeps once.  (A
loop that varies the initial state or a boundary value on one context attaches once and never again: the record survives sweeps.)

    python examples/borehole_calibration_dense.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import borehole_calibration as base  # noqa: E402
import terrarium_jl_amd as trm  # noqa: E402

N_T, K = base.N_T, 16
TRUTH, GUESS, NAMES = base.TRUTH, base.GUESS, base.NAMES


def synthetic_record():
    """(positions, levels, values[N_T][4][1], U_0): what the true column shows at the sensors after every step"""
    integrator, grid = base.column(TRUTH)
    U0 = integrator.state.get("internal_energy")
    levels = base.sensor_levels(grid.Nz)
    values = []
    for _ in range(N_T):
        trm.run(integrator, steps=1)
        values.append(integrator.state.get("temperature")[levels])
    return list(range(1, N_T + 1)), levels, np.stack(values), U0


def misfit_and_gradient(params, positions, levels, d_values, U0):
    """(L, {name: dL/d log(parameter)}, slots used) from one record call and one sweep with the device-resident record attached"""
    integrator, _ = base.column(params, U0)
    st = integrator.state
    st.open_adjoint(-(-N_T // K), K)
    try:
        from terrarium_jl_amd.derivatives import _derivative_series
        with _derivative_series(integrator, params=True):
            st.attach_record(positions, levels, d_values)
            st.step_record(integrator.timestepper.dt, N_T)
            used = st.adjoint_checkpoints()[1]
            st.open_param_gradient()
            st.adjoint_backward()
            L = float(np.sum(st.record_misfit()))
            g = {name: params[name] * float(np.sum(st.param_gradient(name))) for name in NAMES}
    finally:
        st.close_adjoint()
    return L, g, used


def main(iterations=12):
    import torch
    positions, levels, values, U0 = synthetic_record()
    d_values = torch.as_tensor(values, device="cuda")          # the record: uploaded once, outside the loop
    torch.cuda.synchronize()
    params, step = dict(GUESS), 0.2
    L, g, used = misfit_and_gradient(params, positions, levels, d_values, U0)
    print(f"  {len(positions)} samples on {len(levels)} levels, {used} checkpoint slots of {K} steps")
    print("  iteration   misfit / K^2     k_mineral      c_mineral   step in log")
    print(f"  {0:9d}   {L:12.6e}   {params['k_mineral']:9.4f}   {params['c_mineral']:12.5e}")
    history = [(L, dict(params), used)]
    for it in range(1, iterations + 1):
        norm = np.sqrt(sum(g[name] ** 2 for name in NAMES))
        if norm == 0.0:
            break
        trial = {name: params[name] * np.exp(-step * g[name] / norm) for name in NAMES}
        L_trial, g_trial, used = misfit_and_gradient(trial, positions, levels, d_values, U0)
        if L_trial < L:
            params, L, g, step = trial, L_trial, g_trial, 1.5 * step
        else:
            step = 0.5 * step
        print(f"  {it:9d}   {L:12.6e}   {params['k_mineral']:9.4f}   {params['c_mineral']:12.5e}   {step:.3f}")
        history.append((L, dict(params), used))
    print(f"  truth                      {TRUTH['k_mineral']:9.4f}   {TRUTH['c_mineral']:12.5e}")
    return history


if __name__ == "__main__":
    main()
