#!/usr/bin/env python3
"""Calibrating soil thermal properties against a borehole temperature record: the inverse problem the sensitivities of
thermal_parameter_history_sensitivity.py point at.  The column of surface_temperature_history_sensitivity.py,

    PrescribedSurfaceTemperature(:T_ub, FieldTimeSeries(times, values)), ForwardEuler, run! for N_t = 240 steps

is run once with a known conductivity and heat capacity of the mineral constituent; its temperatures at four sensor depths, every
twelve steps, are the synthetic record.  Starting from a wrong guess of both parameters, every iteration runs the column forward once
with the record's samples registered where the run passes them, and backward once (trm.misfit_gradient): the misfit
L = sum 1/2 (T - T_obs)^2 and dL/d(k_mineral), dL/d(c_mineral) from one sweep, whatever the number of observation times.  A few steps
of steepest descent in the logarithms of the two parameters, with a step that grows when the misfit falls and halves when it does not,
bring the misfit down; the example prints it per iteration.

The initial internal energy is the same known profile in every run: the gradient is with respect to the parameters at a fixed U_0
(dL/dU_0 comes from the same sweep and would carry an uncertain initial state as well).

    python examples/borehole_calibration.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from surface_temperature_history_sensitivity import record as surface_record  # noqa: E402
import terrarium_jl_amd as trm  # noqa: E402

N_T = 240
EVERY = 12
SENSORS = (1, 3, 5, 8)                    # levels counted down from the surface
TRUTH = dict(k_mineral=3.8, c_mineral=2.0e6)
GUESS = dict(k_mineral=2.0, c_mineral=3.0e6)
NAMES = tuple(TRUTH)


def column(params, U0=None):
    grid = trm.ColumnGrid(trm.ExponentialSpacing(), num_columns=1)
    properties = trm.SoilThermalProperties(trm.SoilThermalConductivities(mineral=params["k_mineral"]),
                                           trm.SoilHeatCapacities(mineral=params["c_mineral"]))
    soil = trm.SoilEnergyWaterCarbon(energy=trm.SoilEnergyBalance(properties))
    model = trm.SoilModel(grid, soil=soil, initializer=trm.SoilInitializer())
    times, values = surface_record(N_T)
    bcs = trm.merge_boundary_conditions(trm.PrescribedSurfaceTemperature("T_ub", trm.FieldTimeSeries(times, values[:, None])))
    integrator = trm.initialize(model, trm.ForwardEuler(), boundary_conditions=bcs)
    if U0 is not None:                    # the known initial energy profile, under this run's parameters
        integrator.state.set("internal_energy", U0)
        integrator.state.closure()
    return integrator, grid


def sensor_levels(Nz):
    """rows of the host layout (row 0 = bottom layer), increasing"""
    return sorted(Nz - 1 - s for s in SENSORS)


def synthetic_record():
    """(record, U_0): the temperatures the true column shows at the sensors every EVERY steps, and its initial internal energy"""
    integrator, grid = column(TRUTH)
    U0 = integrator.state.get("internal_energy")
    levels = sensor_levels(grid.Nz)
    steps, values = [], []
    for s in range(EVERY, N_T + 1, EVERY):
        trm.run(integrator, steps=EVERY)
        steps.append(s)
        values.append(integrator.state.get("temperature")[levels])
    return trm.TemperatureRecord(steps, levels, np.stack(values)), U0


def misfit_and_gradient(params, record, U0, checkpoint_every=16):
    """(L, {name: dL/d log(parameter)}) from one forward run and one backward sweep"""
    integrator, _ = column(params, U0)
    L, _, g = trm.misfit_gradient(integrator, record, steps=N_T, checkpoint_every=checkpoint_every, wrt_params=True)
    return float(np.sum(L)), {name: params[name] * float(np.sum(g[name])) for name in NAMES}


def main(iterations=12):
    record, U0 = synthetic_record()
    params, step = dict(GUESS), 0.2
    L, g = misfit_and_gradient(params, record, U0)
    print("  iteration   misfit / K^2     k_mineral      c_mineral   step in log")
    print(f"  {0:9d}   {L:12.6e}   {params['k_mineral']:9.4f}   {params['c_mineral']:12.5e}")
    history = [(L, dict(params))]
    for it in range(1, iterations + 1):
        norm = np.sqrt(sum(g[name] ** 2 for name in NAMES))
        if norm == 0.0:
            break
        trial = {name: params[name] * np.exp(-step * g[name] / norm) for name in NAMES}
        L_trial, g_trial = misfit_and_gradient(trial, record, U0)
        if L_trial < L:
            params, L, g, step = trial, L_trial, g_trial, 1.5 * step
        else:
            step = 0.5 * step
        print(f"  {it:9d}   {L:12.6e}   {params['k_mineral']:9.4f}   {params['c_mineral']:12.5e}   {step:.3f}")
        history.append((L, dict(params)))
    print(f"  truth                      {TRUTH['k_mineral']:9.4f}   {TRUTH['c_mineral']:12.5e}")
    return history


if __name__ == "__main__":
    main()
