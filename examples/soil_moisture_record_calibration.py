#!/usr/bin/env python3
"""Calibrating two hydraulic parameters of a soil column against a soil-moisture probe record: the twin experiment of
examples/soil_moisture_calibration.py with a record in place of the final state.

A van Genuchten column (n = 2, Mualem conductivity) drains for half an hour from a saturation profile that is wetter towards the
surface.  The "true" column has K_sat = 1e-5 m/s and alpha = 1 / m; probes at three depths log its saturation every fifth step, and
the middle probe drops out for two samples (a gap: NaN).  The calibration starts from K_sat = 3e-5 m/s and alpha = 1.6 / m and
descends in the logarithms of the two parameters on

    L = 1/2 sum_k sum_probes (sat_{5 k}[probe] - sat_obs)^2.

The record is attached once and read inside the backward launches (trm.soil_moisture_gradient: one attach, one taped run and one
sweep), so an iterate costs one record-and-sweep however many samples the probes logged -- no twin run for the cotangent, no sweep per
observation time.  The sweep returns the misfit, dL/dU_0, dL/dsat_0 and the gradients with respect to the seven hydraulic parameters.
The calibrated numbers are parameters of the model, and a model with other parameters is another context: every iterate builds its
column anew.

    python examples/soil_moisture_record_calibration.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import terrarium_jl_amd as trm  # noqa: E402

N, DZ, DT, STEPS, EVERY = 10, 0.1, 60.0, 30, 5
PROBES = [2, 5, 8]                       # rows of the host layout
NAMES = ("K_sat", "vg_alpha")
TRUTH = dict(K_sat=1.0e-5, vg_alpha=1.0)
GUESS = dict(K_sat=3.0e-5, vg_alpha=1.6)


def column(params):
    """a thawed 1 m column, 0.6 of saturation at the bottom and 0.85 at the top"""
    grid = trm.ColumnGrid(trm.PrescribedSpacing(dz=[DZ] * N), num_columns=1)
    hydraulics = trm.ConstantSoilHydraulics(swrc=trm.VanGenuchten(alpha=params["vg_alpha"], n=2.0), unsat_hydraulic_cond=trm.UnsatKVanGenuchten(),
                                            sat_hydraulic_cond=params["K_sat"])
    soil = trm.SoilEnergyWaterCarbon(hydrology=trm.SoilHydrology(vertical_flow=trm.RichardsEq(), hydraulic_properties=hydraulics))
    integrator = trm.initialize(trm.SoilModel(grid, soil=soil, initializer=trm.SoilInitializer()), trm.ForwardEuler(dt=DT))
    st = integrator.state
    st.set("temperature", 5.0)
    st.set("saturation_water_ice", np.linspace(0.6, 0.85, N)[:, None])
    st.initialize()
    return integrator


def probe_record():
    """what the probes of the true column log: its saturation at PROBES every EVERY-th step, the middle probe silent for two samples"""
    integrator = column(TRUTH)
    steps, values = list(range(EVERY, STEPS + 1, EVERY)), []
    for _ in steps:
        trm.run(integrator, steps=EVERY)
        values.append(integrator.state.get("saturation_water_ice")[PROBES])
    values = np.stack(values)
    values[2:4, 1] = np.nan
    return trm.SoilMoistureRecord(steps, PROBES, values)


def loss_and_gradient(params, record):
    """(L, {name: dL/d log(parameter)}) from one taped run and one backward sweep"""
    misfit, _, grads = trm.soil_moisture_gradient(column(params), record, steps=STEPS, wrt_params=True)
    return float(np.sum(misfit)), {name: params[name] * float(np.sum(grads[name])) for name in NAMES}


def main(iterations=14):
    record = probe_record()
    params, step = dict(GUESS), 0.3
    L, g = loss_and_gradient(params, record)
    samples = int(np.sum(~np.isnan(record.values)))
    print(f"  {samples} samples at {len(record.steps)} times on {len(PROBES)} probes, one sweep per iterate")
    print("  iteration        loss          K_sat      vg_alpha   step in log")
    print(f"  {0:9d}   {L:12.6e}   {params['K_sat']:10.4e}   {params['vg_alpha']:8.4f}")
    history = [(L, dict(params))]
    for it in range(1, iterations + 1):
        norm = np.sqrt(sum(g[name] ** 2 for name in NAMES))
        if norm == 0.0:
            break
        trial = {name: params[name] * np.exp(-step * g[name] / norm) for name in NAMES}
        L_trial, g_trial = loss_and_gradient(trial, record)
        if L_trial < L:
            params, L, g, step = trial, L_trial, g_trial, 1.5 * step
        else:
            step = 0.5 * step
        print(f"  {it:9d}   {L:12.6e}   {params['K_sat']:10.4e}   {params['vg_alpha']:8.4f}   {step:.3f}")
        history.append((L, dict(params)))
    print(f"  truth                      {TRUTH['K_sat']:10.4e}   {TRUTH['vg_alpha']:8.4f}")
    return history


if __name__ == "__main__":
    main()
