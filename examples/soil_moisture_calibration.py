#!/usr/bin/env python3
"""Calibrating two hydraulic parameters of a soil column against a soil-moisture observation: a twin experiment.

A van Genuchten column (n = 2, Mualem conductivity) drains for half an hour from a saturation profile that is wetter towards the
surface.  The "true" column has K_sat = 1e-5 m/s and alpha = 1 / m; its final saturation is kept as the observation.  The calibration
starts from K_sat = 3e-5 m/s and alpha = 1.6 / m and descends in the logarithms of the two parameters on

    L = 1/2 sum (sat_n - sat_obs)^2,

whose cotangent on the final saturation is wsat = sat_n - sat_obs.  One backward sweep per iterate gives dL/dK_sat and dL/dalpha
together with the state gradients (trm.hydraulic_parameter_gradient: the reference gets them from Enzyme through
Duplicated(integrator, dintegrator)).  The calibrated numbers are parameters of the model, and a model with other parameters is another
context: every iterate builds its column anew, as examples/borehole_calibration_dense.py does.

    python examples/soil_moisture_calibration.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import terrarium_jl_amd as trm  # noqa: E402

N, DZ, DT, STEPS = 10, 0.1, 60.0, 30
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


def observation():
    """the final saturation of the true column, [Nz][1]"""
    integrator = column(TRUTH)
    trm.run(integrator, steps=STEPS)
    return integrator.state.get("saturation_water_ice")


def loss_and_gradient(params, sat_obs):
    """(L, {name: dL/d log(parameter)}) from one taped run and one backward sweep"""
    integrator = column(params)
    # (the cotangent needs the final saturation: a plain run of a twin column first, then the taped run with wsat = sat_n - sat_obs)
    twin = column(params)
    trm.run(twin, steps=STEPS)
    residual = twin.state.get("saturation_water_ice") - sat_obs
    _, grads = trm.hydraulic_parameter_gradient(integrator, STEPS, {"saturation": residual})
    return 0.5 * float(np.sum(residual ** 2)), {name: params[name] * float(np.sum(grads[name])) for name in NAMES}


def main(iterations=12):
    sat_obs = observation()
    params, step = dict(GUESS), 0.3
    L, g = loss_and_gradient(params, sat_obs)
    print("  iteration        loss          K_sat      vg_alpha   step in log")
    print(f"  {0:9d}   {L:12.6e}   {params['K_sat']:10.4e}   {params['vg_alpha']:8.4f}")
    history = [(L, dict(params))]
    for it in range(1, iterations + 1):
        norm = np.sqrt(sum(g[name] ** 2 for name in NAMES))
        if norm == 0.0:
            break
        trial = {name: params[name] * np.exp(-step * g[name] / norm) for name in NAMES}
        L_trial, g_trial = loss_and_gradient(trial, sat_obs)
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
