"""Edge-state workloads for the deriving, deferring and interior instances of the fp64 column step (tests/test_edge_states_host.py,
tests/test_gpu_edge_states.py).  Pure numpy, as workloads.py: describes inputs only; it computes nothing of the model.

The smooth state of workloads.make_workload never reaches the places where a derivation at the entry of a launch can differ from the
closure at the exit of the launch before it: a saturation of exactly 1 (or -0.0) behind the repair, a water table that moves, a column
without a saturated cell, the two kinks of the energy closure.  edge_workload overwrites the initial state per column kind
k = column % 8 and drives half the columns with a strong infiltration flux:

    kind  initial state                                             what it exercises
    0     sat = 1 on every level                                    water table at the surface, overflow from step 1
    1     sat capped at 0.97                                        no saturated cell in the column
    2     sat = 0.6, a saturated pocket (two cells = 1) mid-depth   perched pocket
    3     sat = 0.995 everywhere                                    nearly saturated column
    4     sat = 1 except a top cell of 0.9                          water table one face below the surface
    5     uniformly dry (0.6; van Genuchten 0.12)                   dry column
    6     T = 0.0 on every level                                    U = 0, the upper kink of the energy closure
    7     T linear from -0.5 (bottom) to +0.5 degC (top)            freezing front

Even columns (hence the even kinds) take a top saturation flux of -4.0e-4 m/s, the flux of test_saturation_repair_inside_step; odd
columns none."""
import numpy as np

import workloads as W

KINDS = 8
TOP_FLUX = -4.0e-4      # m/s; negative = downward (infiltration)
NSTEPS = 16
DRY = {"default": 0.6, "vg": 0.12}
ILLEGAL_DRY = 0.12      # kind 5 under BrooksCorey in illegal_dry_workload


def kinds(ncol):
    return np.arange(ncol) % KINDS


def pocket(Nz):
    """levels (0 = bottom) of kind 2's saturated pocket: two cells at mid-depth, never the top cell (Nz = 2: the bottom cell)"""
    return np.arange(max(0, Nz // 2 - 1), min(Nz // 2 + 1, Nz - 1))


def _base(hydraulics, Nz, ncol, config):
    lat, lon = W.columns_from_mask("N72")
    sel = np.linspace(0, lat.size - 1, ncol).astype(int)
    return W.make_workload(config, lat[sel], lon[sel], Nz, hydraulics=hydraulics)


def edge_workload(hydraulics, Nz, ncol, config="richards", dry=None):
    """`ncol` columns spread over the N72 mask, the initial state overwritten per column kind.  config "heat" keeps the thermal kinds
    (6, 7) and the heat-only model's saturation of 1."""
    w = _base(hydraulics, Nz, ncol, config)
    kind = kinds(ncol)
    T = np.array(w["fields"]["temperature"], dtype=np.float64)
    T[:, kind == 6] = 0.0
    T[:, kind == 7] = np.linspace(-0.5, 0.5, Nz)[:, None]
    w["fields"]["temperature"] = T
    w["kind"] = kind
    if config == "heat":
        return w
    sat = np.array(w["fields"]["saturation_water_ice"], dtype=np.float64)
    sat[:, kind == 0] = 1.0
    sat[:, kind == 1] = np.minimum(sat[:, kind == 1], 0.97)
    sat[:, kind == 2] = 0.6
    for k in pocket(Nz):
        sat[k, kind == 2] = 1.0
    sat[:, kind == 3] = 0.995
    sat[:, kind == 4] = 1.0
    sat[Nz - 1, kind == 4] = 0.9
    sat[:, kind == 5] = DRY[hydraulics] if dry is None else dry
    w["fields"]["saturation_water_ice"] = sat
    w["bcs"][("saturation_water_ice", "top")] = ("flux", np.where(np.arange(ncol) % 2 == 0, TOP_FLUX, 0.0))
    return w


def illegal_dry_workload(Nz, ncol):
    """edge_workload under the default BrooksCorey hydraulics with kind 5 at sat = 0.12.  d(psi)/d(sat) is so steep there that the
    explicit step is unstable: on the CPU oracle a dry column (odd: no infiltration) whose soil is not frozen reaches sat = 0 and 1 in
    step 2 and goes non-finite in step 3 -- status 0 after steps 1 and 2, TRM_STATUS_COMPOSITION from step 3 on -- and every other
    column stays valid.  A FROZEN dry column stays valid as well (the ice impedance keeps the conductivity small): the one kind-5
    column of a 13-column workload (T0 = -0.31 degC) is such a column, so ILLEGAL_AT lists which shapes reach the illegal state."""
    return edge_workload("default", Nz, ncol, dry=ILLEGAL_DRY)


# (ncol, Nz) of illegal_dry_workload -> the step at which the oracle's status first becomes non-zero (None: never, see above)
ILLEGAL_AT = {(13, 32): None, (67, 32): 3, (67, 40): 3}

# The shapes (ncol, Nz) of tests/test_gpu_edge_states.py, pinned on the oracle by tests/test_edge_states_host.py.  13 columns: odd, so at
# 32 lanes per column the last wave's second column is a clamped copy, and all eight kinds; 67: nine workgroups, the last partial.
# 2 levels: top and bottom lanes adjacent, no interior cell; 30: idle lanes; 32: a full half-wave; 33: the first 64-lane shape, 31 idle
# lanes; 40; 64: a full wave.
SHAPES = ((13, 2), (13, 30), (67, 32), (13, 33), (67, 40), (13, 64))
SIGNATURE_SHAPES = (("default", 67, 32), ("vg", 67, 40))
KINK_SHAPE = (13, 32)
STATUS_SHAPES = tuple(ILLEGAL_AT)
STAGED_SHAPES = ((13, 30), (67, 32), (67, 40))

# the calls every run of these modules makes: (steps, finalize), 16 steps in all
CALLS = ((1, False), (7, False), (1, False), (7, True))


def with_signature(w, extra):
    """The workload with the boundary conditions of one entry of test_gpu_interior_steps.SIGNATURES.  The edge workload's own top
    saturation flux stands only where the entry sets one (signature 34); the other signatures have none."""
    w = dict(w, bcs=dict(w["bcs"]))
    flux = w["bcs"].pop(("saturation_water_ice", "top"))
    if extra == "closed":
        w["bcs"].clear()
        return w
    for key, (kind, value) in extra.items():
        w["bcs"][key] = flux if key == ("saturation_water_ice", "top") else (kind, np.full(w["Nh"], value))
    return w


# ---- the lower kink of the energy closure: U == -Lth exactly on a cell --------------------------------------------------------------
def latent_threshold(params, sat):
    """Lth = L * sat * por as the closure forms it in fp64 (energy_to_temperature_all: L = rho_w * Lsl, por = porosity(p)), from the
    oracle's parameter struct"""
    L = params.rho_w * params.Lsl
    org = params.rho_soc / ((1.0 - params.por_organic) * params.rho_org)
    por = (1.0 - org) * params.por_mineral + org * params.por_organic
    return L * np.asarray(sat, dtype=np.float64) * por


def put_energy_on_lower_kink(w, sides, columns):
    """After initialize, on `columns`: internal_energy = -(L * sat * por) of the cell's own saturation, uploaded to every side (oracles
    and device contexts alike), then closure() on each.  Returns the uploaded energy."""
    import oracle
    params = oracle.default_params(**w["params"])
    U = None
    for s in sides:
        u = np.array(s.get("internal_energy"), dtype=np.float64)
        sat = np.array(s.get("saturation_water_ice"), dtype=np.float64)
        u[:, columns] = -latent_threshold(params, sat[:, columns])
        if U is None:
            U = u
        assert np.array_equal(u, U), "the sides do not agree on the initialised state"
        s.set("internal_energy", u.astype(s.get("internal_energy").dtype))
        s.closure()
    return U


# ---- what a run of the recipe has to reach (tests/test_edge_states_host.py) ---------------------------------------------------------
FEATURES = ("oversaturated_below_top", "oversaturated_top", "surface_excess", "partly_frozen", "water_table_at_surface",
            "water_table_below_surface")


def step_by_hand(o, dt, finalize, seen=None):
    """timestep_euler in its parts, looking at the saturation between explicit_step! and closure!.  `seen`: {feature: count}, updated."""
    o.update_state(True)
    o.explicit_step(dt)
    if seen is not None:
        sat = o.get("saturation_water_ice")
        seen["oversaturated_below_top"] += int(np.count_nonzero((sat[:-1] > 1).any(axis=0)))
        seen["oversaturated_top"] += int(np.count_nonzero(sat[-1] > 1))
    o.closure()
    o.tick(dt)
    if finalize:
        o.compute_auxiliary()
    if seen is not None:
        surface = o.grid()["zF"][-1]
        liq, wt = o.get("liquid_water_fraction"), o.get("water_table")
        seen["surface_excess"] += int(np.count_nonzero(o.get("surface_excess_water") > 0))
        seen["partly_frozen"] += int(np.count_nonzero((liq > 0) & (liq < 1)))
        seen["water_table_at_surface"] += int(np.count_nonzero(wt == surface))
        seen["water_table_below_surface"] += int(np.count_nonzero(wt < surface))
