/* terrarium_hip.h -- C ABI of libterrarium_hip.so
 *
 * MI355X-native (gfx950, hand-written HIP) implementation of ONE hot path of
 * TUM-PIK-ESM/Terrarium.jl: the explicit time step of SoilModel /
 * LandModel(vegetation = nothing) over laterally independent soil columns --
 * heat conduction with freeze/thaw, Richards water transport, bare-ground
 * surface energy balance, forward-Euler / Heun update and the closures.
 *
 * The reference is pure Julia and has NO FFI: its extension surface is multiple
 * dispatch on (state, model) (src/abstract_model.jl:52-95,175-215) and the
 * time-stepper hook timestep!(integrator, ::AbstractTimeStepper, dt)
 * (src/timesteppers/abstract_timestepper.jl:39).  Every entry point below names
 * the reference method it stands in for; INTEGRATION.md shows the ~200-line
 * Julia shim (`ccall`) a maintainer would add on the reference side.
 *
 * Conventions
 *   - every function returns 0 on success, a TRM_E* code otherwise; the message
 *     is available from trm_last_error(ctx).  Nothing throws across the ABI.
 *   - the context owns all device memory; host pointers are borrowed for the
 *     duration of a call.  Calls are synchronous on return EXCEPT trm_step /
 *     trm_step_heun / the compute_* family when TRM_OPT_ASYNC is set.
 *   - one host thread drives a context; contexts are independent; no globals
 *     (reference rule AGENTS.md:44).
 *   - host arrays are [rows][num_columns], x (column) fastest, NO halos, row 0 =
 *     BOTTOM layer, row Nz-1 = surface layer: exactly `interior(field)` of the
 *     reference's (Nh, 1, Nz) Fields (src/grids/column_grid.jl:27-32).  Element
 *     type is double for TRM_F64 contexts and float for TRM_F32.
 *   - there is no CPU fallback: every entry point that computes needs a GPU.
 */
#ifndef TERRARIUM_HIP_H
#define TERRARIUM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRM_ABI_VERSION 20

typedef struct trm_ctx trm_ctx;

/* ---- status codes ------------------------------------------------------- */
enum { TRM_OK = 0, TRM_EINVAL = 1, TRM_EHIP = 2, TRM_ENOMEM = 3, TRM_EUNSUPPORTED = 4,
       TRM_ESTALE = 5, /* the field asked for is not materialised at this point (see trm_step) */
       TRM_ECOMM = 6   /* RCCL could not be loaded / a collective failed */ };

/* ---- number format NF (every reference struct is parameterised by it) ---- */
enum { TRM_F64 = 0, TRM_F32 = 1 };

/* ---- configuration enums -------------------------------------------------- */
enum { TRM_FLOW_NOFLOW = 0, TRM_FLOW_RICHARDS = 1 };        /* soil_hydrology.jl:14, soil_hydrology_rre.jl:18 */
enum { TRM_SWRC_BROOKS_COREY = 0, TRM_SWRC_VAN_GENUCHTEN = 1 }; /* FreezeCurves.jl SWRCs                     */
enum { TRM_UNSATK_LINEAR = 0, TRM_UNSATK_VAN_GENUCHTEN = 1 };   /* soil_hydraulic_properties.jl:166,196     */
/* under NoFlow the reference never fills the z halos of the
 * auxiliary saturation field (they stay 0); MIRROR copies the edge cell instead. */
enum { TRM_HALO_REFERENCE_ZERO = 0, TRM_HALO_MIRROR = 1 };

/* Boundary conditions (Oceananigans Value / Flux / Gradient / default NoFlux). */
enum { TRM_BC_NOFLUX = 0, TRM_BC_VALUE = 1, TRM_BC_FLUX = 2, TRM_BC_GRADIENT = 3 };
enum { TRM_BOTTOM = 0, TRM_TOP = 1 };
enum {
    TRM_BCV_INTERNAL_ENERGY = 0,
    TRM_BCV_SATURATION_WATER_ICE = 1,
    TRM_BCV_TEMPERATURE = 2,
    TRM_BCV_LIQUID_WATER_FRACTION = 3,
    TRM_BCV_PRESSURE_HEAD = 4,
    TRM_BCV_COUNT = 5
};

/* ---- state variables ---------------------------------- */
enum {
    /* 3-D, Nz rows */
    TRM_FIELD_INTERNAL_ENERGY = 0,          /* prognostic, J/m^3   soil_energy.jl:47            */
    TRM_FIELD_SATURATION_WATER_ICE = 1,     /* prognostic (Richards) / auxiliary (NoFlow)        */
    TRM_FIELD_TEMPERATURE = 2,              /* closure, degC      soil_energy_closures.jl:23   */
    TRM_FIELD_LIQUID_WATER_FRACTION = 3,    /* closure             soil_energy_closures.jl:24   */
    TRM_FIELD_PRESSURE_HEAD = 4,            /* closure, m          soil_hydraulic_closures.jl:15 */
    TRM_FIELD_HYDRAULIC_CONDUCTIVITY = 5,   /* Face field, Nz+1 rows  soil_hydrology.jl:81      */
    TRM_FIELD_TEND_INTERNAL_ENERGY = 6,
    TRM_FIELD_TEND_SATURATION_WATER_ICE = 7,
    /* 2-D, 1 row */
    TRM_FIELD_SURFACE_EXCESS_WATER = 8,     /* prognostic, m       soil_hydrology_rre.jl:22     */
    TRM_FIELD_TEND_SURFACE_EXCESS_WATER = 9,
    TRM_FIELD_WATER_TABLE = 10,             /* auxiliary, m        soil_hydrology.jl:80         */
    TRM_FIELD_SKIN_TEMPERATURE = 11,        /* skin_temperature.jl:85                           */
    TRM_FIELD_GROUND_HEAT_FLUX = 12,        /* skin_temperature.jl:86; top Flux BC of U in LandModel */
    TRM_FIELD_SURFACE_SHORTWAVE_UP = 13,    /* radiative_fluxes.jl:104-108                      */
    TRM_FIELD_SURFACE_LONGWAVE_UP = 14,
    TRM_FIELD_SURFACE_NET_RADIATION = 15,
    TRM_FIELD_SENSIBLE_HEAT_FLUX = 16,      /* turbulent_fluxes.jl:54-57                        */
    TRM_FIELD_LATENT_HEAT_FLUX = 17,
    TRM_FIELD_EVAPORATION_GROUND = 18,      /* bare_ground_evaporation.jl:27                    */
    TRM_FIELD_INFILTRATION = 19,            /* direct_surface_runoff.jl:65-68; -I = top Flux BC of sat */
    TRM_FIELD_SURFACE_RUNOFF = 20,
    /* PrescribedAtmosphere inputs (prescribed_atmosphere.jl:89-99) */
    TRM_FIELD_AIR_TEMPERATURE = 21,
    TRM_FIELD_AIR_PRESSURE = 22,
    TRM_FIELD_WINDSPEED = 23,
    TRM_FIELD_SPECIFIC_HUMIDITY = 24,
    TRM_FIELD_RAINFALL = 25,
    TRM_FIELD_SURFACE_SHORTWAVE_DOWN = 26,
    TRM_FIELD_SURFACE_LONGWAVE_DOWN = 27,
    /* 3-D, Nz rows: the user `vwc_forcing` (soil_hydrology.jl:37-38, forcings.jl:13-15) evaluated per cell by the
     * caller [1/s].  Uploading it switches the Richards tendency from the scalar trm_params.vwc_forcing to this
     * field; TRM_OPT_VWC_FORCING_FIELD = 0 switches back. */
    TRM_FIELD_VWC_FORCING = 28,
    /* 2-D inputs of PrescribedAlbedo (src/processes/surface_energy/albedo.jl:8-14): read by the surface energy balance
     * per column instead of trm_params.albedo / .emissivity when trm_params.prescribed_albedo = 1 */
    TRM_FIELD_ALBEDO = 29,
    TRM_FIELD_EMISSIVITY = 30,
    /* ---- vegetation (VegetationCarbon, src/processes/vegetation/; enabled by trm_set_vegetation) -- all 2-D ---- */
    TRM_FIELD_CARBON_VEGETATION = 31,        /* prognostic, kgC/m^2   carbon_dynamics.jl:55                          */
    TRM_FIELD_VEGETATION_AREA_FRACTION = 32, /* prognostic           vegetation_dynamics.jl:27                      */
    TRM_FIELD_TEND_CARBON_VEGETATION = 33,
    TRM_FIELD_TEND_VEGETATION_AREA_FRACTION = 34,
    TRM_FIELD_BALANCED_LEAF_AREA_INDEX = 35, /* carbon_dynamics.jl:56                                                */
    TRM_FIELD_PHENOLOGY_FACTOR = 36,         /* phenology.jl:24-25                                                   */
    TRM_FIELD_LEAF_AREA_INDEX = 37,
    TRM_FIELD_CANOPY_WATER_CONDUCTANCE = 38, /* m/s                  stomatal_conductance.jl:29-30                  */
    TRM_FIELD_LEAF_TO_AIR_CO2_RATIO = 39,
    TRM_FIELD_NET_ASSIMILATION = 40,         /* gC/m^2/s             photosynthesis.jl:73-75                        */
    TRM_FIELD_LEAF_RESPIRATION = 41,
    TRM_FIELD_GROSS_PRIMARY_PRODUCTION = 42, /* kgC/m^2/s                                                            */
    TRM_FIELD_AUTOTROPHIC_RESPIRATION = 43,  /* autotrophic_respiration.jl:33-34                                     */
    TRM_FIELD_NET_PRIMARY_PRODUCTION = 44,
    TRM_FIELD_CO2 = 45,                      /* input, ppm (default 380)   prescribed_atmosphere.jl:10-14           */
    TRM_FIELD_SOIL_MOISTURE_LIMITING_FACTOR = 46, /* input (default 1) without soil; the root-weighted integral of     */
                                             /* plant_available_water with it   plant_available_water.jl:21-36       */
    TRM_FIELD_DAILY_LEAF_RESPIRATION = 47,   /* input, gC/m^2/s      autotrophic_respiration.jl:36                  */
    TRM_FIELD_VEGETATION_GROUND_TEMPERATURE = 48, /* `ground_temperature` input of the standalone VegetationModel      */
                                             /* (default 10 degC, autotrophic_respiration.jl:38); with soil the top cell is read */
    /* 3-D, Nz rows (allocated by trm_set_vegetation) */
    TRM_FIELD_PLANT_AVAILABLE_WATER = 49,    /* plant_available_water.jl:22                                          */
    TRM_FIELD_ROOT_FRACTION = 50,            /* static, normalised   root_distribution.jl:45-63                     */
    /* LandModel with vegetation: PALADYNCanopyInterception / PALADYNCanopyEvapotranspiration, one value per column */
    TRM_FIELD_CANOPY_WATER = 51,             /* prognostic, m        canopy_interception.jl:55                      */
    TRM_FIELD_TEND_CANOPY_WATER = 52,
    TRM_FIELD_CANOPY_WATER_INTERCEPTION = 53, /* m/s                 canopy_interception.jl:56-59                   */
    TRM_FIELD_CANOPY_WATER_REMOVAL = 54,
    TRM_FIELD_SATURATION_CANOPY_WATER = 55,
    TRM_FIELD_RAINFALL_GROUND = 56,          /* rain reaching the ground, m/s: what the runoff scheme routes        */
    TRM_FIELD_EVAPORATION_CANOPY = 57,       /* m/s                  canopy_evapotranspiration.jl:90-92             */
    TRM_FIELD_TRANSPIRATION = 58,
    TRM_FIELD_STEM_AREA_INDEX = 59,          /* input `SAI` (default 0)   canopy_interception.jl:64                 */
    TRM_FIELD_COUNT = 60
};

/* ---- diagnostics ---------------------------------------------------------- */
enum { TRM_REDUCE_SUM = 0, TRM_REDUCE_MIN = 1, TRM_REDUCE_MAX = 2, TRM_REDUCE_HASNAN = 3, TRM_REDUCE_VOLUME_INTEGRAL_Z = 4 };
/* trm_status flag bits: replace the reference's CPU-side @assert / DEBUG NaN scans
 * (soil_volume.jl:26-28,85; diagnostics/debugging.jl:19-25). */
enum { TRM_STATUS_NAN = 1u, TRM_STATUS_COMPOSITION_OUT_OF_RANGE = 2u,
       TRM_STATUS_HANDOFF_TIMEOUT = 4u /* TRM_OPT_SURFACE_IN_LAUNCH: a column wave gave up waiting for its surface fluxes; its columns are NaN */ };

/* ---- options (trm_set_option) --------------------------------------------- */
enum {
    TRM_OPT_ASYNC = 0,          /* 1: trm_step & co. return after enqueueing on the context stream          */
    TRM_OPT_STEP_KERNEL = 1,    /* TRM_KERNEL_*: which implementation trm_step uses                          */
    TRM_OPT_WRITE_KF_EVERY_STEP = 2,/* 1 (default): hydraulic_conductivity is stored by every step launch;   */
                                    /* 0: only by launches that finalize (it is never an input of a step)   */
    TRM_OPT_VWC_FORCING_FIELD = 3,  /* 1 after TRM_FIELD_VWC_FORCING was uploaded: per-cell vwc_forcing; 0: scalar */
    TRM_OPT_PACKED_F32 = 4,         /* 1 (default): fp32 contexts with the reference-default hydraulics step two       */
                                    /* columns per lane with packed fp32 instructions (bit-identical results); 0: off */
    TRM_OPT_DERIVE_CLOSURE_FIELDS = 5, /* When the stored temperature / liquid_water_fraction are known to be the energy     */
                                    /* closure of the stored internal_energy / saturation (the library wrote them), a fused   */
                                    /* Euler step can re-derive them in registers instead of reading them: 2 of 5 field reads */
                                    /* less, bit-identical results.  0: never; 1: whenever legal; 2 (default): for fp64 states  */
                                    /* beyond the 256 MiB Infinity Cache or of >= 24 576 columns, and the liquid fraction alone */
                                    /* for fp32 states beyond the cache on the packed kernel: where it was measured to win      */
                                    /* (DESIGN 4.1, 4.3); 3: the liquid fraction alone (one read less); 4: the liquid fraction   */
                                    /* and, on the packed fp32 step with Richards, the pressure head from the stored saturation */
                                    /* and water table (two reads less; elsewhere as 3)                                          */
                                    /* 5: as 1 (until round 5 the fp64 column program had an instance that derived the pressure */
                                    /* head as well: measured slower twice, removed; EXPERIMENTS.md).  On the fp64 column       */
                                    /* program 3 and 4 select 1 as well: its "liquid fraction alone" instance went the same way */
    TRM_OPT_STEPS_PER_LAUNCH = 6,   /* trm_step keeps every column in registers for up to m steps per launch and writes the */
                                    /* fields once per launch (temporal blocking of run!'s loop, model_integrator.jl:72-88;  */
                                    /* bit-identical to m = 1).  0 (default): the library chooses -- 50 wherever the program  */
                                    /* is legal (branch-free boundary kinds, constants or device-resident series the program  */
                                    /* interpolates itself, no coupled vegetation; fp32 contexts included); 1: one launch per */
                                    /* step (state streams through memory every step: what bench.py's headline measures);     */
                                    /* m > 1: explicit                                                                          */
    TRM_OPT_PIPELINE_PARTS = 7      /* bare-ground LandModel, one launch per step and half: the columns are dealt to two      */
                                    /* halves and every launch covers the soil columns of one half AND the 0-D surface         */
                                    /* processes (land_model.jl:79-88) of the other, so that the latency-bound surface chain  */
                                    /* runs under the column program (columns are independent; bit-identical results).        */
                                    /* Applies to calls of >= 2 steps with constant inputs and the branch-free boundary kinds. */
                                    /* 0: off; 1: whenever legal; 2 (default): the library's rule -- currently never: measured  */
                                    /* within +-2 % at 812 500 columns and +10 % at N145 (every launch carries ~4 us of fixed    */
                                    /* cost)                                                                         */
    ,TRM_OPT_SINGLE_STEP_PROGRAM = 8 /* trm_step(ctx, dt, 1, .) of a bare-ground LandModel whose inputs change every step (a        */
                                    /* coupled atmosphere: speedy_dry_land.jl:45-68): 1 runs the resident column program with the   */
                                    /* surface processes inline for the single step -- ONE launch instead of the k_surface +        */
                                    /* k_column pair; 0: the launch pair; 2 (default): the library's rule (small shards, where the  */
                                    /* step is bound by launch latency: DESIGN 4.9)                                                  */
    ,TRM_OPT_BC_SIGNATURE = 9       /* 1 (default): a per-step ForwardEuler launch whose boundary kinds match one of the signatures    */
                                    /* compiled into the library (none; prescribed surface temperature; that + a bottom heat flux;    */
                                    /* that + an infiltration flux; the LandModel wiring) takes the program with the kinds as          */
                                    /* compile-time constants (-3 ... -10 %,                                                            */
                                    /* DESIGN 4.3); 0: always the program that reads the kinds at run time (same results; A/B, tests)  */
    ,TRM_OPT_ZERO_GRADIENT_FAST = 10 /* 1 (default): a Gradient condition on temperature or pressure head at the BOTTOM whose values   */
                                    /* trm_set_bc received as +0 everywhere -- the reference's FreeDrainage(), soil_model_bcs.jl:40 --  */
                                    /* forms the same halo, bit for bit, as no condition at all, and the context keeps the branch-free */
                                    /* programs (derivation, resident multi-step program, ...) instead of the generic-boundary kernels; */
                                    /* handing the value buffer out (trm_bc_device_ptr) or attaching a series ends it.  0: off (A/B)    */
    ,TRM_OPT_SURFACE_IN_LAUNCH = 11 /* bare-ground LandModel stepped one launch per step (fp64, Richards, the LandModel's boundary wiring,  */
                                    /* one level per lane): 1 = the 0-D surface processes (land_model.jl:79-88) run in the FIRST workgroups */
                                    /* of the step launch, one lane per column, and hand ground heat flux, infiltration and the skin        */
                                    /* temperature to the column workgroups of the same launch through tagged 8-byte words -- ONE launch     */
                                    /* per step instead of the k_surface + k_column pair, same operations per column (bit-identical); the   */
                                    /* inputs may change every step (nothing is evaluated ahead).  A column wave whose bounded wait for     */
                                    /* its words ends unanswered raises TRM_STATUS_HANDOFF_TIMEOUT instead of hanging.  0: the launch pair;  */
                                    /* 2 (default): the library's rule                                                          */
    ,TRM_OPT_DEFER_CLOSURE_STORES = 12 /* 1 (default): a per-step ForwardEuler launch that derives temperature / liquid fraction in        */
                                    /* registers (TRM_OPT_DERIVE_CLOSURE_FIELDS) does not store them either -- the next step derives them    */
                                    /* again -- and the library forms them from the stored (internal_energy, saturation) with one small     */
                                    /* launch in front of the first call that reads or writes field memory (see trm_step): same values, bit  */
                                    /* for bit.  0: stored by every step (a caller that reads one of them after EVERY step: DESIGN 4.3).     */
                                    /* Environment: TRM_DEFER_CLOSURE_STORES = 0 / 1 sets the default of new contexts (A/B)                  */
    ,TRM_OPT_INTERIOR_STEPS = 13    /* 1: inside ONE trm_step / trm_step_timed call of n > 1 steps, the per-step fp64 heat + Richards  */
                                    /* launches (no LandModel, a compiled-in boundary signature, TRM_OPT_DEFER_CLOSURE_STORES in effect) but  */
                                    /* the last store internal_energy, saturation, surface_excess_water and the water table alone; the launch   */
                                    /* behind one derives the pressure head at entry from (saturation, water table) instead of reading it.      */
                                    /* pressure_head, hydraulic_conductivity and the status word are stale only between launches of one call:    */
                                    /* after every call all arrays, the status and the clock are what option 0 leaves, bit for bit.  0: every    */
                                    /* launch stores everything (A/B, tests); 2 (default): the library's rule -- as 1 for states within the      */
                                    /* Infinity Cache (256 MiB), as 0 beyond.  Environment: TRM_INTERIOR_STEPS = 0 / 1 / 2 sets the default      */
    ,TRM_OPT_DERIVATIVE_SERIES = 14 /* 1: trm_step_tangent, trm_step_record and trm_adjoint_backward accept boundary time series (whole       */
                                    /* records, trm_set_bc_series) of kind Value on temperature and Flux on internal energy, bottom or top,      */
                                    /* on the branch-free boundary kinds: the kernels evaluate them in front of every step, seeds and           */
                                    /* gradients of such a pair have the series' shape (trm_tangent_bc_series_upload,                            */
                                    /* trm_adjoint_bc_series_download).  0 (default): a context with a series attached is refused with          */
                                    /* TRM_EUNSUPPORTED by those three calls                                                                      */
    ,TRM_OPT_DERIVATIVE_SERIES_PARAMS = 15 /* 1, together with TRM_OPT_DERIVATIVE_SERIES = 1: a context that carries such boundary series also   */
                                    /* accepts trm_tangent_param_set and trm_adjoint_param_open, and the three stepping calls run with          */
                                    /* parameter seeds or an open parameter gradient: one launch carries the node seeds / gradients of the      */
                                    /* series and the thermal parameters' (TRM_INFO_LAST_PROGRAM: bits 26 / 30 and 31).  0 (default): the two   */
                                    /* together are refused with TRM_EUNSUPPORTED.  Without TRM_OPT_DERIVATIVE_SERIES it changes nothing        */
    ,TRM_OPT_DERIVATIVE_RICHARDS = 16 /* 1: the state-seed calls of the tangent -- trm_tangent_open, trm_tangent_upload, trm_tangent_download,   */
                                    /* trm_tangent_device_ptr, trm_tangent_closure and trm_step_tangent -- accept an fp64 heat + Richards        */
                                    /* SoilModel (ForwardEuler, Nz <= 64, the branch-free boundary kinds): seeds on the initial internal energy  */
                                    /* and the initial saturation, tangents of internal energy, saturation, temperature, liquid fraction and      */
                                    /* pressure head (TRM_TANGENT_SATURATION, TRM_TANGENT_PRESSURE_HEAD).  Every other derivative call -- seeds   */
                                    /* on boundaries, parameters or series, tangent records, every trm_adjoint_* opener -- refuses a Richards      */
                                    /* context with TRM_EUNSUPPORTED "on a Richards context: state seeds only".  0 (default): every derivative    */
                                    /* call refuses a Richards context as "the heat-only SoilModel (NoFlow) only"                                 */
    ,TRM_OPT_DERIVATIVE_RICHARDS_ADJOINT = 17 /* 1: the per-step tape of the adjoint -- trm_adjoint_open, trm_adjoint_close, trm_adjoint_upload,  */
                                    /* trm_adjoint_download, trm_adjoint_device_ptr, trm_adjoint_tape, trm_step_record and trm_adjoint_backward   */
                                    /* -- accepts what TRM_OPT_DERIVATIVE_RICHARDS opens to the tangent: cotangents of the final internal energy, */
                                    /* saturation, temperature, liquid fraction and pressure head (TRM_ADJOINT_SATURATION,                        */
                                    /* TRM_ADJOINT_PRESSURE_HEAD), gradients with respect to the initial internal energy and saturation.          */
                                    /* trm_adjoint_open_checkpointed, trm_adjoint_bc_open, trm_adjoint_param_open, every trm_adjoint_observe*     */
                                    /* and trm_adjoint_record_* refuse a Richards context with TRM_EUNSUPPORTED "on a Richards context:           */
                                    /* final-state cotangents on a per-step tape only".  Independent of TRM_OPT_DERIVATIVE_RICHARDS, which the    */
                                    /* tangent calls still need.  0 (default): every adjoint call answers a Richards context as without it        */
    ,TRM_OPT_DERIVATIVE_RICHARDS_PARAMS = 18 /* 1, together with TRM_OPT_DERIVATIVE_RICHARDS_ADJOINT = 1: trm_adjoint_param_open on a Richards   */
                                    /* context with an open per-step adjoint opens the gradients with respect to the seven hydraulic             */
                                    /* parameters (TRM_HYDRAULIC_PARAM_*), and trm_adjoint_backward forms them in the same sweep                  */
                                    /* (TRM_INFO_LAST_PROGRAM: bit 31).  trm_adjoint_bc_open, the checkpointed tape, observations and records     */
                                    /* stay refused there.  0 (default), or without that option: every call answers a Richards context as         */
                                    /* without it                                                                                                  */
    ,TRM_OPT_DERIVATIVE_RICHARDS_RECORD = 19 /* 1, together with TRM_OPT_DERIVATIVE_RICHARDS_ADJOINT = 1: the seven attached-record calls --     */
                                    /* trm_adjoint_observe_record, trm_adjoint_observe_record_device, trm_adjoint_record_detach,                  */
                                    /* trm_adjoint_record_residual_download, trm_adjoint_record_residual_device_ptr,                              */
                                    /* trm_adjoint_record_misfit_download and trm_adjoint_record_info -- accept a Richards context with an open   */
                                    /* per-step adjoint.  The record observes saturation_water_ice (a soil-moisture record) and is read inside    */
                                    /* the backward launches, with or without the hydraulic-parameter gradients of the option above               */
                                    /* (TRM_INFO_LAST_PROGRAM is that of the same launch without a record).  The per-position calls               */
                                    /* (trm_adjoint_observe, trm_adjoint_observe_misfit), trm_adjoint_open_checkpointed and trm_adjoint_bc_open   */
                                    /* stay refused there.  0 (default), or without that option: every call answers a Richards context as         */
                                    /* without it                                                                                                  */
};
/* DIAGNOSTIC, read-only (trm_get_option): which fast paths the NEXT step will take -- what the library tracks about its own
 * buffers.  Tests pin them (a wrong value costs speed, never correctness, so nothing else would notice). */
enum {
    TRM_INFO_TOP_ARRAYS_CURRENT = 100, /* 1: the LandModel's next surface evaluation reads the compact top-cell arrays the last   */
                                       /* fused step wrote (coalesced) instead of gathering one word per column from the fields   */
    TRM_INFO_CLOSURE_CONSISTENT = 101,  /* 1: the stored temperature / liquid fraction are the closure of the stored state, so a  */
                                       /* step may re-derive them in registers (TRM_OPT_DERIVE_CLOSURE_FIELDS).  "The next step   */
                                       /* may derive": stays 1 while the arrays themselves are stale (TRM_INFO_CLOSURE_STORED = 0) */
    TRM_INFO_GENERIC_BOUNDARY_KERNELS = 103, /* 1: the context's boundary kinds need the generic-boundary kernels (k_step_wave, ...)   */
    TRM_INFO_BC_SIGNATURE = 102,       /* the boundary-condition signature of the context's current kinds (BCSIG bits: 1 / 2 Value on  */
                                       /* temperature bottom / top, 4 / 8 Flux on energy / saturation bottom, 16 / 32 top, 64 LandModel) */
    TRM_INFO_LAST_PROGRAM = 105,       /* which kernel instance the last step launch of the context selected (TRM_PROGRAM_* below), 0     */
                                       /* before the first step: family in bits 0-7, then one field per selection rule                    */
    TRM_INFO_CLOSURE_STORED = 106,     /* 1: the temperature / liquid fraction ARRAYS are current; 0: the last step launches left them      */
                                       /* unstored (TRM_OPT_DEFER_CLOSURE_STORES) and the next reader materialises them                     */
    TRM_INFO_MATERIALIZATIONS = 107,   /* how many times the context has materialised them (one small launch each)                          */
    TRM_INFO_INTERIOR_LAUNCHES = 108,  /* how many step launches of the context were interior launches (TRM_OPT_INTERIOR_STEPS)             */
    TRM_INFO_DERIVATIVE_SERIES = 109   /* how many time series the last derivative launch of the context (tangent, record or backward)      */
                                       /* evaluated in the kernel (TRM_OPT_DERIVATIVE_SERIES); 0 otherwise                                  */
};
/* kernel families reported in the low byte of TRM_INFO_LAST_PROGRAM; bits 8-9 the hydraulics instance (0 the reference default, 1 van
 * Genuchten n = 2, 2 run-time exponents), 10-11 lanes per column / 32, 12-14 which closure fields are derived, 15 per-column outputs
 * staged, 16 per-column inputs through the scalar path, 17-24 the compiled-in boundary signature + 1 (0: kinds read at run time) */
enum {
    TRM_PROGRAM_NONE = 0, TRM_PROGRAM_COLUMN_EULER = 1, TRM_PROGRAM_COLUMN_HEUN = 2, TRM_PROGRAM_COLUMN_MULTI = 3,
    TRM_PROGRAM_PACKED_F32 = 4, TRM_PROGRAM_GENERIC_EULER = 5, TRM_PROGRAM_GENERIC_HEUN = 6, TRM_PROGRAM_COLUMN_LAND = 7,
    TRM_PROGRAM_DEEP = 8, TRM_PROGRAM_WIDE = 9, TRM_PROGRAM_LAND_INTERLEAVED = 10, TRM_PROGRAM_UNFUSED = 11, TRM_PROGRAM_VEGETATION = 12,
    TRM_PROGRAM_PACKED_LAND = 13, TRM_PROGRAM_COLUMN_TANGENT = 14,
    TRM_PROGRAM_COLUMN_ADJOINT = 15,
    TRM_PROGRAM_COLUMN_TANGENT_RICHARDS = 16,  /* trm_step_tangent on a Richards context: bits 8-9 the hydraulics, 10-11 lanes per column / 32 */
    TRM_PROGRAM_COLUMN_ADJOINT_RICHARDS = 17   /* trm_step_record and trm_adjoint_backward on a Richards context: the same bits */
};
/* bits of TRM_INFO_LAST_PROGRAM beside the ones above (25-27 are per family: surface processes inline / time series in the multi-step
 * program, the program and the generic boundaries of the deep and wide columns): how the step's time averages were accumulated
 * (trm_average_open) -- by the step launch itself (the resident multi-step program), or by a k_accumulate launch behind it.  Neither is
 * set while no accumulator is open. */
enum { TRM_PROGRAM_AVERAGES_IN_LAUNCH = 268435456 /* 1 << 28 */, TRM_PROGRAM_AVERAGES_AFTER_LAUNCH = 536870912 /* 1 << 29 */ };
/* ... and bit 31, the last one the two derivative families leave free (25-27 and 30 are taken there, 28-29 above): the launch carried
 * seeds on, or formed the gradient with respect to, the thermal parameters (trm_tangent_param_set, trm_adjoint_param_open) or, in the
 * family TRM_PROGRAM_COLUMN_ADJOINT_RICHARDS, the hydraulic parameters (TRM_OPT_DERIVATIVE_RICHARDS_PARAMS).  The id is an
 * int: with this bit it reads as a negative number, and the bits are those of its two's complement. */
enum { TRM_PROGRAM_PARAMETERS = (-2147483647 - 1) /* bit 31 */ };
enum {
    TRM_KERNEL_FUSED = 0,       /* one launch per step: lane = soil level, a column per (half-)wavefront,     */
                                /* wavefront shuffles for the vertical stencil (Nz <= 64; two levels per lane */
                                /* for 65 ... 128 levels, four for 129 ... 256: ForwardEuler and Heun with    */
                                /* every boundary kind; anything deeper takes the unfused kernels)            */
    TRM_KERNEL_UNFUSED = 1      /* one launch per reference kernel, in the reference's order (A/B comparator) */
};

/* ---- grid: ColumnGrid(arch, NF, vert, num_columns)  src/grids/column_grid.jl:20-34 */
typedef struct trm_grid {
    int32_t precision;        /* TRM_F64 | TRM_F32                                                        */
    int32_t num_layers;       /* Nz >= 2                                                                   */
    int64_t num_columns;      /* Nh >= 1 (this device's shard)                                             */
    const double* thickness;  /* [Nz] get_spacing(vert): index 0 = SURFACE layer (vertical_discretization.jl:20) */
    double dx;                /* x spacing of the underlying RectilinearGrid; <= 0 selects 1/Nh (x = (0,1)) */
    int32_t device;           /* HIP device ordinal                                                        */
    int32_t reserved;
} trm_grid;

/* ---- parameters: the flat POD of SURVEY 8(a12); defaults = reference defaults -- */
typedef struct trm_params {
    /* PhysicalConstants  src/processes/physical_constants.jl:9-51 */
    double rho_w, rho_i, rho_a, c_a, Lsl, Llg, Lsg, g, Tref, sigma, kappa_vk, eps_mw, R_a;
    /* SoilThermalConductivities / SoilHeatCapacities  soil_thermal_properties.jl:14-46 */
    double k_water, k_ice, k_air, k_mineral, k_organic;
    double c_water, c_ice, c_air, c_mineral, c_organic;
    /* ConstantSoilPorosity soil_porosity.jl:7-13; ConstantSoilCarbonDensity constant_soil_carbon.jl:10-16 */
    double por_mineral, por_organic, rho_soc, rho_org;
    /* ConstantSoilHydraulics / SoilHydraulicsSURFEX + SWRC + UnsatK  soil_hydraulic_properties.jl:66-221 */
    double K_sat, theta_res, bc_psi_s, bc_lambda, vg_alpha, vg_n, impedance;
    double vwc_forcing;       /* spatially constant vwc_forcing source/sink [1/s] (soil_hydrology.jl:37-38) */
    /* ConstantAlbedo, ImplicitSkinTemperature, ConstantAerodynamics, PrescribedAtmosphere,
     * DirectSurfaceRunoff, ConstantEvaporationResistanceFactor */
    double albedo, emissivity, kappa_s, C_h, min_windspeed, tau_r, beta_evap;
    double field_capacity;    /* field_capacity(hydraulic_properties, texture) (soil_hydraulic_properties.jl:93-97,150-155): read by
                                 the soil-moisture evaporation resistance only                                        */
    int32_t flow;             /* TRM_FLOW_*                                                               */
    int32_t swrc;             /* TRM_SWRC_*                                                               */
    int32_t unsat_k;          /* TRM_UNSATK_*                                                             */
    int32_t seb;              /* 0: SoilModel; 1: LandModel(vegetation = nothing) coupling (land_model.jl) */
    int32_t halo_policy;      /* TRM_HALO_*                                                               */
    int32_t prescribed_albedo;/* 0: ConstantAlbedo (the two scalars above); 1: PrescribedAlbedo -- per-column inputs
                                 TRM_FIELD_ALBEDO / TRM_FIELD_EMISSIVITY (albedo.jl:8-14, abstract_types.jl:120-131)   */
    int32_t evap_resistance;  /* ground evaporation resistance factor beta (ground_resistance_factor.jl): 0 = constant
                                 `beta_evap` (ConstantEvaporationResistanceFactor), 1 = SoilMoistureResistanceFactor:
                                 (1 - cos(pi * theta_1 / theta_fc))^2 / 4 below field capacity, 1 above (Lee & Pielke 1992) */
    int32_t reserved;
} trm_params;

/* Fill `p` with the reference defaults. */
int trm_default_params(trm_params* p);

/* ---- vegetation: the parameter structs of VegetationCarbon's processes (needleleaf-tree PFT defaults) --------------- */
typedef struct trm_vegetation_params {
    /* LUEPhotosynthesis  photosynthesis.jl:17-68 */
    double tau25, Kc25, Ko25, q10_tau, q10_Kc, q10_Ko, alpha_leaf, alpha_a, alpha_C3, cq, k_ext, T_CO2_high, T_CO2_low,
        T_photos_high, T_photos_low, theta_r;
    /* MedlynStomatalConductance  stomatal_conductance.jl:16-24 */
    double g1, g_min;
    /* PALADYNAutotrophicRespiration  autotrophic_respiration.jl:14-23 */
    double cn_sapwood, cn_root, aws;
    /* PALADYNCarbonDynamics  carbon_dynamics.jl:18-43 */
    double SLA, awl, LAI_min, LAI_max, gamma_L, gamma_R, gamma_S;
    /* PALADYNVegetationDynamics  vegetation_dynamics.jl:15-22 */
    double nu_seed, gamma_v_min;
    /* StaticExponentialRootDistribution  root_distribution.jl:23-29 */
    double root_a, root_b;
    /* wilting point / field capacity of the soil's hydraulic properties (FieldCapacityLimitedPAW) */
    double wilting_point, field_capacity;
    /* PhysicalConstants.C_mass  physical_constants.jl:50 */
    double C_mass;
    /* PALADYNCanopyInterception (canopy_interception.jl:37-49): interception factor, canopy extinction coefficient,
     * interception capacity [m], removal timescale [s]; PALADYNCanopyEvapotranspiration.C_can: ground-canopy drag
     * coefficient (canopy_evapotranspiration.jl:33-40).  Used by TRM_VEGETATION_COUPLED only. */
    double alpha_int, canopy_k_ext, w_can_max, tau_w, C_can;
} trm_vegetation_params;
int trm_default_vegetation_params(trm_vegetation_params* p);
/* Enables the vegetation processes of the context (allocating their 3-D fields, setting the input defaults and the static
 * root fractions).  TRM_VEGETATION_STANDALONE: the context IS a VegetationModel (src/models/vegetation/vegetation_model.jl):
 * trm_step / trm_step_heun / trm_update_state / trm_compute_auxiliary / trm_compute_tendencies / trm_explicit_step act on
 * the vegetation state alone; soil moisture limitation and ground temperature are inputs.  One launch covers
 * update_state! + explicit_step! for all `nsteps` (the 0-D column stays in registers).
 * TRM_VEGETATION_COUPLED (contexts with surface_energy_balance = 1): LandModel(grid; soil, vegetation) of
 * src/models/coupled/land_model.jl:79-97.  compute_auxiliary! becomes soil hydraulics -> plant available water from the
 * soil state, ground temperature = top soil cell, the vegetation processes -> canopy interception -> canopy
 * evapotranspiration (transpiration through the stomatal conductance, ground evaporation below the canopy, evaporation of
 * intercepted water) -> runoff of the rain reaching the ground -> the surface energy balance with the latent heat of all
 * three humidity fluxes; canopy_water, carbon_vegetation and vegetation_area_fraction are stepped with the soil.  The
 * 0-D part of one step is ONE launch in front of the soil column kernel; the resident multi-step program does not apply
 * (Euler steps run one launch pair each).  trm_step_heun takes four launches per step: the 0-D processes at the state, the
 * soil column with both stages in registers (storing only what the 0-D processes need of the stage), the 0-D processes at
 * the stage, the averaged 0-D update. */
enum { TRM_VEGETATION_OFF = 0, TRM_VEGETATION_STANDALONE = 1, TRM_VEGETATION_COUPLED = 2 };
int trm_set_vegetation(trm_ctx* ctx, const trm_vegetation_params* p, int mode);
/* FieldCapacityLimitedPAW (plant_available_water.jl:36-94): plant_available_water per cell from the soil state of the
 * context and soil_moisture_limiting_factor = sum_k PAW_k * root_fraction_k. */
int trm_compute_plant_available_water(trm_ctx* ctx);

/* initialize(model, timestepper) allocation part (src/state_variables.jl:303-314, 418-430):
 * creates all state buffers on `g->device`, zero-filled, inputs at their defaults. */
int trm_create(const trm_grid* g, const trm_params* p, trm_ctx** out);
int trm_destroy(trm_ctx* ctx);
const char* trm_last_error(const trm_ctx* ctx);
int trm_abi_version(void);

/* Geometry queries: rows of a field (Nz, Nz+1 or 1), and the grid the library derived
 * (z of faces [Nz+1] bottom first, z of centres [Nz], dz centre [Nz], dz face [Nz+1]). */
int trm_field_rows(const trm_ctx* ctx, int field, int64_t* rows);
int trm_get_grid(const trm_ctx* ctx, double* z_faces, double* z_centers, double* dz_center, double* dz_face);

/* set!(field, array) / Array(interior(field)) */
int trm_upload(trm_ctx* ctx, int field, const void* host);
int trm_download(trm_ctx* ctx, int field, void* host);
/* Rows [row0, row0 + nrows) of a field, host layout [nrows][num_columns]: `ground_temperature` (soil_energy.jl:52-57) is
 * row Nz - 1 of temperature -- one row through PCIe, not the field. */
int trm_download_rows(trm_ctx* ctx, int field, int row0, int nrows, void* host);
/* ---- ColumnRingGrid (src/grids/column_ring_grid.jl:37-59,102-149) -------------------------------------------------------
 * trm_set_ring_grid: the columns of the context are the points `mask_index[i]` (strictly increasing, one per column) of a
 * full grid of `num_points` points in ring order -- `findall(mask)`; for a context that holds one shard of the columns, the
 * shard's slice of that list.  Uploaded once; scatter / gather then run on the device:
 *   trm_download_ring / trm_scatter_ring_device   RingGrids.Field(field, grid; fill_value) (lines 102-115): rows of a field
 *       on the full grid, [nrows][num_points], `fill` outside the mask -- into host memory, or into a device buffer of a
 *       coupled model on the same device (speedy_dry_land.jl:45-66 reads the land state as ring-grid fields)
 *   trm_upload_ring / trm_gather_ring_device      Oceananigans.Field(ring_field, grid) (lines 117-149): the masked points of
 *       a full-grid array [rows][num_points] become the field (all rows of it) */
int trm_set_ring_grid(trm_ctx* ctx, int64_t num_points, const int64_t* mask_index);
int trm_download_ring(trm_ctx* ctx, int field, int row0, int nrows, double fill, void* host);
int trm_scatter_ring_device(trm_ctx* ctx, int field, int row0, int nrows, double fill, void* dev_out);
int trm_upload_ring(trm_ctx* ctx, int field, const void* host_full);
int trm_gather_ring_device(trm_ctx* ctx, int field, const void* dev_full);
/* Device address of a field, for zero-copy consumers on the same device.  The device layout is z-fastest:
 * element (column i, level k) of a 3-D field is at dev[i * pitch_elems + k] (pitch 32 for Nz <= 32, 64 for
 * Nz <= 64); 2-D fields are dev[i] (pitch 1).  The top face of hydraulic_conductivity is not part of this
 * buffer (use trm_download).  The 3-D vegetation fields TRM_FIELD_PLANT_AVAILABLE_WATER and TRM_FIELD_ROOT_FRACTION are allocated by
 * trm_set_vegetation: before it the call fails with TRM_EINVAL ("the field exists only after trm_set_vegetation") instead of handing
 * back a null address, as does trm_stage_field_device_ptr. */
int trm_field_device_ptr(trm_ctx* ctx, int field, void** dev, int64_t* pitch_elems);

/* Field boundary conditions (src/models/soil/soil_model_bcs.jl, src/boundary_conditions.jl:25-28):
 * `values` is a per-column array [Nh] or NULL to broadcast `scalar`. */
/* Device array [num_columns] of the boundary values of (var, side), as set by trm_set_bc / trm_set_bc_series: a coupled
 * model that lives on the same device writes the next coupling interval's values there itself (the SpeedyWeather
 * coupling of examples/simulations/speedy_dry_land.jl:45-66 does `set!(state.inputs.air_temperature, Tair)` per coupling
 * step).  Valid until the context is destroyed; writes must be ordered before the next trm_step on the context's stream
 * (trm_set_stream) or by a device synchronisation.  Fails if the condition carries no values (NoFlux) or a time series. */
int trm_bc_device_ptr(trm_ctx* ctx, int var, int side, void** dev);
int trm_set_bc(trm_ctx* ctx, int bc_var, int side, int kind, const void* values, double scalar);
/* update_inputs! (src/state_variables.jl:154-162): same as trm_upload on an input field. */
int trm_set_forcing(trm_ctx* ctx, int input_field, const void* per_column);
/* The same from DEVICE memory, stream-ordered: `dev_per_column` ([num_columns], context precision, on the context's device) is
 * copied into the input field on the context stream without synchronising the host -- a coupled model on the same device hands
 * over the next coupling interval's inputs between two asynchronous trm_step calls (speedy_dry_land.jl:45-68 does
 * `set!(state.inputs.air_temperature, Tair)` per coupling step).  The source must stay valid until the copy has executed
 * (trm_synchronize, or stream order on a shared stream: trm_set_stream).  Zero-copy alternative: write the field's own
 * buffer (trm_field_device_ptr) on the context stream. */
int trm_set_forcing_device(trm_ctx* ctx, int input_field, const void* dev_per_column);

/* ---- time series input sources --------------------------------------------------------------------------
 * FieldTimeSeriesInputSource (src/input_output/input_sources.jl:142-171): update_inputs! sets the input
 * field to `fts[Time(clock.time)]`, Oceananigans' time interpolation of a FieldTimeSeries.  Here the whole
 * series lives in HBM ([nt][Nh], uploaded once; 288 GB hold years of hourly forcing for a shard), and every
 * step of a trm_step / trm_step_heun loop evaluates it at the context clock before anything else runs, so one
 * call can span any number of forcing intervals.  `times` must be strictly increasing; nt >= 1.
 * The same mechanism drives time-dependent boundary values (the reference's functional / discrete-form
 * boundary conditions, evaluated on its own clock).
 *   TRM_TIME_LINEAR    linear interpolation, linear extrapolation outside [t_1, t_nt]   (Oceananigans `Linear`)
 *   TRM_TIME_CLAMP     linear interpolation, end values outside                         (`Clamp`)
 *   TRM_TIME_CYCLICAL  periodic with period (t_nt - t_1) + (t_nt - t_{nt-1})            (`Cyclical`)
 * Between nodes n1 < n2: value = v[n2] * f + v[n1] * (1 - f), f = (1 / (t[n2] - t[n1])) * (t - t[n1]), evaluated in
 * double and rounded once to the context precision; on an interior node the node's values are copied.
 *   TRM_TIME_RASTER    the Raster input source of ext/TerrariumRastersExt (lines 96-121): between nodes
 *                      v[n1] + (t - t[n1]) * (v[n2] - v[n1]) / (t[n2] - t[n1]) with (v[n2] - v[n1]) formed in the context
 *                      precision and the rest in double, the node's values on a node, the end values beyond the ends */
enum { TRM_TIME_LINEAR = 0, TRM_TIME_CLAMP = 1, TRM_TIME_CYCLICAL = 2, TRM_TIME_RASTER = 3 };
/* `values`: [nt][Nh] in the context precision.  Replaces any earlier series or constant of the same input. */
int trm_set_forcing_series(trm_ctx* ctx, int input_field, int nt, const double* times, const void* values, int time_indexing);
/* Boundary value series for (bc_var, side) with the given kind (VALUE / FLUX / GRADIENT). */
int trm_set_bc_series(trm_ctx* ctx, int bc_var, int side, int kind, int nt, const double* times, const void* values, int time_indexing);
/* Drops every series (inputs and boundary values keep what was last evaluated). */
int trm_clear_series(trm_ctx* ctx);
/* update_inputs!(state, clock): evaluates every series at the context clock (done implicitly by trm_step,
 * trm_step_heun and trm_update_state). */
int trm_update_inputs(trm_ctx* ctx);

/* ---- windowed time series -----------------------------------------------------------------------------
 * A forcing record that does not fit in HBM -- one hourly year of the 7 atmospheric inputs is ~199 GB for a 0.1-degree shard --
 * streams through a fixed window: create the series with its first levels (trm_set_forcing_series / trm_set_bc_series),
 * then alternate
 *     trm_series_trim_before(ctx, t)        -- releases the levels no evaluation at a time >= t can touch (the node at or
 *                                              before t and everything after it stay)
 *     trm_series_append(ctx, ...)           -- continues a series with `nt` further levels (`times` strictly increasing
 *                                              and beyond the last level held).  The values are staged through pinned
 *                                              memory and copied on a side stream UNDER whatever the context stream is
 *                                              running; the next step that evaluates the series waits for them.  Freed
 *                                              slots of the ring are reused; without free slots the ring grows.
 * `is_bc` = 0: `id` is the input field, `side` ignored; `is_bc` = 1: `id` is the bc_var, `side` the boundary.  Results
 * are bit-identical to the all-resident series as long as the window covers [t, t + dt] of every step taken (FieldTimeSeries
 * `InMemory(chunk)` backends play this role on the reference side).  TRM_TIME_CYCLICAL series cannot be windowed. */
int trm_series_append(trm_ctx* ctx, int is_bc, int id, int side, int nt, const double* times, const void* values);
/* Declares a series as WINDOWED (trm_series_append does the same implicitly): only windowed series are touched by
 * trm_series_trim_before -- a fully resident series that lives in the same context keeps its whole record -- and a windowed
 * series refuses (TRM_EINVAL) an evaluation at a time before the levels it still holds instead of extrapolating from its trimmed
 * head.  `levels` > the levels held reserves ring capacity for that many (0: leave the capacity as it is). */
int trm_series_window(trm_ctx* ctx, int is_bc, int id, int side, int levels);
int trm_series_trim_before(trm_ctx* ctx, double t);
int trm_series_info(const trm_ctx* ctx, int is_bc, int id, int side, int64_t* levels_held, int64_t* capacity, double* t_first, double* t_last);

/* reset!(state) + reset!(clock) of initialize!(integrator) (state_variables.jl:102-120, model_integrator.jl:96-99): every
 * prognostic, auxiliary and tendency field to zero, the status word cleared, the clock to (0, 0).  Inputs keep their values
 * (initialize!(state, inputs) re-evaluates their sources next), as do boundary values, series and options. */
int trm_reset(trm_ctx* ctx);

/* initialize!(state, model) process initialisers (soil_coupled.jl:45-54): hydraulics, water table,
 * sat -> psi, T -> U.  Call after uploading the initial temperature / saturation. */
int trm_initialize(trm_ctx* ctx);
/* update_state!(state, model, inputs; compute_tendencies)  src/state_variables.jl:72-80 */
int trm_update_state(trm_ctx* ctx, int compute_tendencies);
/* compute_auxiliary!(state, model)  soil_model.jl:39-42 / land_model.jl:79-88 */
int trm_compute_auxiliary(trm_ctx* ctx);
/* compute_tendencies!(state, model) soil_model.jl:44-47 (accumulates into the tendency fields) */
int trm_compute_tendencies(trm_ctx* ctx);
/* reset_tendencies!(state)  src/state_variables.jl:127-136 */
int trm_reset_tendencies(trm_ctx* ctx);
/* explicit_step!(state, grid, timestepper, dt)  abstract_timestepper.jl:65-77 */
int trm_explicit_step(trm_ctx* ctx, double dt);
/* closure!/invclosure!(state, model)  soil_coupled.jl:99-122 */
int trm_closure(trm_ctx* ctx);
int trm_invclosure(trm_ctx* ctx);

/* `nsteps` x timestep!(integrator, ForwardEuler, dt; finalize = false), then compute_auxiliary! once
 * if `finalize` (forward_euler.jl:19-31, model_integrator.jl:72-88,124-131).  nsteps = 1, finalize = 1
 * is the reference's timestep!(integrator, dt); finalize = 1 with nsteps = n is run!(steps = n).
 *
 * Tendency fields (TRM_FIELD_TEND_*): the reference leaves the last step's tendencies -- compute_tendencies! plus the
 * flux-boundary term compute_z_bcs! adds inside explicit_step!, averaged over the two stages for Heun -- in
 * state.tendencies.  The fused kernels (TRM_KERNEL_FUSED) keep tendencies in registers and store them only from the
 * launch that finalizes: after a call with finalize = 1 the tendency fields hold exactly what the reference's would;
 * after a call with finalize = 0 they are NOT materialised and trm_download / trm_reduce / trm_field_device_ptr of a
 * TRM_FIELD_TEND_* field fail with TRM_ESTALE until trm_update_state(ctx, 1), trm_reset_tendencies or a finalizing
 * step has run.  TRM_KERNEL_UNFUSED materialises them at every step.
 *
 * Temperature and liquid_water_fraction read through the library are always what the reference's would be.  Under
 * TRM_OPT_DEFER_CLOSURE_STORES (default) the large-grid per-step launches, which derive both from (internal_energy, saturation) at
 * entry, do not store them; the first call after such steps that touches field memory -- any download, upload, reduction,
 * trm_field_device_ptr, trm_save_state, trm_average_open, another kind of step ... -- first forms them with one small launch on the
 * context stream (no error code, nothing to call).  trm_step, trm_step_timed, trm_step_all, trm_synchronize(_all), trm_status, the
 * clock and option getters and trm_last_error do not.  A device pointer to a state field ends deferral for the context. */
int trm_step(trm_ctx* ctx, double dt, int nsteps, int finalize);
/* Same for Heun (heun.jl:37-71): with TRM_KERNEL_FUSED and Nz <= 64 ONE launch per step (both stages on the column held in
 * registers; the stage never touches memory; every boundary kind), four for TRM_VEGETATION_COUPLED; ONE launch for 65 ... 128
 * levels with the branch-free boundary kinds as well; otherwise the reference-order kernels on a second copy of the state. */
int trm_step_heun(trm_ctx* ctx, double dt, int nsteps, int finalize);
/* DIAGNOSTIC (benchmarks): as trm_step, bracketed by HIP events on the context stream: *ms = device time of the launches. */
int trm_step_timed(trm_ctx* ctx, double dt, int nsteps, int finalize, float* ms);
/* The same for trm_step_heun. */
int trm_step_heun_timed(trm_ctx* ctx, double dt, int nsteps, int finalize, float* ms);

/* ---- Heun with state-dependent forcings / boundary values (heun.jl:37-71 with forcings.jl:13-19, boundary_conditions.jl:25-28) --
 * The reference evaluates a user's `forcing(i, j, k, grid, clock, fields)` / `getbc(..., clock, fields)` inside the tendency
 * kernel at BOTH Heun stages: at the state (clock t) and at the stage (the predicted state, clock t + dt).  A closure cannot
 * cross a C ABI; its values can, without leaving the device (see trm_field_device_ptr): the caller evaluates its function on
 * the state's buffers into the state's boundary / input / vwc_forcing buffers, then
 *     trm_heun_predict(ctx, dt)            -- heun.jl:41-52: update_state!(state), stage := state, explicit_step!(stage),
 *                                             closure!(stage), tick!(stage.clock); series are evaluated at t + dt for the stage
 *     (the caller evaluates its function on the STAGE's buffers -- trm_stage_field_device_ptr -- into the stage's boundary /
 *      input / vwc_forcing buffers -- trm_stage_bc_device_ptr, trm_stage_field_device_ptr of the input --, on the context stream)
 *     [trm_heun_stage_auxiliary(ctx)       -- the first half of update_state!(stage): reset tendencies, compute_auxiliary!(stage).
 *      (then the caller evaluates what the reference evaluates INSIDE compute_tendencies!(stage): a forcing function)]
 *     trm_heun_correct(ctx, dt, finalize)  -- heun.jl:54-71: update_state!(stage) (what is left of it), average_tendencies!,
 *                                             explicit_step!(state), closure!(state), tick!(clock) (+ compute_auxiliary! if `finalize`)
 * WHAT THE STAGE'S FIELDS HOLD when the caller reads them: after trm_heun_predict every field of the stage is the reference's at
 * the same point -- prognostic and closure fields of the predicted state, auxiliary fields (hydraulic_conductivity, the surface
 * fluxes, ...) still the STATE's copies (copyto!(stage, state), heun.jl:45): what a boundary-value function finds when
 * fill_halo_regions! evaluates it, BEFORE compute_auxiliary!(stage).  After trm_heun_stage_auxiliary the auxiliary fields are the
 * stage's own: what a forcing function finds inside the tendency kernel.  The stage's clock has ticked: time t + dt, iteration + 1.
 * The pair equals one trm_step_heun(ctx, dt, 1, finalize) bit for bit when the stage's values are the ones the library would
 * have used itself.  It runs on the reference-order kernels (the stage lives in memory between the two calls by construction).
 * A boundary condition or input whose stage buffer has been handed out keeps it; trm_step_heun refreshes such buffers from
 * the state's values at every step, so mixing the two forms is safe.
 * Any other call that writes the state, the clock, a boundary condition or an option between trm_heun_predict and trm_heun_correct
 * drops the predicted stage: trm_heun_correct then fails with TRM_EINVAL instead of correcting with a stage of another state. */
int trm_heun_predict(trm_ctx* ctx, double dt);
int trm_heun_stage_auxiliary(trm_ctx* ctx);
int trm_heun_correct(trm_ctx* ctx, double dt, int finalize);
/* Device address of a field of the Heun STAGE (layout as trm_field_device_ptr): the predicted state after trm_heun_predict --
 * to read --, or an input field / TRM_FIELD_VWC_FORCING of the stage -- to write before trm_heun_correct. */
int trm_stage_field_device_ptr(trm_ctx* ctx, int field, void** dev, int64_t* pitch_elems);
/* Device array [num_columns] of the STAGE's boundary values of (var, side) (allocated on first use as a copy of the state's) */
int trm_stage_bc_device_ptr(trm_ctx* ctx, int var, int side, void** dev);

/* ---- DIAGNOSTIC entry points (benchmarks, tests; not part of the reference interface) -----------------------------------
 * trm_step_timed / trm_step_heun_timed (above) and the device-side one-slot snapshot below exist for bench.py and the A/B
 * tools: a binder of the reference interface does not need them.  Restart files go through trm_download / trm_upload /
 * trm_set_clock ("Restart").
 * Device-side checkpoint of the whole state (every field, the clock, the status word): trm_save_state copies it into
 * a second set of buffers owned by the context, trm_restore_state copies it back.  One slot; no host traffic. */
int trm_save_state(trm_ctx* ctx);
int trm_restore_state(trm_ctx* ctx);

/* ---- time averages (Oceananigans' AveragedTimeInterval / WindowedTimeAverage as the reference's output writers use them) -------
 * An accumulator lives in the context and sums one field over a window of steps; one handle per (field, window), so two writers can
 * average the same field over different windows.
 *   trm_average_open(ctx, field, &handle)   allocates an accumulator of `field`, zero, window length 0
 *   trm_average_reset(ctx, handle)          starts a new window: sum and window length to zero
 *   trm_average_read(ctx, handle, host, &window_seconds, &steps)
 *                                           mean = sum / window_seconds, rounded once to the context precision, host layout
 *                                           [rows][Nh] as trm_download; window_seconds and steps may be NULL.  A window of zero
 *                                           steps is TRM_ESTALE.
 *   trm_average_close(ctx, handle)          releases it; the handle is invalid from then on (TRM_EINVAL)
 * Arithmetic.  Every step taken by a STEPPING entry point -- trm_step, trm_step_heun, trm_heun_correct, their _timed forms,
 * trm_step_all / trm_step_heun_all -- adds to every open accumulator, per launch:
 *     acc[i] <- acc[i] + P[i],   window <- window + dt (per step, in order),   P[i] = sum_k (double)dt * (double)x_k[i]
 * where x_k is the field after step k of the launch and P starts at 0.0 and adds the launch's steps in order (a launch of one step:
 * one term).  Products and sums are rounded separately; accumulators and partials are double for both precisions.  The value counted
 * is the one after the step (right endpoint, weight dt): our reading of Oceananigans' WindowedTimeAverage with stride 1, from memory
 * -- no reference-held value pins it.  "After the step" is what the step leaves in the field: the prognostic and closure fields of
 * the new state, the water table of the new state, and the surface diagnostics (skin temperature, fluxes) as the step's own surface
 * processes formed them -- the evaluation a finalizing call adds afterwards (compute_auxiliary!) is not counted.
 * Component calls (trm_explicit_step, trm_update_state, trm_heun_predict, ...) do not accumulate.  trm_reset zeroes every open
 * accumulator and keeps the handles; trm_save_state / trm_restore_state do not include accumulators.
 * Fields: internal energy, saturation, temperature, liquid fraction, pressure head, surface excess water, water table; with the
 * LandModel also skin temperature, ground heat flux, shortwave up, longwave up, net radiation, sensible and latent heat flux, ground
 * evaporation, infiltration and surface runoff.  Anything else (tendencies, inputs, vegetation) is TRM_EUNSUPPORTED, as is a
 * surface field of a SoilModel and any field of a standalone VegetationModel.
 * Paths (TRM_INFO_LAST_PROGRAM: TRM_PROGRAM_AVERAGES_*): the resident multi-step program accumulates in its own launch; every other
 * program is followed by one k_accumulate launch per step, and while an open accumulator needs that path (a multi-step program
 * without the accumulation: deep columns; a field the fused form does not cover) the library steps one launch per step. */
int trm_average_open(trm_ctx* ctx, int field, int* handle);
int trm_average_reset(trm_ctx* ctx, int handle);
int trm_average_read(trm_ctx* ctx, int handle, void* host, double* window_seconds, int64_t* steps);
int trm_average_close(trm_ctx* ctx, int handle);

/* ---- forward-mode tangents of the heat-only step (the reference differentiates timestep! with Enzyme) -----------------------------
 * Tangents with respect to the initial internal energy of a SoilModel with NoFlow, ForwardEuler, fp64, Nz <= 64, every boundary kind
 * of the heat-only programs (NoFlux, Value / Gradient on temperature, Flux on energy) and both halo policies.  Boundary values are
 * constants: their tangent is 0 unless trm_tangent_bc_upload seeds them (below).
 *   trm_tangent_open(ctx)                   allocates the three tangent fields below, Nz rows each, zero
 *   trm_tangent_close(ctx)                  frees them
 *   trm_tangent_upload / _download(ctx, which, host)
 *                                           host layout [Nz][Nh] as trm_upload / trm_download of a 3-D field
 *   trm_tangent_device_ptr(ctx, which, &dev, &pitch)
 *                                           device layout as trm_field_device_ptr: element (level k, column i) at dev[i * pitch + k]
 *   trm_tangent_closure(ctx)                dT and dliq from the stored U and dU: the tangent of trm_closure
 *   trm_step_tangent(ctx, dt, nsteps)       nsteps ForwardEuler steps of the state and its tangent.  The state afterwards -- every
 *                                           field, the status word, the clock -- is that of trm_step(ctx, dt, nsteps, 1), bit for bit;
 *                                           dU, dT, dliq are the tangents of the new U, T, liq.  The stored T and liq are taken to
 *                                           be the closure of the stored U (true after trm_initialize, trm_closure and every step).
 * The tangent follows the branch of the closure the primal takes in every cell: dT = dU / C thawed or frozen, 0 in phase change;
 * dliq = -dU / (-L_theta + eps) in phase change, 0 otherwise (and where L_theta = 0).
 * TRM_INFO_LAST_PROGRAM of a trm_step_tangent is TRM_PROGRAM_COLUMN_TANGENT (bit 25: Gradient halos on temperature, where trm_step
 * takes the generic-boundary kernel).  Up to TRM_OPT_STEPS_PER_LAUNCH steps per launch (0: as trm_step).
 * Errors: TRM_EINVAL without a context or an open tangent; TRM_EUNSUPPORTED for fp32, Richards, the LandModel or vegetation,
 * Nz > 64, an attached time series, an open time average, a Value or Gradient condition on saturation, liquid fraction or pressure
 * head, or a per-cell vwc_forcing field.  Every other call that changes the state -- trm_step, trm_step_heun, the two-call Heun,
 * trm_explicit_step, trm_initialize, trm_invclosure, trm_upload of internal energy or saturation, trm_restore_state, trm_reset --
 * makes the tangent stale: trm_tangent_download of dT or dliq, trm_tangent_closure and trm_step_tangent return TRM_ESTALE until a
 * new trm_tangent_upload of dU seeds it again.
 * Heat + Richards, with TRM_OPT_DERIVATIVE_RICHARDS set: the seven calls above accept an fp64 SoilModel with RichardsEq on the branch-free
 * boundary kinds.  trm_tangent_open allocates five fields there: the three above, TRM_TANGENT_SATURATION and TRM_TANGENT_PRESSURE_HEAD,
 * which exist only while a tangent is open on a Richards context (on a NoFlow context the indices 3 and 4 are a bad argument).  The seeds
 * are dU and dsat: trm_tangent_upload takes `which` 0 and 3 there, trm_tangent_download and trm_tangent_device_ptr 0 ... 4;
 * trm_tangent_closure forms dT, dliq and dpsi from the stored state, dU and dsat; trm_step_tangent leaves the state of
 * trm_step(ctx, dt, nsteps, 1) bit for bit -- saturation, pressure head, water table, surface_excess_water, hydraulic conductivity and the
 * tendencies included -- and the five tangents (TRM_INFO_LAST_PROGRAM: TRM_PROGRAM_COLUMN_TANGENT_RICHARDS).  The tangent of
 * surface_excess_water is not formed.  The staleness rules are the ones above (trm_upload of the saturation makes the tangent stale). */
enum { TRM_TANGENT_INTERNAL_ENERGY = 0, TRM_TANGENT_TEMPERATURE = 1, TRM_TANGENT_LIQUID_WATER_FRACTION = 2,
       TRM_TANGENT_SATURATION = 3,      /* Richards contexts only: the seed / tangent of saturation_water_ice */
       TRM_TANGENT_PRESSURE_HEAD = 4 }; /* Richards contexts only: the tangent of pressure_head (an output: not uploaded) */
int trm_tangent_open(trm_ctx* ctx);
int trm_tangent_close(trm_ctx* ctx);
int trm_tangent_upload(trm_ctx* ctx, int which, const void* host);
int trm_tangent_download(trm_ctx* ctx, int which, void* host);
int trm_tangent_device_ptr(trm_ctx* ctx, int which, void** dev, int64_t* pitch_elems);
int trm_tangent_closure(trm_ctx* ctx);
int trm_step_tangent(trm_ctx* ctx, double dt, int nsteps);
/* Seeds on the boundary values: the tangent with respect to what drives the run.  A boundary value enters the heat-only step as a Value
 * or a Gradient on temperature (also a zero Gradient at the bottom, which the primal skips: its derivative is not zero) or as a Flux on
 * internal energy; the values are constant over the steps, and so are their seeds.
 *   trm_tangent_bc_upload(ctx, bc_var, side, host)
 *                                           host[num_columns] doubles: the seed d(value) of the pair (bc_var, side), bc_var
 *                                           TRM_BCV_TEMPERATURE or TRM_BCV_INTERNAL_ENERGY, side TRM_BOTTOM or TRM_TOP.  The four seed
 *                                           arrays are allocated by the first upload, zeroed by trm_tangent_open and freed by
 *                                           trm_tangent_close.  A pair whose current kind reads no value contributes nothing, whatever
 *                                           its seed.  Seeds are not state: no call makes them stale, and the upload does not seed dU
 *                                           (a stale tangent stays stale).
 * Once a seed has been uploaded since trm_tangent_open, trm_step_tangent runs the seeded instances: TRM_INFO_LAST_PROGRAM carries
 * bit 26.  The state afterwards is still that of trm_step, bit for bit, and zero seeds give the tangents of the unseeded run.
 * Errors: TRM_EINVAL without a context or an open tangent, for any other bc_var, a side other than 0 / 1, or a NULL pointer. */
int trm_tangent_bc_upload(trm_ctx* ctx, int bc_var, int side, const void* host);
/* Seeds on a boundary time series (TRM_OPT_DERIVATIVE_SERIES = 1): the tangent with respect to the record that drives the run.  With the
 * option set, trm_step_tangent accepts boundary series on the four pairs above (Value on temperature, Flux on internal energy; whole
 * records on the branch-free boundary kinds) and evaluates them in the launch, in front of every step, as trm_step does: the state
 * afterwards is that of trm_step with the same series, bit for bit.
 *   trm_tangent_bc_series_upload(ctx, bc_var, side, nt, host)
 *                                           host[nt][num_columns] doubles: the seed d(node value) of every node of the pair's series; nt
 *                                           must be the levels the series holds.  A step's seed is s[n1] w1 + s[n2] w2 over the two
 *                                           nodes that bracket its time, with the weights of the primal's interpolation (w2 = f,
 *                                           w1 = 1 - f; Raster: w2 = f / g; one node where the time is clamped or lands on a node).
 *                                           Zeroed by trm_tangent_open, freed by trm_tangent_close; a series nobody has seeded has zero
 *                                           seeds.  A pair without a series keeps its constant value and its trm_tangent_bc_upload seed.
 * Every operation is linear in the seeds: doubling them doubles the tangents bit for bit.  TRM_INFO_DERIVATIVE_SERIES reports the
 * series the last launch evaluated.  Refused with TRM_EUNSUPPORTED by trm_step_tangent: a series of kind Gradient, any series on the
 * generic boundary kinds, an input (forcing) series, a windowed or trimmed series, and parameter seeds together with a series unless
 * TRM_OPT_DERIVATIVE_SERIES_PARAMS = 1: then trm_tangent_param_set is accepted on a context with series, and one launch carries the node
 * seeds and the parameter seeds (bits 26 and 31), the parameter terms of every step formed at the boundary values the series gave it.
 * Errors: TRM_EINVAL without a context or an open tangent, for a pair without a series, an nt other than the series' levels or a NULL
 * pointer; trm_tangent_bc_upload on a seriesed pair (option set) returns TRM_EINVAL and names this call; TRM_ENOMEM. */
int trm_tangent_bc_series_upload(trm_ctx* ctx, int bc_var, int side, int nt, const void* host);
/* Seeds on the thermal parameters: the tangent with respect to the five conductivities and five heat capacities of trm_params
 * (SoilThermalConductivities, SoilHeatCapacities; Enzyme gives the reference these through Duplicated(integrator, dintegrator)), in the
 * order of trm_params.  Porosity, rho_soc, Lsl and the saturation are not differentiated.
 *   trm_tangent_param_set(ctx, seed)        seed[TRM_THERMAL_PARAM_COUNT] doubles, d(parameter); the same for every column.  They are
 *                                           constants like the boundary seeds: not state, nothing makes them stale, trm_tangent_open
 *                                           zeroes them.  The call allocates the four boundary seed arrays (zero) if no
 *                                           trm_tangent_bc_upload has: parameter seeds always ride with the boundary-seeded instances.
 * Once it has been called since trm_tangent_open, trm_step_tangent runs the parameter-seeded instances (TRM_INFO_LAST_PROGRAM: bits 26
 * and 31, TRM_PROGRAM_PARAMETERS), and trm_tangent_closure and the incoming closure of trm_step_tangent add the heat-capacity term
 * dT += -(T / C) dC.  The state afterwards is still that of trm_step, bit for bit; ten zero seeds give the tangents of the unseeded run.
 * Errors: TRM_EUNSUPPORTED where the tangent is; TRM_EINVAL without a context or an open tangent, for a NULL pointer, and when one of
 * the five conductivities is <= 0 (the kernels hold sqrt(k), which has no derivative there). */
enum {
    TRM_THERMAL_PARAM_K_WATER = 0, TRM_THERMAL_PARAM_K_ICE = 1, TRM_THERMAL_PARAM_K_AIR = 2, TRM_THERMAL_PARAM_K_MINERAL = 3,
    TRM_THERMAL_PARAM_K_ORGANIC = 4, TRM_THERMAL_PARAM_C_WATER = 5, TRM_THERMAL_PARAM_C_ICE = 6, TRM_THERMAL_PARAM_C_AIR = 7,
    TRM_THERMAL_PARAM_C_MINERAL = 8, TRM_THERMAL_PARAM_C_ORGANIC = 9, TRM_THERMAL_PARAM_COUNT = 10
};
int trm_tangent_param_set(trm_ctx* ctx, const double seed[TRM_THERMAL_PARAM_COUNT]);
/* Tangent records: the temperature and its tangent sampled inside the launches of trm_step_tangent, at positions and levels given once --
 * J v at the samples of a temperature record from one run, the forward twin of trm_adjoint_observe_record.
 *   trm_tangent_record_attach(ctx, npos, positions, nlevels, levels)
 *                                           positions[npos]: tangent-step counts since the attach or the last rewind, >= 0, strictly
 *                                           increasing; levels[nlevels]: rows of the host layout, inside [0, Nz), strictly increasing.
 *                                           Allocates the samples of T and of dT, [npos][nlevels][Nh] doubles each, fills both with NaN
 *                                           and sets the position counter to 0.  One record at a time.
 *   trm_tangent_record_rewind(ctx)          the counter back to 0, both arrays NaN: the next trm_step_tangent starts at position 0
 *   trm_tangent_record_detach(ctx)          drops it; trm_tangent_open and trm_tangent_close drop it as well
 *   trm_tangent_record_download(ctx, which, host) / trm_tangent_record_device_ptr(ctx, which, &dev)
 *                                           which: TRM_TANGENT_RECORD_TEMPERATURE or TRM_TANGENT_RECORD_TANGENT
 *   trm_tangent_record_info(ctx, &npos, &nlevels, &position, &bytes)
 *                                           zeros without a record; position: the counter; bytes: the device memory held for it
 * With a record attached, trm_step_tangent stores T and dT of the state after every step whose count the record lists, on the listed
 * levels, and advances the counter by the steps it ran -- across calls and across changes of dt.  Position 0 is the state the first call
 * after the attach or the rewind starts from: the T its closure forms at the stored U, and the dT of trm_tangent_closure.  A position no
 * step has reached reads NaN.  Steps behind the last position sample nothing.  The state and the three tangents are those of the run
 * without a record, bit for bit, and so is TRM_INFO_LAST_PROGRAM.  No fields other than temperature, no duplicate positions.
 * Errors: TRM_EUNSUPPORTED where the tangent is; TRM_EINVAL without a context, an open tangent or (rewind, detach, download, device_ptr)
 * an attached record, for NULL pointers, a bad list or `which`, and for a second attach; TRM_ENOMEM. */
enum { TRM_TANGENT_RECORD_TEMPERATURE = 0, TRM_TANGENT_RECORD_TANGENT = 1 };
int trm_tangent_record_attach(trm_ctx* ctx, int npos, const int32_t* positions, int nlevels, const int32_t* levels);
int trm_tangent_record_rewind(trm_ctx* ctx);
int trm_tangent_record_detach(trm_ctx* ctx);
int trm_tangent_record_download(trm_ctx* ctx, int which, void* host);
int trm_tangent_record_device_ptr(trm_ctx* ctx, int which, void** dev);
int trm_tangent_record_info(const trm_ctx* ctx, int* npos, int* nlevels, int64_t* position, int64_t* bytes);

/* ---- reverse-mode gradients of the heat-only run (the reference pulls a seed back through run! with Enzyme's Reverse mode) ---------
 * The gradient g = dL/dU_0 of L = <wU, U_n> + <wT, T_n> + <wliq, liq_n> with respect to the initial internal energy, for what the
 * tangent covers (above): the transpose of the linear map trm_step_tangent applies, one backward sweep for any number of inputs.
 * The gradient with respect to the boundary values comes from trm_adjoint_bc_open, with respect to the thermal parameters from
 * trm_adjoint_param_open (both below); every other parameter is a constant.
 *   trm_adjoint_open(ctx, capacity_steps)   allocates the cotangent fields of U, T, liq (zero) and a tape of capacity_steps slots; one
 *                                           slot is Nh x Nzp x 8 bytes (the internal energy before a step).  Opening again starts a
 *                                           fresh tape and zeroes the cotangents.
 *   trm_adjoint_close(ctx)                  frees them
 *   trm_adjoint_upload(ctx, which, host)    the cotangents wU / wT / wliq of the final U / T / liq, host layout [Nz][Nh]
 *   trm_adjoint_download(ctx, which, host)  after trm_adjoint_backward: TRM_ADJOINT_INTERNAL_ENERGY is g, the other two are zero
 *                                           (folded in)
 *   trm_adjoint_device_ptr(ctx, which, &dev, &pitch)
 *                                           device layout as trm_field_device_ptr
 *   trm_adjoint_tape(ctx, &recorded, &capacity)
 *   trm_step_record(ctx, dt, nsteps)        nsteps ForwardEuler steps, the internal energy before each stored in the next tape slot, dt
 *                                           kept per step on the host.  The state afterwards -- every field, the status word, the clock
 *                                           -- is that of trm_step(ctx, dt, nsteps, 1), bit for bit, in the launches trm_step would
 *                                           issue on the multi-step program.  The stored T and liq are taken to be the closure of the
 *                                           stored U, as for trm_step_tangent.
 *   trm_adjoint_backward(ctx)               pulls the cotangents back through every taped step, newest first, and empties the tape:
 *                                           one launch per block of up to TRM_OPT_STEPS_PER_LAUNCH taped steps that share one dt.  With
 *                                           an empty tape it is the closure's transpose alone: g = wU + a wT + b wliq, a and b the
 *                                           slopes dT/dU and dliq/dU of trm_tangent_closure at the stored state.
 * TRM_INFO_LAST_PROGRAM of both is TRM_PROGRAM_COLUMN_ADJOINT: bit 25 as for the tangent family (Gradient halos on temperature, the
 * generic halo form), bit 26 set for a backward launch and clear for a record launch.
 * Errors: TRM_EINVAL without a context or an open adjoint, for a bad `which`, capacity_steps < 1, nsteps < 0, and for a trm_step_record
 * of more steps than the tape has slots left (nothing is stepped; state and tape are unchanged).  TRM_EUNSUPPORTED for what the tangent
 * refuses.  TRM_ENOMEM when the tape does not fit.  TRM_ESTALE from trm_adjoint_backward and trm_step_record when anything but
 * trm_step_record has changed the state since the first taped step (the calls listed for the tangent, and trm_step_tangent), or
 * trm_set_bc / trm_set_bc_series a boundary condition: the sweep reads the boundary values the context holds when it runs, which must be
 * the ones the record ran with.  Nothing is stepped or pulled back then.  trm_adjoint_open, or a trm_adjoint_backward that succeeded,
 * starts a fresh tape.  trm_step_record is a state-changing call for an open tangent.  A tangent and an adjoint may be open at once.
 *
 * The checkpointed tape keeps the internal energy before every `interval`-th step alone; trm_adjoint_backward forms the states in
 * between again, inside its launches, by re-running the recorded steps bit for bit.  The gradient is the per-step tape's bit for bit;
 * the tape is `interval` times smaller, and the sweep runs interval - 1 of every interval steps a second time.
 *   trm_adjoint_open_checkpointed(ctx, capacity_slots, interval)
 *                                           allocates the cotangent fields as trm_adjoint_open does and capacity_slots checkpoint
 *                                           slots of Nh x Nzp x 8 bytes.  interval is 1 ... TRM_ADJOINT_MAX_INTERVAL;
 *                                           TRM_ADJOINT_DEFAULT_INTERVAL is the largest that costs the sweep no occupancy.  Opening
 *                                           in either mode replaces an open adjoint of the other mode.
 *   trm_adjoint_checkpoints(ctx, &interval, &slots_used, &slots_capacity)
 *                                           interval is 0 for a per-step tape, whose slots are steps
 * Every other call above works on either tape.  Segments: the taped steps are split into segments of up to `interval` steps under
 * one dt, each with its first state in one slot.  A trm_step_record call opens a new segment -- and takes a slot -- when the tape
 * is empty, when the open segment holds `interval` steps, or when its dt differs from the call's.  The call works out the slots it
 * needs before it launches anything: TRM_EINVAL with nothing stepped if they do not fit.  Its launches are still those of trm_step, so
 * one may straddle segment boundaries.  trm_adjoint_backward issues one launch per segment, newest first.  trm_adjoint_tape reports
 * the steps taped and capacity_slots x interval.  TRM_INFO_LAST_PROGRAM carries bit 27 for the launches of a checkpointed tape.
 * Errors as above; TRM_EINVAL for capacity_slots < 1 or an interval out of range.
 *
 * Heat + Richards, with TRM_OPT_DERIVATIVE_RICHARDS_ADJOINT set: trm_adjoint_open, _close, _upload, _download, _device_ptr, trm_adjoint_tape,
 * trm_step_record and trm_adjoint_backward accept what the Richards tangent covers (fp64, Nz <= 64, the branch-free boundary kinds, constant
 * boundary values, no series, no vwc_forcing field).  L = <wU, U_n> + <wsat, sat_n> + <wT, T_n> + <wliq, liq_n> + <wpsi, psi_n>;
 * trm_adjoint_open allocates five cotangent fields there, all five uploadable (on a NoFlow context the indices 3 and 4 are a bad
 * argument), and a slot of the tape is 2 x Nh x Nzp x 8 bytes: the internal energy and the saturation before a step.  After
 * trm_adjoint_backward TRM_ADJOINT_INTERNAL_ENERGY holds dL/dU_0, TRM_ADJOINT_SATURATION holds dL/dsat_0 and the other three are zero: the
 * transpose of the linear map trm_step_tangent applies there, branch for branch.  trm_step_record leaves what trm_step(ctx, dt, nsteps, 1)
 * leaves, bit for bit; the stored T, liq and psi are taken to be the closures of the stored U and sat.  TRM_INFO_LAST_PROGRAM of both calls is
 * TRM_PROGRAM_COLUMN_ADJOINT_RICHARDS.  The staleness rules are the ones above (trm_upload of the saturation makes a tape that holds steps
 * stale).  The checkpointed tape, boundary, parameter and series gradients, observations and records refuse a Richards context with
 * TRM_EUNSUPPORTED "on a Richards context: final-state cotangents on a per-step tape only".  (The hydraulic parameters:
 * TRM_OPT_DERIVATIVE_RICHARDS_PARAMS, beside trm_adjoint_param_open below.  Soil-moisture records: TRM_OPT_DERIVATIVE_RICHARDS_RECORD,
 * beside trm_adjoint_observe_record below.) */
enum { TRM_ADJOINT_INTERNAL_ENERGY = 0, TRM_ADJOINT_TEMPERATURE = 1, TRM_ADJOINT_LIQUID_WATER_FRACTION = 2,
       TRM_ADJOINT_SATURATION = 3,      /* Richards contexts only: the cotangent of saturation_water_ice, and dL/dsat_0 after a sweep */
       TRM_ADJOINT_PRESSURE_HEAD = 4 }; /* Richards contexts only: the cotangent of pressure_head */
int trm_adjoint_open(trm_ctx* ctx, int capacity_steps);
int trm_adjoint_close(trm_ctx* ctx);
int trm_adjoint_upload(trm_ctx* ctx, int which, const void* host);
int trm_adjoint_download(trm_ctx* ctx, int which, void* host);
int trm_adjoint_device_ptr(trm_ctx* ctx, int which, void** dev, int64_t* pitch_elems);
int trm_adjoint_tape(const trm_ctx* ctx, int* recorded, int* capacity);
#define TRM_ADJOINT_MAX_INTERVAL 32      /* 64 KiB of LDS per workgroup in the backward launch: 2 KiB per step of a segment */
#define TRM_ADJOINT_DEFAULT_INTERVAL 16
int trm_adjoint_open_checkpointed(trm_ctx* ctx, int capacity_slots, int interval);
int trm_adjoint_checkpoints(const trm_ctx* ctx, int* interval, int* slots_used, int* slots_capacity);
int trm_step_record(trm_ctx* ctx, double dt, int nsteps);
int trm_adjoint_backward(trm_ctx* ctx);
/* Boundary gradients: dL/d(value) of the boundary values that drove the taped steps -- the surface temperature, a temperature gradient,
 * the ground or geothermal heat flux -- from the same sweep, for the pairs trm_tangent_bc_upload seeds.
 *   trm_adjoint_bc_open(ctx)                allocates four accumulators of num_columns doubles, zero; from then on trm_adjoint_backward
 *                                           runs the accumulating instances (TRM_INFO_LAST_PROGRAM: bit 30) on either tape.
 *                                           trm_adjoint_open keeps them (zeroed); trm_adjoint_close frees them.
 *   trm_adjoint_bc_download(ctx, bc_var, side, host)
 *                                           host[num_columns] doubles.  After a trm_adjoint_backward that succeeded: dL/d(value) of the
 *                                           pair of that sweep -- the sum over all taped steps, the value being constant over the tape
 *                                           (a trm_set_bc in between makes the tape stale) -- and exact zeros for a pair whose kind
 *                                           reads no value.  After a sweep that failed the content is unspecified.
 *   trm_adjoint_bc_device_ptr(ctx, bc_var, side, &dev)
 *                                           the accumulator on the device, num_columns contiguous doubles
 * The sum runs over the taped steps newest first, one step at a time in a register of the column's edge lane, and is carried from launch
 * to launch: it does not depend on TRM_OPT_STEPS_PER_LAUNCH or on the checkpoint interval, the checkpointed tape gives the per-step
 * tape's bits, and g = dL/dU_0 is bit for bit what the sweep without boundary gradients gives.
 * Errors: TRM_EINVAL without a context or an open adjoint, for _download / _device_ptr before trm_adjoint_bc_open, for a bc_var other
 * than TRM_BCV_TEMPERATURE / TRM_BCV_INTERNAL_ENERGY, a side other than 0 / 1, or a NULL pointer; TRM_ENOMEM. */
int trm_adjoint_bc_open(trm_ctx* ctx);
int trm_adjoint_bc_download(trm_ctx* ctx, int bc_var, int side, void* host);
int trm_adjoint_bc_device_ptr(trm_ctx* ctx, int bc_var, int side, void** dev);
/* Gradients through a boundary time series (TRM_OPT_DERIVATIVE_SERIES = 1): dL/d(node value) of every node of the series that drive the
 * run, from the same sweep.  With the option set, trm_step_record accepts the boundary series trm_step_tangent accepts, evaluates them
 * in the launch and keeps the rows (bracketing nodes and fractions) of every taped step; trm_adjoint_backward runs the accumulating
 * instances (it opens the four per-column accumulators, zero, if nobody has) with those rows, never a clock of its own.
 *   trm_adjoint_bc_series_download(ctx, bc_var, side, nt, host)
 *                                           host[nt][num_columns] doubles.  After a trm_adjoint_backward that succeeded: the node
 *                                           gradients of the pair's series of that sweep -- a step adds w1 term to node n1 and w2 term to
 *                                           node n2 of its bracket -- and exact zeros for nodes no taped step touched (and before the
 *                                           first sweep).  nt must be the levels the series holds.
 *   trm_adjoint_bc_series_device_ptr(ctx, bc_var, side, &dev, &nt)
 *                                           the accumulator on the device, nt x num_columns contiguous doubles
 * Each (node, column) sum runs over the taped steps newest first and always continues from the stored value: it does not depend on
 * TRM_OPT_STEPS_PER_LAUNCH, on how the trm_step_record calls were split or on the checkpoint interval.  A pair without a series keeps
 * its per-column gradient (trm_adjoint_bc_download) in the same sweep.  trm_set_bc_series, trm_clear_series, trm_series_append,
 * trm_series_window and trm_series_trim_before make a tape that holds steps stale.
 * Errors: TRM_EINVAL without a context or an open adjoint, for a pair without a series, an nt other than the series' levels or a NULL
 * pointer; trm_adjoint_bc_download / _device_ptr on a seriesed pair (option set) return TRM_EINVAL and name these calls; TRM_EUNSUPPORTED
 * from trm_step_record / trm_adjoint_backward as for trm_step_tangent, and for an open parameter gradient together with a series unless
 * TRM_OPT_DERIVATIVE_SERIES_PARAMS = 1: then trm_adjoint_param_open is accepted on a context with series and one sweep delivers g, the
 * node gradients, the per-column gradients of the pairs without a series and the ten parameter gradients (bits 30 and 31), on either
 * tape; g and the node gradients are bit for bit those of the sweep without the parameter gradient. */
int trm_adjoint_bc_series_download(trm_ctx* ctx, int bc_var, int side, int nt, void* host);
int trm_adjoint_bc_series_device_ptr(trm_ctx* ctx, int bc_var, int side, void** dev, int* nt);
/* Parameter gradients: dL/d(parameter) of the ten thermal parameters trm_tangent_param_set seeds (TRM_THERMAL_PARAM_*), per column, from
 * the same sweep.
 *   trm_adjoint_param_open(ctx)             allocates eight per-cell accumulators (Nh x Nzp doubles each) and the result, zero, and
 *                                           implies trm_adjoint_bc_open: from then on trm_adjoint_backward runs the instances that
 *                                           accumulate both (TRM_INFO_LAST_PROGRAM: bits 30 and 31) on either tape, and ends with one
 *                                           reduction launch.  trm_adjoint_open keeps them (zeroed); trm_adjoint_close frees them.
 *   trm_adjoint_param_download(ctx, which, host)
 *                                           host[num_columns] doubles.  After a trm_adjoint_backward that succeeded: dL/d(parameter
 *                                           `which`) of each column's share of L (the parameter is one number for all columns: their
 *                                           sum is the gradient of the scalar L).  After a sweep that failed the content is unspecified.
 *   trm_adjoint_param_device_ptr(ctx, which, &dev)
 *                                           the same on the device, num_columns contiguous doubles
 * Every lane sums its own cell's terms over the taped steps newest first, carried from launch to launch; the reduction adds a column's
 * cells from the bottom up.  The sums do not depend on TRM_OPT_STEPS_PER_LAUNCH or on the checkpoint interval, and g = dL/dU_0 and the
 * boundary gradients are bit for bit what the sweep without parameter gradients gives.
 * Errors: TRM_EUNSUPPORTED where the adjoint is; TRM_EINVAL without a context or an open adjoint, for _download / _device_ptr before
 * trm_adjoint_param_open, a `which` outside 0 ... TRM_THERMAL_PARAM_COUNT - 1, a NULL pointer, and for trm_adjoint_param_open when one
 * of the five conductivities is <= 0; TRM_ENOMEM.
 *
 * Heat + Richards, with TRM_OPT_DERIVATIVE_RICHARDS_ADJOINT and TRM_OPT_DERIVATIVE_RICHARDS_PARAMS both set: the three calls serve the seven
 * hydraulic parameters of trm_params (TRM_HYDRAULIC_PARAM_*: K_sat, theta_res, bc_psi_s, bc_lambda, vg_alpha, vg_n, impedance) on what the
 * per-step tape covers there (fp64, ForwardEuler, Nz <= 64, the branch-free boundary kinds with constant values, no series, no
 * vwc_forcing field).
 *   trm_adjoint_param_open(ctx)             on a Richards context with an open per-step adjoint: allocates seven per-cell accumulators
 *                                           (Nh x Nzp doubles each) and the per-column results, zero.  It does NOT imply
 *                                           trm_adjoint_bc_open, which stays refused there.  From then on trm_adjoint_backward runs the
 *                                           accumulating instances (TRM_INFO_LAST_PROGRAM: family 17 with bit 31) and ends with one
 *                                           reduction launch.  trm_adjoint_open keeps them (zeroed); trm_adjoint_close frees them.
 *   trm_adjoint_param_download(ctx, which, host) / trm_adjoint_param_device_ptr(ctx, which, &dev)
 *                                           `which` one of the seven TRM_HYDRAULIC_PARAM_* ids, which continue the thermal ids (one id
 *                                           space); num_columns doubles: each column's share of dL/d(parameter).
 * The gradient is the sum over the taped steps and the cells of Kcbar dKc/dp + psibar dpsi/dp -- Kcbar and psibar the cotangents of a
 * cell's hydraulic conductivity and pressure head in the step's transpose -- plus wpsi dpsi/dp at the stored final state.  A parameter
 * the context's hydraulics never read gives exact zeros (vg_alpha, vg_n, impedance under Brooks-Corey with the linear conductivity;
 * bc_psi_s, bc_lambda under van Genuchten).  d(x^a)/da = x^a ln x, and 0 where x^a is 0; a zero cotangent in front of a slope gives 0
 * whatever the slope, so zero cotangents give exactly zero gradients and scaling them by a power of two scales the gradients bit for bit;
 * a cell flagged as an illegal composition gives NaN.  The sums do not depend on TRM_OPT_STEPS_PER_LAUNCH or on how the trm_step_record
 * calls were split, and dL/dU_0 and dL/dsat_0 are bit for bit those of the sweep without the parameter gradient.
 * Errors: with either option at 0 the calls answer a Richards context as above.  TRM_EINVAL "bad argument" for the thermal ids 0 ... 9
 * on a Richards context, for the hydraulic ids on a NoFlow context, and for a NULL pointer; TRM_EINVAL without an open adjoint or before
 * trm_adjoint_param_open; TRM_ENOMEM.  Forward-mode seeds on these parameters, and porosity, rho_soc and vwc_forcing as parameters, are
 * not provided. */
enum {
    TRM_HYDRAULIC_PARAM_K_SAT = 10,     /* = TRM_THERMAL_PARAM_COUNT: one id space with the thermal ids */
    TRM_HYDRAULIC_PARAM_THETA_RES = 11, TRM_HYDRAULIC_PARAM_BC_PSI_S = 12, TRM_HYDRAULIC_PARAM_BC_LAMBDA = 13,
    TRM_HYDRAULIC_PARAM_VG_ALPHA = 14, TRM_HYDRAULIC_PARAM_VG_N = 15, TRM_HYDRAULIC_PARAM_IMPEDANCE = 16,
    TRM_HYDRAULIC_PARAM_COUNT = 7
};
int trm_adjoint_param_open(trm_ctx* ctx);
int trm_adjoint_param_download(trm_ctx* ctx, int which, void* host);
int trm_adjoint_param_device_ptr(trm_ctx* ctx, int which, void** dev);
/* Adjoint observations: losses that read the run at taped positions and not at its end alone -- a borehole record, temperatures at a
 * few depths at many times (the reference differentiates such a loss by pulling a seed back through run! once per observation time;
 * here the cotangents enter one sweep).  An observation belongs to the taped position p at which it is registered, the number of steps
 * on the tape, 0 <= p <= n: it is registered between trm_step_record calls and refers to the state the context holds then, U_p and its
 * closure.  `levels`: nlevels rows of the host layout of trm_download (row 0 = bottom layer), strictly increasing.
 *   trm_adjoint_observe(ctx, which, nlevels, levels, host)
 *                                           linear: host[nlevels][num_columns] doubles, the cotangent w of U, T or liq (which:
 *                                           TRM_ADJOINT_*) on those levels; adds <w, X_p[levels]> to L.  Stands in for one more seed
 *                                           and sweep of the reference.
 *   trm_adjoint_observe_misfit(ctx, nlevels, levels, observed, weight)
 *                                           misfit: observed[nlevels][num_columns] temperatures T_obs and weights w >= 0 of the same
 *                                           shape (NULL: 1); adds 1/2 w (T_p - T_obs)^2 per cell to the column's loss at once (one small
 *                                           launch) and w (T_p - T_obs) to the cotangent of T_p in the sweep.  A NaN in `observed` is a
 *                                           gap in the logger's record: it contributes nothing, exactly as a weight 0.  Stands in for
 *                                           the loss function a calibration differentiates with Enzyme.
 *   trm_adjoint_misfit_download(ctx, host)  host[num_columns] doubles: each column's share of the misfit so far (zeros without one)
 *   trm_adjoint_misfit_device_ptr(ctx, &dev) the same on the device, num_columns contiguous doubles
 *   trm_adjoint_observations(ctx, &count, &bytes)
 *                                           observations registered and the device memory they hold: an observation keeps what the
 *                                           caller gave, nlevels x num_columns x 8 bytes per array plus 4 bytes per level, never a field
 * trm_adjoint_backward pulls the final cotangents of trm_adjoint_upload back as before and, when it has pulled back every step >= p,
 * adds wU + a_p wT + b_p wliq on the observed cells to lam, a_p and b_p the closure slopes at U_p; with a parameter gradient open wT
 * also goes through the heat capacity of that closure onto the parameter sums.  U_p is tape slot p; on the checkpointed tape an
 * observation closes the open segment, so that the next taped step opens one -- and takes a slot, which trm_step_record counts before
 * it launches anything -- and U_p is its checkpoint; for p = n it is the state itself.  The sweep splits at observed positions: on the
 * per-step tape a block also ends there.  Order of every sum, whatever the split:
 *   lam of a cell         ... the steps > p - 1, then the observations of p in registration order, then step p - 1 ...; those of p = n
 *                         come first, in front of the fold of the final wT and wliq
 *   parameter sums        the fold, the steps of the sweep's first launch, the observations of p = n (the launch that folds starts its
 *                         sums from 0, so they follow it), then as lam: the observations of p in front of step p - 1, those of p = 0 last
 *   boundary, node sums   accumulated from lam alone: nothing new
 *   misfit of a column    the observations in registration order, the levels of each in list order
 * One lane owns a cell in every one of them: no atomics.  Scaling every cotangent and weight by a power of two scales every gradient bit
 * for bit; with every cotangent zero the sweep gives the values of the sweep without observations; dL/dU_0 of the checkpointed tape is
 * the per-step tape's.  With no observation registered every call issues the launches it issued before and gives the same bits.
 * trm_adjoint_open*, trm_adjoint_close and a trm_adjoint_backward that succeeded drop all observations and zero the misfit; a sweep that
 * failed leaves the tape stale.  Observations do not touch the state, the clock or the status word, make no tangent stale, and their
 * launches do not write TRM_INFO_LAST_PROGRAM: after a sweep it is that of the sweep's last launch.
 * Errors: TRM_EINVAL without a context or an open adjoint, for a bad `which`, nlevels < 1, a level outside 0 ... Nz-1 or out of order,
 * a NULL levels / host / observed, a negative or NaN weight; TRM_ESTALE on a stale tape; TRM_ENOMEM. */
int trm_adjoint_observe(trm_ctx* ctx, int which, int nlevels, const int32_t* levels, const void* host);
int trm_adjoint_observe_misfit(trm_ctx* ctx, int nlevels, const int32_t* levels, const void* observed, const void* weight);
int trm_adjoint_misfit_download(trm_ctx* ctx, void* host);
int trm_adjoint_misfit_device_ptr(trm_ctx* ctx, void** dev);
int trm_adjoint_observations(const trm_ctx* ctx, int* count, int64_t* bytes);

/* ---- Attached records: a temperature record read INSIDE the backward launches ---------------------------------------------------
 * The calls above make every observed position a launch boundary (and, checkpointed, a slot), and a sweep drops them.  A record that
 * is ATTACHED to the open adjoint is neither: it is given once, survives sweeps, and the backward kernels read it themselves.
 *   positions[npos]                 taped-step counts, >= 0, strictly increasing: position p is the state after p taped steps of the
 *                                   current tape (0: the state at the first trm_step_record)
 *   levels[nlevels]                 rows of the host layout, strictly increasing (as trm_adjoint_observe_misfit)
 *   observed[npos][nlevels][num_columns], weight of the same shape (NULL: 1)
 * L = sum_k sum_j 1/2 w (T_{p_k}[level_j] - T_obs)^2 per column; a NaN in `observed` or a weight 0 contributes nothing.  With a record
 * attached trm_adjoint_backward gives the gradient of L plus the final cotangents with respect to everything the open rides cover:
 * position p < n is injected by the launch that pulls back step p, right behind that step (steps > p - 1, the observation of p, step
 * p - 1); position n enters with the fold.  No position ends a launch, none takes a checkpoint slot: a checkpointed tape of n steps
 * under one dt takes ceil(n / K) slots whatever the record.
 *   trm_adjoint_observe_record(ctx, npos, positions, nlevels, levels, observed, weight)
 *                                           host arrays, copied to the device once
 *   trm_adjoint_observe_record_device(ctx, npos, positions, nlevels, levels, d_observed, d_weight)
 *                                           device arrays of the context's device, kept by pointer: they stay the caller's and must
 *                                           outlive the attachment.  The library cannot read them here, so the weights are NOT
 *                                           validated: the kernels treat a weight that is not > 0 (negative, NaN) as 0.
 *   trm_adjoint_record_detach(ctx)          drops the record
 *   trm_adjoint_record_residual_download(ctx, host)   host[npos][nlevels][num_columns]: r = T_p - T_obs of the last sweep, +0 for a gap
 *   trm_adjoint_record_residual_device_ptr(ctx, &dev) the same on the device
 *   trm_adjoint_record_misfit_download(ctx, host)     host[num_columns]: sum of 1/2 w r^2 per column, positions ascending, levels in
 *                                                     list order, one term at a time (not the buffer of trm_adjoint_misfit_download)
 *   trm_adjoint_record_info(ctx, &npos, &nlevels, &bytes)  zeros without a record; bytes: the device memory the library holds for it
 * Residuals and misfit stay readable until the next sweep, a detach or trm_adjoint_close.  The record is dropped by
 * trm_adjoint_record_detach, trm_adjoint_open* (a new tape) and trm_adjoint_close; trm_adjoint_backward keeps it, successful or not, so a
 * loop of "upload U_0, trm_step_record, trm_adjoint_backward" never sends it again.  Attaching with steps on the tape is allowed:
 * positions count from the tape's start.  The two paths do not mix: while a record is attached trm_adjoint_observe* are refused, and
 * attaching is refused while per-position observations are registered.  These calls touch neither state, clock nor status, make no
 * tangent stale, and TRM_INFO_LAST_PROGRAM of a record-reading launch is that of the same launch without a record.
 * Errors: TRM_EINVAL without a context or an open adjoint, npos < 1, nlevels < 1, NULL pointers, positions negative or not strictly
 * increasing, a level outside 0 ... Nz-1 or out of order, a negative or NaN host weight, a second attach without a detach, the mixing
 * rules, a download before a sweep has run with this record; trm_adjoint_backward: TRM_EINVAL, before anything is launched and with the
 * tape left usable, for a record with a position behind the taped steps; TRM_ENOMEM.
 *
 * Heat + Richards, with TRM_OPT_DERIVATIVE_RICHARDS_ADJOINT and TRM_OPT_DERIVATIVE_RICHARDS_RECORD both set: the seven calls accept a
 * Richards context with an open per-step adjoint, and the record observes saturation_water_ice -- what a soil-moisture probe logs.
 * The arrays, the lifetime, the staleness rules, the validation of an attach and the refusal of a record longer than the tape are the
 * ones above, with `observed` holding saturations: L = sum_k sum_j 1/2 w (sat_{p_k}[level_j] - sat_obs)^2 per column, residuals
 * r = sat_p - sat_obs (+0 for a gap), the misfit summed as above.  trm_adjoint_backward gives the gradient of L plus the final
 * cotangents with respect to the initial internal energy and saturation and, with the hydraulic-parameter gradients open
 * (TRM_OPT_DERIVATIVE_RICHARDS_PARAMS), the seven hydraulic parameters, from one sweep.  Saturation is a state variable: the sample
 * of position p is added to the saturation cotangent itself, right behind the pull-back of step p (position n: in front of the fold),
 * and reaches the parameters through the steps below it.  Per cell the order is the sample of n, the fold, steps > p, the sample of
 * p, step p - 1, ...: gradients, residuals and misfit do not depend on TRM_OPT_STEPS_PER_LAUNCH or on how the trm_step_record calls
 * were split.  A gap adds nothing, not even the sign of a zero: a record of NaNs or of weights 0 gives the sweep without a record,
 * bit for bit.  Temperature, liquid-water or pressure-head records, the per-position calls and the checkpointed tape stay refused on
 * a Richards context.  With either option at 0 the seven calls answer a Richards context as before. */
int trm_adjoint_observe_record(trm_ctx* ctx, int npos, const int32_t* positions, int nlevels, const int32_t* levels, const void* observed, const void* weight);
int trm_adjoint_observe_record_device(trm_ctx* ctx, int npos, const int32_t* positions, int nlevels, const int32_t* levels, const void* d_observed, const void* d_weight);
int trm_adjoint_record_detach(trm_ctx* ctx);
int trm_adjoint_record_residual_download(trm_ctx* ctx, void* host);
int trm_adjoint_record_residual_device_ptr(trm_ctx* ctx, void** dev);
int trm_adjoint_record_misfit_download(trm_ctx* ctx, void* host);
int trm_adjoint_record_info(const trm_ctx* ctx, int* npos, int* nlevels, int64_t* bytes);

int trm_clock(const trm_ctx* ctx, double* time, int64_t* iteration);
int trm_set_clock(trm_ctx* ctx, double time, int64_t iteration);

/* Local (this device's columns) reduction of a field.  SUM/MIN/MAX/HASNAN give one value per row in
 * out[rows]; VOLUME_INTEGRAL_Z gives one value (sum over columns of sum_k f*dz) and takes a cell-centred 3-D field (Nz rows)
 * only.  trm_reduce_global (below) combines the devices' results.
 * MIN / MAX are Julia's Base.minimum / maximum: a NaN anywhere in a row gives NaN (HASNAN is 1 for that row, SUM and
 * VOLUME_INTEGRAL_Z are NaN by arithmetic), and where zeros of both signs tie, MIN is -0.0 and MAX is +0.0, whatever the order of
 * the fold (minimum([0.0, -0.0]) === -0.0, maximum([-0.0, 0.0]) === 0.0).  Infinities are ordinary values: HASNAN of a row of
 * infinities is 0, the SUM of +Inf and -Inf is NaN.
 * The 3-D vegetation fields TRM_FIELD_PLANT_AVAILABLE_WATER and TRM_FIELD_ROOT_FRACTION are allocated by trm_set_vegetation: before it
 * trm_reduce (and with it trm_reduce_global / trm_reduce_global_all) fails with TRM_EINVAL ("the field exists only after
 * trm_set_vegetation") before anything is launched, as trm_upload / trm_download do. */
int trm_reduce(trm_ctx* ctx, int field, int op, double* out);
int trm_status(trm_ctx* ctx, uint32_t* flags);
/* Sets the status word: a restart puts back the flags its checkpoint carried (the word is sticky: steps only OR into it), so a run
 * that had produced a NaN before the checkpoint does not report a clean status after the restart; 0 clears it. */
int trm_set_status(trm_ctx* ctx, uint32_t flags);

/* ---- multi-device diagnostics ----------------------------------------------------------------------------------------
 * The global grid of laterally independent columns is block-sharded over the devices of a node, one context (and one
 * host process or thread) per device; the step path has NO collective.  Diagnostics that span the shards -- the
 * reference's `sum(field)`, `minimum`, `maximum`, `any(isnan, ...)` on a whole Field, the CPU-side @assert scans -- are
 * combined inside the library with one RCCL all-reduce of <= 2 * (Nz + 1) doubles on the context's side stream (xGMI:
 * latency-bound, link bandwidth irrelevant), so a host in any language gets global values without a communication
 * layer of its own.  RCCL is opened lazily (dlopen) by the first of these calls.
 *   rank 0:      trm_comm_unique_id(id);  broadcast the 128 bytes to the other ranks by any means (MPI, a file, a pipe)
 *   every rank:  trm_comm_init(ctx, rank, world, id);    -- collective: returns once every rank has called it
 *                trm_reduce_global / trm_status_global   -- collective, same arguments on every rank
 * trm_reduce_global gives what trm_reduce would give on the unsharded grid: SUM / VOLUME_INTEGRAL_Z sums over ranks
 * (in RCCL's deterministic ring order), MIN / MAX / HASNAN exactly, a NaN on any rank propagating into MIN / MAX.  The zero-sign
 * rule of trm_reduce holds across the shards where the library folds them itself (trm_reduce_global_all without communicators); the
 * sign of a zero that RCCL's min / max pick between ranks is RCCL's. */
int trm_comm_unique_id(void* id128);
int trm_comm_init(trm_ctx* ctx, int rank, int world_size, const void* id128);
int trm_comm_destroy(trm_ctx* ctx);
/* *world_size = 0 while the context has no communicator */
int trm_comm_info(const trm_ctx* ctx, int* rank, int* world_size);
int trm_reduce_global(trm_ctx* ctx, int field, int op, double* out);
int trm_status_global(trm_ctx* ctx, uint32_t* flags);
/* ---- ONE host process (thread) driving n contexts, one per device -- the reference's host is one Julia process
 * (column_grid.jl:32, model_integrator.jl:72-88).  trm_comm_init is a blocking collective: a single thread that holds every
 * context would wait in the first call for ranks it has not reached yet.  The *_all forms take all contexts at once:
 *   trm_comm_init_all     one RCCL communicator per context, created inside one ncclGroupStart / ncclGroupEnd; contexts must
 *                         sit on distinct devices (RCCL refuses two ranks per device); rank = position in `ctxs`
 *   trm_step_all          trm_step on every context without waiting in between (each on its own stream), then one wait for
 *                         all of them unless the contexts are asynchronous (TRM_OPT_ASYNC); trm_synchronize_all waits
 *   trm_reduce_global_all / trm_status_global_all
 *                         what trm_reduce_global / trm_status_global give, for all contexts from one thread: the per-device
 *                         partial results are combined by grouped RCCL all-reduces when the contexts carry communicators
 *                         (trm_comm_init_all), and on the host otherwise (one process needs no wire for <= 2 (Nz + 1)
 *                         doubles per device): same values, `out` written once. */
int trm_comm_init_all(trm_ctx** ctxs, int n);
int trm_step_all(trm_ctx** ctxs, int n, double dt, int nsteps, int finalize);
int trm_step_heun_all(trm_ctx** ctxs, int n, double dt, int nsteps, int finalize);
int trm_synchronize_all(trm_ctx** ctxs, int n);
int trm_reduce_global_all(trm_ctx** ctxs, int n, int field, int op, double* out);
int trm_status_global_all(trm_ctx** ctxs, int n, uint32_t* flags);

int trm_set_option(trm_ctx* ctx, int option, int value);
int trm_get_option(const trm_ctx* ctx, int option, int* value);
/* Adopt an external hipStream_t (e.g. torch's current stream); NULL restores the context's own. */
int trm_set_stream(trm_ctx* ctx, void* hip_stream);
int trm_synchronize(trm_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* TERRARIUM_HIP_H */
