// trm_host.hpp -- host side shared by the translation units of libterrarium_hip.so: the context, the launch arguments and
// the launch policies (which kernel instance a context takes).  The kernel instantiations are spread over the trm_launch_*.hip
// files (one family per file, compiled in parallel); the C ABI is spread over the trm_*_api.hip files: the context (trm_context_api.hip),
// field I/O (trm_field_io_api.hip), time series (trm_series_api.hip), the step sequences (trm_step_api.hip), the communicators
// (trm_comm_api.hip) and the derivatives (trm_derivative_api.hip); what they share is declared here.  Nothing here is part of the ABI.
#pragma once
#include "../../include/terrarium_hip.h"
#include "trm_kernels.hpp"
#include "trm_column.hpp"
#include "trm_vegetation.hpp"
#include "trm_dispatch.hpp"

#include <rccl/rccl.h>   // types only: the library is opened lazily by trm_comm_init (no link-time dependency)

#include <cmath>
#include <limits>
#include <type_traits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>
#include <vector>

struct FieldSet {
    void* f[TRM_FIELD_COUNT];
    void* kf_top;  // top face (face Nz) of the hydraulic_conductivity Face field, [Nh]
    void* raw[TRM_FIELD_COUNT];   // the allocations behind f[] (f = raw + the field's skew, see alloc_fields)
};

// The position table of a record, the adjoint's (trm_ctx::rec) or the tangent's (trm_ctx::trec): what the caller gave -- `positions` (step
// counts) and `levels` (rows of the host layout), both strictly increasing; npos == 0: none attached -- and the int32 tables the kernels
// index: row_of_level[Nz], then row_of_position[entries] (entries == 0: not built).  `host`: the staging copy, alive while its upload is
// in flight; `d_tables`: the device copy.  The functions are record_table_* (below).
struct RecordTable {
    std::vector<int> positions, levels;
    int npos = 0, nlevels = 0;
    std::vector<int32_t> host;
    double* d_tables = nullptr;
    int entries = 0;
};

struct trm_ctx {
    int precision = TRM_F64;
    long Nh = 0;
    int Nz = 0, Nzp = 0, device = 0;  // Nzp: level pitch of the z-fastest device layout
    size_t esize = 8;
    trm_params params;
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    FieldSet state{}, stage{}, saved{};
    bool has_stage = false, has_saved = false;
    double saved_time = 0.0;
    int64_t saved_iteration = 0;
    uint32_t saved_status = 0;
    bool saved_tend_valid = true;
    void* bc_value[TRM_BCV_COUNT][2] = {};
    int bc_kind[TRM_BCV_COUNT][2] = {};
    // A Gradient condition whose values the library KNOWS to be +0 everywhere (set through trm_set_bc from host values, the device
    // buffer never handed out since): at the BOTTOM its halo, edge + (+0) * (-dz) = edge + (-0), IS the edge value bit for bit -- the
    // halo the branch-free programs form where no condition is set.  The reference's FreeDrainage() (GradientBoundaryCondition(0) on
    // the pressure head, soil_model_bcs.jl:40) is that case, and need not take the generic-boundary kernels (Policy::generic_bcs).
    bool bc_zero_gradient[TRM_BCV_COUNT][2] = {};
    void *d_zC = nullptr, *d_zF = nullptr, *d_dzc = nullptr, *d_rdzc = nullptr, *d_rdzf = nullptr, *d_psiz = nullptr, *d_lvl = nullptr;
    void* d_rootf = nullptr;   // static root fraction per level [Nz] (root_distribution.jl:45-63)
    std::vector<double> h_zF, h_zC, h_dzc, h_dzf;  // as derived in NF, widened
    double dzf_bot = 0, dzf_top = 0, dzc_bot = 0, dzc_top = 0, Az = 1;
    uint32_t* d_status = nullptr;
    // time series input sources: whole series resident on the device, evaluated at the clock every step
    struct Series {
        bool is_bc = false;
        int field = 0, var = 0, side = 0, indexing = 0;
        std::vector<double> times;  // the time levels currently held, oldest first
        void* d_values = nullptr;   // [cap][Nh]: a ring of time levels, level n of `times` in slot (head + n) % cap
        long cap = 0, head = 0;
        long pending_from = -1;     // first level (index into `times`) whose copy may still be in flight, or -1
        bool windowed = false;      // levels have been appended (trm_series_append): trm_series_trim_before may release its head
        bool trimmed = false;       // ... and has: evaluations before `trimmed_before` would need levels that are gone
        double trimmed_before = 0.0;
        size_t slot(int n) const { return (size_t)((head + n) % cap); }
    };
    std::vector<Series> series;
    // trm_series_append: host values are staged through pinned memory and copied on a side stream under the running steps
    hipStream_t copy_stream = nullptr;
    hipEvent_t copy_done = nullptr;     // the last appended levels have reached the device
    hipEvent_t copy_order = nullptr;    // the context stream's work at the time levels were last released (trim)
    bool copy_pending = false, order_recorded = false;
    void* h_stage = nullptr;            // pinned staging buffer
    size_t h_stage_cap = 0;
    // ring grid (ColumnRingGrid, column_ring_grid.jl:37-59): column i <-> point ring_index[i] of the full grid
    long ring_points = 0;
    int32_t* d_ring_inv = nullptr;      // [ring_points] column of a grid point, -1 outside the mask
    int32_t* d_ring_idx = nullptr;      // [Nh] grid point of a column
    void* d_ring = nullptr;             // staging [rows][ring_points]
    size_t ring_cap = 0;
    void* bc_value_stage[TRM_BCV_COUNT][2] = {};  // Heun: the stage evaluates its boundary series at t + dt
    // the two-call Heun (trm_heun_predict / trm_heun_correct): stage buffers the caller writes between the two calls
    bool stage_bc_user[TRM_BCV_COUNT][2] = {};    // handed out by trm_stage_bc_device_ptr
    bool stage_vwc_own = false;                   // the stage reads its own per-cell vwc_forcing (else the state's)
    bool heun_pending = false;                    // trm_heun_predict has run, trm_heun_correct has not
    bool heun_stage_aux = false;                  // ... and trm_heun_stage_auxiliary has (compute_auxiliary!(stage) is done)
    double heun_dt = 0.0;
    void* d_top3 = nullptr;  // LandModel: [3][Nh] (T, sat, liq) of the top cell as left by the last fused step
    bool top_valid = false;  // ... and whether they still describe the state (any other writer clears it)
    bool top_escaped = false;  // a device pointer to T / sat / liq was handed out: never trust the copies again
    bool tend_valid = true;    // the tendency fields hold what the reference would (false after a fused step that did not finalize)
    // the stored (temperature, liquid_water_fraction) ARE the energy closure of the stored (internal_energy, saturation):
    // true after a fused step / closure!, false after anything else wrote one of the four fields.  Lets the step derive
    // them in registers instead of reading them (k_column<DERIVE>).
    bool closure_consistent = false, closure_escaped = false, saved_closure_consistent = false;
    // TRM_OPT_DEFER_CLOSURE_STORES: a deriving per-step launch does not store T / liq (nothing reads them before the next step derives
    // them again).  `closure_deferred`: the T / liq arrays are stale and the stored (U, sat) define them -- every entry point that may
    // read or write field memory materialises them first (flush_closure, k_materialize_closure).
    int opt_defer_closure = 1;
    bool closure_deferred = false;
    int64_t materializations = 0;   // TRM_INFO_MATERIALIZATIONS: k_materialize_closure launches so far
    // TRM_OPT_INTERIOR_STEPS: inside one trm_step call the fp64 Richards per-step launches but the last store U, sat, surface_excess_water
    // and the water table alone (k_column_psi<PSI_INTERIOR>), and the launch behind one derives the pressure head at entry.
    // `psi_consistent`: the stored pressure_head / water_table are what a k_column ForwardEuler launch left for the stored saturation
    // (set by Ops::fused_epilogue after such a launch, cleared by everything else that sets closure_consistent).
    int opt_interior = 2;           // 0 off, 1 whenever legal, 2 the library's rule (StepPolicy::interior_capable)
    bool psi_consistent = false;
    int64_t interior_launches = 0;  // TRM_INFO_INTERIOR_LAUNCHES
    void* d_zero = nullptr;  // [Nh] zeros: stands in for the value array of every unset boundary condition
    double* d_reduce = nullptr;  // scratch for trm_reduce
    size_t reduce_cap = 0;
    void* d_io = nullptr;        // staging buffer of trm_upload / trm_download (host layout [rows][Nh])
    size_t io_cap = 0;
    double time = 0.0;
    int64_t iteration = 0;
    int opt_packed = 1;   // fp32: two columns per lane with packed math where the path allows it
    int opt_async = 0, opt_kernel = TRM_KERNEL_FUSED, opt_write_kf = 1, opt_vwc_field = 0;
    int opt_derive = 2;
    int opt_steps_per_launch = 0;   // 0: chosen by the library (auto_steps_per_launch), 1: one launch per step, m > 1: up to m steps per launch
    // Two halves of the columns (TRM_OPT_PIPELINE_PARTS): the per-step LandModel path runs the latency-bound 0-D surface
    // processes of one half in the same launch as the soil columns of the other (k_land_euler).  Columns are independent.
    int opt_pipeline = 2;           // 0: off, 1: whenever legal, 2: auto (column threshold)
    int opt_zero_gradient_fast = 1; // TRM_OPT_ZERO_GRADIENT_FAST: FreeDrainage()-like conditions on the branch-free programs
    int opt_bc_signature = 1;       // TRM_OPT_BC_SIGNATURE: 1 the program with the boundary kinds compiled in where one matches
    int opt_single_step = 2;        // TRM_OPT_SINGLE_STEP_PROGRAM: 0 off, 1 whenever legal, 2 the library's rule
    int part = -1;                  // part the launch helpers currently address (-1: all columns)
    long part_lo[2] = {0, 0}, part_n[2] = {0, 0};
    // Launch arguments (DevParams, View of the state / the stage, StageView) are built once and reused by every launch;
    // any call that changes what they are built from (boundary conditions, options, lazily allocated buffers) clears
    // `args_valid` and the next launch rebuilds them.
    // multi-device diagnostics: one RCCL communicator per context, collectives on a side stream (never on the step path)
    ncclComm_t comm = nullptr;
    int comm_rank = 0, comm_world = 1;
    uint64_t comm_group = 0;    // hash of the ncclUniqueId the communicator was created from (0: none)
    hipStream_t comm_stream = nullptr;
    double* d_comm = nullptr;   // [2 * (Nz + 1) + 8] doubles: send | recv
    // vegetation (trm_set_vegetation)
    int veg_mode = TRM_VEGETATION_OFF;
    trm_vegetation_params veg_params{};
    // multi-step program with time series: device copies of the slot table and the per-step rows
    void* d_series_table = nullptr;
    void* d_series_rows = nullptr;
    size_t series_rows_cap = 0;
    // pinned staging for them: a ring, so that a launch never waits for the stream -- only for the copy that used the same
    // staging buffer four launches ago
    struct RowStage { void* h = nullptr; size_t cap = 0; hipEvent_t done = nullptr; bool pending = false; };
    RowStage row_stage[4];
    int row_stage_next = 0;
    // LandModel, TRM_OPT_SURFACE_IN_LAUNCH: the surface processes run in the first workgroups of the step launch (k_column_land) and
    // hand ground heat flux, infiltration and skin temperature to the column workgroups through granules tagged with the launch's epoch
    unsigned debug_handoff_tag_bias = 0;        // TRM_DEBUG_HANDOFF_TAG_BIAS (tests of the bounded wait)
    unsigned long long* d_gran = nullptr;   // [Nh][6], zero at allocation (epoch 0 is never used)
    uint32_t front_epoch = 0;               // epoch of the last such launch
    int opt_front = 2;                      // 0 off, 1 whenever legal, 2 the library's rule
    int last_program = 0;                   // TRM_INFO_LAST_PROGRAM: the kernel instance the last step launch selected
    // time averages (trm_average_*): handle = index; field -1 marks a closed slot.  d_sum is [field_elems] doubles in the field's
    // device layout.
    struct Average { int field = -1; double* d_sum = nullptr; double window = 0.0; int64_t steps = 0; };
    std::vector<Average> averages;
    double* d_acc_partial[trm::ACC_SLOTS] = {};   // the fused path's partials of a field with more than one open accumulator
    // forward-mode tangents (trm_tangent_*): dU, dT, dliq in the device layout of a 3-D field ([Nh][Nzp] doubles), null while closed; on a
    // Richards context (TRM_OPT_DERIVATIVE_RICHARDS) also dsat and dpsi, which are allocated there and nowhere else.
    // `tan_stale`: another call has changed the state since the tangent was seeded (trm_tangent_upload of dU clears it).
    double* d_tan[5] = {};
    bool tan_stale = false;
    // the seeds of the boundary values (trm_tangent_bc_upload), [Nh] doubles each: d(temperature value) bottom, top, d(internal-energy
    // flux) bottom, top.  Allocated by the first upload, zeroed by trm_tangent_open; `tan_bc_seeded`: one has been uploaded since
    // trm_tangent_open, and trm_step_tangent runs the seeded instances.  Seeds are not state: nothing makes them stale.
    double* d_tan_bc[4] = {};
    bool tan_bc_seeded = false;
    // the seeds of the thermal parameters (trm_tangent_param_set) as the kernels take them: of the eight numbers DevParams holds, in the
    // order sk_water, sk_ice, sk_air, s0, c_water, c_ice, c_air, C0 (thermal_param_chain below).  Zeroed by trm_tangent_open;
    // `tan_param_seeded`: set since trm_tangent_open, and trm_step_tangent / trm_tangent_closure run the parameter-seeded instances.
    double tan_param[8] = {};
    bool tan_param_seeded = false;
    // TRM_OPT_DERIVATIVE_SERIES: 1 lets trm_step_tangent / trm_step_record / trm_adjoint_backward run with boundary time series on the four
    // pairs above, evaluated in the launch (trm_series_derivative.hpp); 0 (default): they refuse a context with a series attached.
    // `derivative_series`: TRM_INFO_DERIVATIVE_SERIES, the series the last derivative launch evaluated in-kernel.
    int opt_derivative_series = 0, derivative_series = 0;
    // TRM_OPT_DERIVATIVE_SERIES_PARAMS: thermal-parameter seeds / gradients ride together with the series (RIDE_PARAM_SERIES)
    int opt_derivative_series_params = 0;
    // TRM_OPT_DERIVATIVE_RICHARDS: the tangent's state-seed calls accept a heat + Richards context (k_column_tangent_rich)
    int opt_derivative_richards = 0;
    // TRM_OPT_DERIVATIVE_RICHARDS_ADJOINT: the per-step tape of the adjoint accepts a heat + Richards context (k_column_adjoint_rich)
    int opt_derivative_richards_adjoint = 0;
    // TRM_OPT_DERIVATIVE_RICHARDS_PARAMS: together with the option above, trm_adjoint_param_open opens the gradients with respect to the
    // seven hydraulic parameters on such a context (k_column_adjoint_rich_params)
    int opt_derivative_richards_params = 0;
    // TRM_OPT_DERIVATIVE_RICHARDS_RECORD: together with TRM_OPT_DERIVATIVE_RICHARDS_ADJOINT, the seven attached-record calls accept such a
    // context: a soil-moisture record read inside the backward launches (k_column_adjoint_rich_record)
    int opt_derivative_richards_record = 0;
    // the seeds of the seriesed pairs (trm_tangent_bc_series_upload), [nt][Nh] doubles in the order of d_tan_bc, `tan_bcs_nt` their
    // levels; null: none yet (trm_step_tangent allocates zeros).  Zeroed by trm_tangent_open, freed by trm_tangent_close.
    double* d_tan_bcs[4] = {};
    long tan_bcs_nt[4] = {};
    // reverse-mode gradients (trm_adjoint_*): the cotangent fields of U, T, liq in the same layout, and the tape of trm_step_record --
    // `tape_cap` slots of [Nh][Nzp] doubles, slot k the internal energy before taped step k, `tape_dt[k]` that step's dt.  `adj_stale`:
    // another call has changed the state or a boundary condition since the first taped step (state_changed / bc_changed below).
    // On a Richards context (TRM_OPT_DERIVATIVE_RICHARDS_ADJOINT) also the cotangent fields of sat and psi, allocated there and nowhere
    // else, and a slot is two fields: the internal energy and, behind it, the saturation before the step.
    double* d_adj[5] = {};
    // the boundary-gradient accumulators (trm_adjoint_bc_open), [Nh] doubles each, in the order of d_tan_bc; null: the sweep runs the
    // instances without
    double* d_adj_bc[4] = {};
    // the thermal-parameter accumulators (trm_adjoint_param_open): eight per-cell fields [Nh][Nzp] in the order of tan_param, and the
    // result of k_param_reduce, [TRM_THERMAL_PARAM_COUNT][Nh]; null: the sweep runs the instances without
    // the node accumulators of the seriesed pairs (trm_adjoint_bc_series_download), [nt][Nh] doubles in the order of d_tan_bc, zeroed in
    // front of every sweep; `tape_rows`: the SeriesRows trm_step_record uploaded, [taped step][series] -- the sweep uploads the slice a
    // launch covers, so that it sees exactly the record's brackets and fractions
    double* d_adj_bcs[4] = {};
    long adj_bcs_nt[4] = {};
    std::vector<trm::SeriesRow> tape_rows;
    double* d_adj_param[8] = {};
    double* d_adj_param_out = nullptr;
    // the hydraulic-parameter accumulators of a Richards context (trm_adjoint_param_open under TRM_OPT_DERIVATIVE_RICHARDS_PARAMS): seven
    // per-cell fields [Nh][Nzp] in the order of TRM_HYDRAULIC_PARAM_*, and the result of k_hyd_param_reduce,
    // [TRM_HYDRAULIC_PARAM_COUNT][Nh]; null: the sweep runs the instances without
    double* d_adj_hyd[7] = {};
    double* d_adj_hyd_out = nullptr;
    double* d_tape = nullptr;
    int tape_cap = 0;
    std::vector<double> tape_dt;
    bool adj_stale = false;
    // the checkpointed tape (trm_adjoint_open_checkpointed): `ckpt_interval` K > 0, `tape_cap` counts checkpoint slots, tape_dt stays
    // empty and `tape_segs` lists the taped steps instead -- a segment is up to K consecutive steps under one dt, its first state in
    // `slot` (segments take the slots in order)
    struct TapeSegment {
        int first, len;
        double dt;
        int slot;
    };
    int ckpt_interval = 0;
    std::vector<TapeSegment> tape_segs;
    // adjoint observations (trm_adjoint_observe, trm_adjoint_observe_misfit; trm_launch_observe.hip): cotangents that enter lam at a taped
    // position, in registration order.  An observation keeps what the caller gave and nothing else: `arrays` arrays of [nlevels][Nh]
    // doubles (linear: the cotangent; misfit: T_obs, then the weights if any were given) and behind them the nlevels int32 levels, in
    // one allocation.  `d_misfit`: each column's share of the misfit so far, [Nh] doubles, null until the first misfit observation.
    // `tape_seg_closed`: an observation has closed the open segment of the checkpointed tape (open_segment_room), so that the next
    // taped step opens one and the observed state is a checkpoint.
    struct Observation {
        int position;   // steps on the tape when it was registered
        int kind;       // TRM_ADJOINT_* (linear), OBSERVE_MISFIT
        int nlevels, arrays;
        double* d_data;
        const double* array(int a, long Nh) const { return a < arrays ? d_data + (size_t)a * (size_t)nlevels * (size_t)Nh : nullptr; }
        const int32_t* levels(long Nh) const { return (const int32_t*)(d_data + (size_t)arrays * (size_t)nlevels * (size_t)Nh); }
        int64_t bytes(long Nh) const { return (int64_t)arrays * nlevels * (int64_t)Nh * 8 + (int64_t)nlevels * 4; }
    };
    static constexpr int OBSERVE_MISFIT = 3;
    std::vector<Observation> observations;
    double* d_misfit = nullptr;
    bool tape_seg_closed = false;
    // An attached temperature record (trm_adjoint_observe_record*; DESIGN 4.8 "Attached records"): read inside the backward launches, kept
    // across sweeps, dropped by a detach, a new tape or trm_adjoint_close.  `rec`: its positions (taped-step counts) and levels; the tables
    // are built for a tape of rec.entries - 1 steps by the first sweep, and again by a sweep over another count.  `d_rec_observed` /
    // `d_rec_weight` ([npos][nlevels][Nh]; the weights may be null): the library's copies in `d_rec_owned`, or the caller's device arrays
    // (then d_rec_owned is null).  `d_rec_out`: the residuals [npos][nlevels][Nh] and behind them the misfit [Nh].  `rec_swept`: a sweep
    // has run with this record, so the residuals and the misfit are its.
    RecordTable rec;
    double* d_rec_owned = nullptr;
    const double *d_rec_observed = nullptr, *d_rec_weight = nullptr;
    double* d_rec_out = nullptr;
    bool rec_swept = false;
    // A tangent record (trm_tangent_record_attach; DESIGN 4.7 "Tangent records"): T and dT sampled inside the tangent launches, kept until
    // a detach, trm_tangent_open or trm_tangent_close.  `trec`: its positions (tangent-step counts since the attach or the last rewind)
    // and levels; the tables are built at the attach, up to tangent_record_limit.  `d_trec`: the samples of T and of dT,
    // [npos][nlevels][Nh] each, NaN where no launch has stored.  `trec_position`: tangent steps run since the attach or the last rewind.
    RecordTable trec;
    double* d_trec[2] = {};
    long long trec_position = 0;
    bool args_valid = false;
    void* args = nullptr;   // LaunchArgs<NF>*, owned
    void (*args_free)(void*) = nullptr;
    std::string err;
};

namespace trmh {
using namespace trm;

// errors: the message stays with the context (trm_last_error); without one, with the calling thread
int fail(trm_ctx* ctx, int code, const std::string& msg);

#define TRM_HIP(ctx, call)                                                                               \
    do {                                                                                                 \
        hipError_t e__ = (call);                                                                         \
        if (e__ != hipSuccess)                                                                           \
            return ::trmh::fail(ctx, TRM_EHIP, std::string(#call) + ": " + hipGetErrorString(e__));     \
    } while (0)

// ---- shared by the entry points of the trm_*_api.hip files: everything that crosses between them, each defined (and described) in the
// one file named.  trm_context_api.hip:
int finish(trm_ctx* c, int rc);                 // the end of a launching entry point: waits for the stream unless TRM_OPT_ASYNC
void tick(trm_ctx* c, double dt, int nsteps);   // tick! per step
void bc_changed(trm_ctx* c);                    // a boundary condition has changed under an open tape
void state_changed(trm_ctx* c);                 // ... the state has, under an open tangent or tape
int flush_closure(trm_ctx* c);                  // T / liq into their arrays if the last step launches left them unstored
int io_buffer(trm_ctx* c, size_t bytes);        // the staging buffer d_io, grown to `bytes`
// trm_field_io_api.hip: host data [Nz][Nh] to / from a 3-D device buffer [Nh][Nzp] through d_io, synchronised (instantiated for double and
// float).  `top`: the [Nh] buffer of a Face field's top face, which travels as row Nz of the host array (null: Nz rows)
template <class NF> int upload_3d(trm_ctx* c, const NF* host, NF* dev, NF* top = nullptr);
template <class NF> int download_3d(trm_ctx* c, const NF* dev, NF* host, const NF* top = nullptr);
// the derivative buffers of the context (d_tan*, d_adj*, d_tape) are freed here and nowhere else: the close calls, an open that fails,
// trm_destroy (trm_derivative_api.hip)
void release_tangent(trm_ctx* c);
void release_adjoint(trm_ctx* c);
// ... each named by the trm_<unit>_api.hip file that defines it.  Hidden: they serve the entry points alone and are no dynamic symbols
#pragma GCC visibility push(hidden)
int alloc_fields(trm_ctx* c, FieldSet& s);                     // context: the fields of `s` the context has and that are not allocated yet, zeroed; synchronised
int fill_input_row(trm_ctx* c, int field, double value);       // context: every column of a 2-D field of the state set to `value`; synchronised
int upload_field(trm_ctx* c, int field, const void* host);     // field_io: host data [rows][Nh] of the context's precision into a field of the state; synchronised
int sync_copies(trm_ctx* c);                                   // series: every H2D copy of trm_series_append has finished (before a series buffer is freed or reallocated)
int check_ctx_list(trm_ctx** ctxs, int n, const char* who);    // comm: n contexts that are shards of one grid, or the refusal `who` reports; clears their messages
#pragma GCC visibility pop

// TRM_ENTER: any entry point but the three of the two-call Heun step and the read-only ones.  A stage predicted by
// trm_heun_predict belongs to the state and clock it was predicted from: whatever else runs in between drops it, and a later
// trm_heun_correct fails ("call trm_heun_predict first") instead of averaging tendencies of a stage that describes another state.
// Both materialise T / liq first if the last step launches left them unstored (flush_closure, TRM_OPT_DEFER_CLOSURE_STORES): whatever
// the entry point reads or writes, it finds the arrays an eagerly storing context has.  TRM_ENTER_KEEP: the entry points that neither
// read nor write field memory, or order the accesses themselves -- trm_step / trm_step_timed (Ops::fused_launch), trm_restore_state
// (overwrites the fields), trm_synchronize, trm_status; the getters that take no macro at all belong here too.
#define TRM_ENTER_KEEP(c)                                    \
    if (!(c)) return TRM_EINVAL;                             \
    TRM_HIP(c, hipSetDevice((c)->device));
#define TRM_ENTER_HEUN(c)                                    \
    TRM_ENTER_KEEP(c)                                        \
    if ((c)->closure_deferred)                               \
        if (int rc_flush__ = ::trmh::flush_closure(c)) return rc_flush__;
#define TRM_ENTER(c)                                         \
    TRM_ENTER_HEUN(c)                                        \
    (c)->heun_pending = false;


inline long field_rows(const trm_ctx* c, int field) {
    if (field == TRM_FIELD_HYDRAULIC_CONDUCTIVITY) return c->Nz + 1;
    if (field <= TRM_FIELD_TEND_SATURATION_WATER_ICE || field == TRM_FIELD_VWC_FORCING) return c->Nz;
    if (field == TRM_FIELD_PLANT_AVAILABLE_WATER || field == TRM_FIELD_ROOT_FRACTION) return c->Nz;
    return 1;
}
inline bool valid_field(int f) { return f >= 0 && f < TRM_FIELD_COUNT; }
inline bool is_input_field(int f) {
    return (f >= TRM_FIELD_AIR_TEMPERATURE && f <= TRM_FIELD_SURFACE_LONGWAVE_DOWN) || f == TRM_FIELD_ALBEDO || f == TRM_FIELD_EMISSIVITY ||
           (f >= TRM_FIELD_CO2 && f <= TRM_FIELD_VEGETATION_GROUND_TEMPERATURE) || f == TRM_FIELD_STEM_AREA_INDEX;
}
inline bool is_3d(int field) {
    return field <= TRM_FIELD_TEND_SATURATION_WATER_ICE || field == TRM_FIELD_VWC_FORCING || field == TRM_FIELD_PLANT_AVAILABLE_WATER ||
           field == TRM_FIELD_ROOT_FRACTION;
}
// the 3-D vegetation fields exist only once trm_set_vegetation has run
inline bool is_lazy_field(int field) { return field == TRM_FIELD_PLANT_AVAILABLE_WATER || field == TRM_FIELD_ROOT_FRACTION; }
// elements of the device buffer of a field: [Nh][Nzp] for 3-D fields, [Nh] for 2-D fields
inline size_t field_elems(const trm_ctx* c, int field) { return is_3d(field) ? (size_t)c->Nh * c->Nzp : (size_t)c->Nh; }

template <class NF> struct StageView { const NF *bcT_bot, *bcT_top; };
template <class NF> struct LaunchArgs {
    DevParams<NF> p;
    View<NF> state, stage;
    View<NF> part[2];   // the state's view restricted to the two pipeline parts
    StageView<NF> w;
};
// columns the launch helpers currently address: all of them, or one pipeline part
inline long ncols(const trm_ctx* c) { return c->part >= 0 ? c->part_n[c->part] : c->Nh; }
inline long first_col(const trm_ctx* c) { return c->part >= 0 ? c->part_lo[c->part] : 0; }
// Launch arguments (DevParams, View of the state / the stage, StageView) are built once and reused by every launch (defined in
// trm_context_api.hip, instantiated for double and float)
template <class NF> const LaunchArgs<NF>& launch_args(trm_ctx* c);
template <class NF> const View<NF>& cached_view(trm_ctx* c, const FieldSet& s) {
    const LaunchArgs<NF>& a = launch_args<NF>(c);
    if (&s == &c->stage) return a.stage;
    return c->part >= 0 ? a.part[c->part] : a.state;
}
// the state's view as the step launches see it (one pipeline part, or everything)
template <class NF> const View<NF>& state_view(trm_ctx* c) { return cached_view<NF>(c, c->state); }

inline dim3 cell_grid(const trm_ctx* c, long /*rows*/ = 0) { return dim3((unsigned)(((size_t)c->Nh * c->Nzp + 255) / 256), 1, 1); }
inline dim3 col_grid(const trm_ctx* c) { return dim3((unsigned)((ncols(c) + 255) / 256), 1, 1); }
// lane = level kernels: one column per LPC lanes, 4 waves per workgroup
inline dim3 wave_grid(const trm_ctx* c, int lpc) {
    long waves = (ncols(c) + (64 / lpc) - 1) / (64 / lpc);
    return dim3((unsigned)((waves + 3) / 4), 1, 1);
}
inline dim3 column_grid(const trm_ctx* c, int lpc) {
    dim3 grid = wave_grid(c, lpc);
    grid.x = (grid.x * 4 + (TRM_STEP_BLOCK / 64) - 1) / (TRM_STEP_BLOCK / 64);  // wave_grid counts 4-wave workgroups
    return grid;
}
// addresses one part of the columns for the lifetime of the scope
struct PartScope {
    trm_ctx* c;
    PartScope(trm_ctx* ctx, int q) : c(ctx) { c->part = q; }
    ~PartScope() { c->part = -1; }
};

// Time interpolation indices of a series at time t (defined in trm_series_api.hip)
void series_time_indices(const std::vector<double>& times, int indexing, double t, int& n1, int& n2, double& f, double& g);

// ---- launch policies: which kernel instance a context takes (pure host logic, shared by every translation unit) -------------
template <class NF> struct Policy {
    static bool richards(const trm_ctx* c) { return c->params.flow == TRM_FLOW_RICHARDS; }
    static bool coupled(const trm_ctx* c) { return c->veg_mode == TRM_VEGETATION_COUPLED; }
    // hydraulics specialisation of this context (trm_device.hpp: HYD_*)
    static int hyd(const trm_ctx* c) {
        if (c->params.swrc == TRM_SWRC_BROOKS_COREY && c->params.unsat_k == TRM_UNSATK_LINEAR) {
            // the compile-time instance is lambda = 0.2 (-1/lambda = -5 exactly, Base's integer power); other lambda: generic
            const PowSpec<NF> spec = make_pow_spec<NF>(NF(-1) / (NF)c->params.bc_lambda);
            return (spec.kind == POW_INT && spec.n == -5) ? HYD_BC_LINEAR : HYD_GENERIC;
        }
        if (c->params.swrc == TRM_SWRC_VAN_GENUCHTEN && c->params.unsat_k == TRM_UNSATK_VAN_GENUCHTEN) {
            // the compile-time instance is van Genuchten's n = 2 (every reference test and example); other n: generic
            // (n = 2 exactly: -1/m = -2 {INT}, 1/n = (n-1)/n = 1/2 {HALVES, 1}, n/(n+1) = RN(2/3) {THIRDS, 2} in make_pow_spec)
            if (c->params.vg_n == 2.0) return HYD_VG_N2;
        }
        return HYD_GENERIC;
    }
    // the branch-free fused kernel covers Value on temperature and Flux on the prognostics; anything else is generic
    static bool generic_bcs(const trm_ctx* c) {
        bool generic = c->opt_vwc_field != 0;   // a per-cell vwc_forcing field is read by the generic instance only
        // (a zero gradient on temperature or pressure head at the bottom is the edge-value halo of the branch-free programs: see
        // trm_ctx::bc_zero_gradient.  Not on saturation / liquid fraction, whose unset halo follows the halo policy, and not at the top,
        // where edge + (+0) * dz turns an edge value of -0.0 into +0.0)
        auto plain = [&](int var, int side) { return side == 0 && c->opt_zero_gradient_fast && c->bc_kind[var][side] == TRM_BC_GRADIENT && c->bc_zero_gradient[var][side]; };
        for (int side = 0; side < 2; ++side) {
            generic = generic || (c->bc_kind[TRM_BCV_TEMPERATURE][side] == TRM_BC_GRADIENT && !plain(TRM_BCV_TEMPERATURE, side));
            for (int var : {TRM_BCV_SATURATION_WATER_ICE, TRM_BCV_LIQUID_WATER_FRACTION, TRM_BCV_PRESSURE_HEAD})
                generic = generic || c->bc_kind[var][side] == TRM_BC_VALUE ||
                          (c->bc_kind[var][side] == TRM_BC_GRADIENT && !(var == TRM_BCV_PRESSURE_HEAD && plain(var, side)));
        }
        return generic;
    }
    // Deriving T and liq in registers saves 2 of 11 field accesses and costs ~40 instructions per cell.  Measured on MI355X
    // (profiles/r03/exp4_ab_derive.log, interleaved medians on one box; fp64): 8 x N145 (HBM-resident) 215 vs 261 us, N145
    // 25.1 vs 27.3 us with the reference-default hydraulics, 33.6 vs 35.1 (LandModel), 34.4 vs 35.6 (LandModel, van Genuchten);
    // it loses on small grids (N72 heat-only: 7.1 vs 6.6 us, latency-bound) and for the packed fp32 kernel, which is not short of
    // bytes (C5: liquid fraction alone 523 vs 500 us, both 562 vs 533).  Deriving the liquid fraction alone (mode 3: one read
    // less, the temperature divide saved) sits between the two everywhere (8 x N145: 238 us) and is kept as an option only.
    // AUTO (2): fp64 states beyond the Infinity Cache, or of >= 24 576 columns; fp32 states beyond the cache on the packed kernel:
    // the liquid fraction alone (the numbers above for the packed kernel predate the store ordering of round 3; see below).
    template <bool RICH> static int derive_now(const trm_ctx* c) {
        // (the coupled vegetation reads T and liq of the whole column from memory every step)
        if (!c->closure_consistent || c->closure_escaped || coupled(c) || c->opt_derive == 0) return DERIVE_NONE;
        if (c->opt_derive == 1) return DERIVE_T_LIQ;
        // (3, 4: the packed fp32 step's modes -- the liquid fraction alone; that and the pressure head.  The fp64 column program had
        // instances for "liquid fraction alone" and "pressure head as well" (value 5) until round 5: both measured slower than
        // deriving T and liq, EXPERIMENTS.md; the values now select what the library offers there: both T and liq)
        const bool packed = std::is_same<NF, float>::value && packed_path(c);
        if (c->opt_derive == 3) return packed ? DERIVE_LIQ : DERIVE_T_LIQ;
        if (c->opt_derive == 5) return DERIVE_T_LIQ;
        if (c->opt_derive == 4) return packed ? (RICH ? DERIVE_LIQ_PSI : DERIVE_LIQ) : DERIVE_T_LIQ;
        const size_t state_bytes = (size_t)(RICH ? 6 : 4) * (size_t)c->Nh * (size_t)c->Nzp * sizeof(NF);
        const bool beyond_cache = state_bytes > ((size_t)256 << 20);
        const bool large = c->Nh >= 24576;
        // fp32 on the packed kernel, HBM-resident: the liquid fraction alone (r3, re-measured on the final kernels,
        // profiles/r03/exp21_derive_liq_fp32.log: C5 443.7 vs 457.9 us, C5-VG 472.5 vs 476.3; before the store ordering it lost)
        if (std::is_same<NF, float>::value) return (beyond_cache && packed_path(c)) ? DERIVE_LIQ : DERIVE_NONE;
        return (beyond_cache || large) ? DERIVE_T_LIQ : DERIVE_NONE;
    }
    // The per-column outputs of the column program through the workgroup's staging table (template parameter STAGED) or as direct 2-lane
    // stores.  Measured (profiles/r03/exp20_staged_small_stores.log, same box, alternating): staged wins where the state streams
    // from HBM (8 x N145: 201.7 vs 212.9 us, -5.3 %) and on the LandModel with its seven outputs (C4 33.7 vs 34.4), it loses
    // where the step is launch- and latency-bound (C3 25.2 vs 24.7, N72 heat-only 7.3 vs 6.7): the barrier in front of the
    // staged store.  TRM_STAGED_SMALL = 0 / 1 in the environment forces it (experiments).
    // The per-column inputs of the column program through the scalar memory path: cache-resident states (see column_program).
    // TRM_SCALAR_INPUTS = 0 / 1 in the environment forces it (experiments, tests).
    template <bool RICH> static int scalar_inputs_now(const trm_ctx* c) {
        static const int forced = [] { const char* e = std::getenv("TRM_SCALAR_INPUTS"); return e ? std::atoi(e) : -1; }();
        if (forced >= 0) return forced != 0;
        const size_t state_bytes = (size_t)(RICH ? 6 : 4) * (size_t)c->Nh * (size_t)c->Nzp * sizeof(NF);
        return state_bytes <= ((size_t)256 << 20) ? 1 : 0;
    }
    // The packed fp32 step does not gain (C5 472 vs 468 us, C5-VG 500 vs 487; exp20b): staging is off there unless forced.
    template <bool RICH> static int staged_now(const trm_ctx* c, bool packed = false) {
        static const int forced = [] { const char* e = std::getenv("TRM_STAGED_SMALL"); return e ? std::atoi(e) : -1; }();
        if (forced >= 0) return forced != 0;
        if (packed) return 0;
        const size_t state_bytes = (size_t)(RICH ? 6 : 4) * (size_t)c->Nh * (size_t)c->Nzp * sizeof(NF);
        const bool beyond_cache = state_bytes > ((size_t)256 << 20);
        return (beyond_cache || (c->params.seb != 0 && c->Nh >= 24576)) ? 1 : 0;
    }
    // The (STAGED, SCALAR_IN) combinations that have instances (round 5: the ones no rule selects were removed).  The rules above
    // give (0, 1) for cache-resident states, (1, 1) for large cache-resident LandModels, (1, 0) beyond the cache; the environment
    // switches of the tests can ask for anything: (0, 0) -- direct 2-lane stores AND vector loads of one address -- has no
    // instance anywhere (-> (0, 1)); (1, 1) exists where a surface energy balance can run: the LandModel signature and the
    // programs that read the kinds at run time (elsewhere -> (1, 0)).
    static void io_paths(bool land_or_runtime_kinds, int& staged, int& scalar_in) {
        if (!staged && !scalar_in) scalar_in = 1;
        if (staged && scalar_in && !land_or_runtime_kinds) scalar_in = 0;
    }
    // fp32: two columns per lane with packed math (trm_packed_f32.hpp) -- the reference-default hydraulics, and van
    // Genuchten retention with Mualem conductivity
    static bool packed_path(const trm_ctx* c) {
        if (!std::is_same<NF, float>::value || !c->opt_packed || generic_bcs(c)) return false;
        if (hyd(c) == HYD_VG_N2) return true;
        return hyd(c) == HYD_BC_LINEAR;
    }
    // soil levels per lane of the fused column kernels: one (k_column, <= 64 levels), two (k_column_deep, 65 ... 128) or four
    // (k_column_wide, 129 ... 256: trm_column_deep.hpp / trm_column_wide.hpp), one column per wavefront from two on; 0: deeper, no
    // fused kernel
    static int levels_per_lane(const trm_ctx* c) { return c->Nz <= 64 ? 1 : c->Nz <= 128 ? 2 : c->Nz <= 256 ? 4 : 0; }
    // slot of the multi-step program a series feeds, or -1 when the program cannot take it (the step then runs per launch)
    static int series_slot(const trm_ctx* c, const trm_ctx::Series& sr) {
        if (sr.is_bc) {
            const int kind = c->bc_kind[sr.var][sr.side];
            if (sr.var == TRM_BCV_TEMPERATURE && kind == TRM_BC_VALUE) return sr.side == TRM_TOP ? SLOT_T_TOP : SLOT_T_BOT;
            if (sr.var == TRM_BCV_INTERNAL_ENERGY && kind == TRM_BC_FLUX && !(c->params.seb && sr.side == TRM_TOP)) return sr.side == TRM_TOP ? SLOT_FU_TOP : SLOT_FU_BOT;
            if (sr.var == TRM_BCV_SATURATION_WATER_ICE && kind == TRM_BC_FLUX && richards(c) && !(c->params.seb && sr.side == TRM_TOP)) return sr.side == TRM_TOP ? SLOT_FS_TOP : SLOT_FS_BOT;
            return -1;
        }
        if (!c->params.seb) return -1;     // (inputs nobody reads: leave them to update_inputs!)
        switch (sr.field) {
            case TRM_FIELD_AIR_TEMPERATURE: return SLOT_TAIR;
            case TRM_FIELD_AIR_PRESSURE: return SLOT_PRES;
            case TRM_FIELD_WINDSPEED: return SLOT_WIND;
            case TRM_FIELD_SPECIFIC_HUMIDITY: return SLOT_QAIR;
            case TRM_FIELD_RAINFALL: return SLOT_RAIN;
            case TRM_FIELD_SURFACE_SHORTWAVE_DOWN: return SLOT_SWD;
            case TRM_FIELD_SURFACE_LONGWAVE_DOWN: return SLOT_LWD;
            case TRM_FIELD_ALBEDO: return c->params.prescribed_albedo ? SLOT_ALBEDO : -1;
            case TRM_FIELD_EMISSIVITY: return c->params.prescribed_albedo ? SLOT_EMISSIVITY : -1;
            default: return -1;
        }
    }
    static bool series_fit_program(const trm_ctx* c) {
        for (const auto& sr : c->series)
            if (series_slot(c, sr) < 0) return false;
        return true;
    }
    static VegDev<NF> veg_dev(const trm_ctx* c) {
        VegDev<NF> p;
        const double* s = &c->veg_params.tau25;
        NF* t = &p.tau25;
        for (int n = 0; n < 40; ++n) t[n] = (NF)s[n];
        p.eps_mw = (NF)c->params.eps_mw;
        p.one_minus_eps_mw = NF(1) - p.eps_mw;
        p.sqrt_eps = std::sqrt(std::numeric_limits<NF>::epsilon());
        p.paw_span = p.field_capacity - p.wilting_point;
        p.rpaw_span = NF(1) / p.paw_span;
        p.ln_q10_tau = std::log(p.q10_tau); p.ln_q10_Kc = std::log(p.q10_Kc); p.ln_q10_Ko = std::log(p.q10_Ko);
        p.ts_k1 = NF(2) * std::log(NF(1) / NF(0.99) - NF(1)) / (p.T_CO2_low - p.T_photos_low);     // photosynthesis.jl:165-188
        p.ts_k2 = NF(0.5) * (p.T_CO2_low + p.T_photos_low);
        p.ts_k3 = std::log(NF(0.99) / NF(0.01)) / (p.T_CO2_high - p.T_photos_high);
        return p;
    }
    static VegView<NF> veg_view(const trm_ctx* c) { return veg_view(c, c->state); }
    static VegView<NF> veg_view(const trm_ctx* c, const FieldSet& s) {
        VegView<NF> v;
        auto F = [&](int id) { return (NF*)s.f[id]; };
        v.Nh = c->Nh;
        v.C_veg = F(TRM_FIELD_CARBON_VEGETATION); v.nu = F(TRM_FIELD_VEGETATION_AREA_FRACTION);
        v.G_C_veg = F(TRM_FIELD_TEND_CARBON_VEGETATION); v.G_nu = F(TRM_FIELD_TEND_VEGETATION_AREA_FRACTION);
        v.LAI_b = F(TRM_FIELD_BALANCED_LEAF_AREA_INDEX); v.phen = F(TRM_FIELD_PHENOLOGY_FACTOR); v.LAI = F(TRM_FIELD_LEAF_AREA_INDEX);
        v.gw_can = F(TRM_FIELD_CANOPY_WATER_CONDUCTANCE); v.lambda_c = F(TRM_FIELD_LEAF_TO_AIR_CO2_RATIO);
        v.An = F(TRM_FIELD_NET_ASSIMILATION); v.Rd = F(TRM_FIELD_LEAF_RESPIRATION); v.GPP = F(TRM_FIELD_GROSS_PRIMARY_PRODUCTION);
        v.Ra = F(TRM_FIELD_AUTOTROPHIC_RESPIRATION); v.NPP = F(TRM_FIELD_NET_PRIMARY_PRODUCTION);
        v.Tair = F(TRM_FIELD_AIR_TEMPERATURE); v.pres = F(TRM_FIELD_AIR_PRESSURE); v.qair = F(TRM_FIELD_SPECIFIC_HUMIDITY);
        v.swd = F(TRM_FIELD_SURFACE_SHORTWAVE_DOWN); v.CO2 = F(TRM_FIELD_CO2); v.smlf = F(TRM_FIELD_SOIL_MOISTURE_LIMITING_FACTOR);
        v.daily_Rd = F(TRM_FIELD_DAILY_LEAF_RESPIRATION);
        v.Tground = F(TRM_FIELD_VEGETATION_GROUND_TEMPERATURE);
        v.Tground_stride = 1;
        const bool canopy = coupled(c);
        auto G = [&](int id) { return canopy ? F(id) : (NF*)nullptr; };
        v.w_can = G(TRM_FIELD_CANOPY_WATER); v.G_w_can = G(TRM_FIELD_TEND_CANOPY_WATER); v.I_can = G(TRM_FIELD_CANOPY_WATER_INTERCEPTION);
        v.R_can = G(TRM_FIELD_CANOPY_WATER_REMOVAL); v.f_can = G(TRM_FIELD_SATURATION_CANOPY_WATER); v.rain_ground = G(TRM_FIELD_RAINFALL_GROUND);
        v.E_can = G(TRM_FIELD_EVAPORATION_CANOPY); v.transp = G(TRM_FIELD_TRANSPIRATION); v.SAI = G(TRM_FIELD_STEM_AREA_INDEX);
        v.paw = F(TRM_FIELD_PLANT_AVAILABLE_WATER);
        v.rootf = (const NF*)c->d_rootf;   // static: one copy serves the stage as well
        if (c->part >= 0 && &s == &c->state) {   // one pipeline part: columns [lo, lo + n)
            const long lo = first_col(c);
            v.Nh = ncols(c);
            for (NF** q : {&v.C_veg, &v.nu, &v.G_C_veg, &v.G_nu, &v.LAI_b, &v.phen, &v.LAI, &v.gw_can, &v.lambda_c, &v.An, &v.Rd, &v.GPP, &v.Ra, &v.NPP,
                           &v.w_can, &v.G_w_can, &v.I_can, &v.R_can, &v.f_can, &v.rain_ground, &v.E_can, &v.transp})
                if (*q) *q += lo;
            for (const NF** q : {&v.Tair, &v.pres, &v.qair, &v.swd, &v.CO2, &v.smlf, &v.daily_Rd, &v.Tground, &v.SAI})
                if (*q) *q += lo * (q == &v.Tground ? v.Tground_stride : 1);
            if (v.paw) v.paw += lo * c->Nzp;
        }
        return v;
    }
};
// the context's boundary kinds as a BCSIG signature (trm_kernels.hpp); meaningful where the branch-free kinds hold (Policy::generic_bcs)
inline int bc_signature_of(const trm_ctx* c) {
    const bool rich = c->params.flow == TRM_FLOW_RICHARDS;
    int sig = (c->bc_kind[TRM_BCV_TEMPERATURE][0] == TRM_BC_VALUE ? BCSIG_T_BOT : 0) | (c->bc_kind[TRM_BCV_TEMPERATURE][1] == TRM_BC_VALUE ? BCSIG_T_TOP : 0) |
              (c->bc_kind[TRM_BCV_INTERNAL_ENERGY][0] == TRM_BC_FLUX ? BCSIG_FU_BOT : 0) | ((rich && c->bc_kind[TRM_BCV_SATURATION_WATER_ICE][0] == TRM_BC_FLUX) ? BCSIG_FS_BOT : 0);
    if (c->params.seb) return sig | BCSIG_LAND;      // (the LandModel's wiring owns the top flux conditions: land_model.jl:56-61)
    return sig | (c->bc_kind[TRM_BCV_INTERNAL_ENERGY][1] == TRM_BC_FLUX ? BCSIG_FU_TOP : 0) | ((rich && c->bc_kind[TRM_BCV_SATURATION_WATER_ICE][1] == TRM_BC_FLUX) ? BCSIG_FS_TOP : 0);
}
// TRM_INFO_LAST_PROGRAM: which kernel instance a step launch selected -- family | HYD << 8 | (LPC / 32) << 10 | DERIVE << 12 |
// STAGED << 15 | SCALAR_IN << 16 | (BCSIG + 1) << 17 (0 there: the kinds are read at run time)
inline int program_id(int family, int hyd, int lpc, int derive, int staged, int scalar_in, int bcsig) {
    return family | (hyd << 8) | ((lpc / 32) << 10) | (derive << 12) | ((staged ? 1 : 0) << 15) | ((scalar_in ? 1 : 0) << 16) | ((bcsig + 1) << 17);
}
// ... and the family bits the derivative launches add (TRM_PROGRAM_COLUMN_TANGENT / _ADJOINT; bit 31 is TRM_PROGRAM_PARAMETERS)
constexpr int PROGRAM_GENERIC_HALOS = 1 << 25;   // Gradient halos on temperature, where trm_step takes k_step_wave
constexpr int PROGRAM_BC_SEEDS = 1 << 26;        // tangent: the boundary seeds ride along
constexpr int PROGRAM_BACKWARD = 1 << 26;        // adjoint: the backward launch (the record has it clear)
constexpr int PROGRAM_CHECKPOINTED = 1 << 27;    // adjoint: the checkpointed tape
constexpr int PROGRAM_BC_GRADIENT = 1 << 30;     // adjoint: the boundary gradients ride along
// One kernel launch on the context's stream, checked: like TRM_HIP it RETURNS from the enclosing function with the error.
// tests/launch_dispatch.cpp defines the macro before this header, to count launches instead of making them (no kernel is instantiated
// there); a replacement must stay a single statement and may only return an error code from the enclosing function.
#ifndef TRM_LAUNCH
#define TRM_LAUNCH(c, K, grid, block, ...)                                     \
    do {                                                                       \
        hipLaunchKernelGGL(K, grid, block, 0, (c)->stream, __VA_ARGS__);       \
        TRM_HIP(c, hipGetLastError());                                         \
    } while (0)
#endif
// whether a step launch stores the hydraulic conductivity: the finalizing one, or every one under TRM_OPT_WRITE_KF_EVERY_STEP
inline int write_kf(const trm_ctx* c, int finalize) { return (c->opt_write_kf || finalize) ? 1 : 0; }
// The arguments of a column program launch: `nsteps` steps of program `prog` (PROG_*), the stage's temperature boundary values
// (Heun: evaluated at t + dt), the multi-step program's series table, and for the Heun of the vegetation-coupled LandModel the
// stage's soil state, which the 0-D processes evaluated at the stage read (null otherwise)
template <class NF> ColumnArgs<NF> column_args(trm_ctx* c, double dt, int finalize, int nsteps, int prog) {
    const LaunchArgs<NF>& la = launch_args<NF>(c);
    ColumnArgs<NF> a{};
    a.dt = (NF)dt;
    a.finalize = finalize;
    a.write_kf = write_kf(c, finalize);
    a.nsteps = nsteps;
    a.bcT_bot_stage = la.w.bcT_bot;
    a.bcT_top_stage = la.w.bcT_top;
    a.series = (const SeriesTable<NF>*)c->d_series_table;
    a.series_rows = (const SeriesRow*)c->d_series_rows;
    a.nseries = (int)c->series.size();
    a.store_closure = 1;      // (0: StepPlan::store_closure, taken over by the launchers of the deriving per-step instances alone)
    if (prog == PROG_HEUN && Policy<NF>::coupled(c)) {
        a.stage_sat = (NF*)c->stage.f[TRM_FIELD_SATURATION_WATER_ICE];
        a.stage_liq = (NF*)c->stage.f[TRM_FIELD_LIQUID_WATER_FRACTION];
        a.stage_T = (NF*)c->stage.f[TRM_FIELD_TEMPERATURE];
        a.stage_S = (NF*)c->stage.f[TRM_FIELD_SURFACE_EXCESS_WATER];
    }
    return a;
}

// One fused step launch, decided once (StepPolicy::plan_step, below) and handed to the launcher: the route of Ops::step_launch, in the order it is
// tried, and -- for ForwardEuler on k_column / k_column_land, which have an instance per value; the other launches keep the plain form below -- what is
// derived, how the per-column values travel (after Policy::io_paths), the boundary signature (-1: kinds read at run time), whether T / liq are
// stored, how the pressure head arrives and leaves (PSI_*; `check_entry`: the launch before was an interior launch).  `derives_unread`: a deriving
// k_column / k_column_land launch of every column, which reads neither T nor liq from memory; `psi_step`: a k_column / k_column_psi launch of a Richards state.
enum StepRoute { ROUTE_SURFACE_IN_LAUNCH, ROUTE_ACCUM_IN_LAUNCH, ROUTE_LEVELS, ROUTE_PACKED, ROUTE_GENERIC, ROUTE_COLUMN };
struct StepPlan {
    StepRoute route = ROUTE_COLUMN;
    int derive = DERIVE_NONE, staged = 0, scalar_in = 1, sig = -1, store_closure = 1, psi_form = PSI_STORED, check_entry = 0;
    bool derives_unread = false, psi_step = false;
    const char* refusal = nullptr;      // the context cannot take the launch the call needs here (the caller fails with this text)
};

// ---- the launchers: declared here, defined and explicitly instantiated in the trm_launch_*.hip files ------------------------
// reference-order kernels, the 0-D surface kernel, update_inputs! of the time series (trm_launch_unfused.hip)
template <class NF> struct Unfused {
    static int await_levels(trm_ctx* c, trm_ctx::Series& sr, int last_level);
    static int update_inputs(trm_ctx* c, const FieldSet& s, double time);
    // the slot table and the rows of a multi-step launch with time series; `keep` / `kept`: the tape of trm_step_record
    static int upload_series_rows(trm_ctx* c, double dt, int nsteps, std::vector<SeriesRow>* keep = nullptr, const SeriesRow* kept = nullptr);
    static int hydraulics(trm_ctx* c, const FieldSet& s);
    static int surface(trm_ctx* c, const FieldSet& s, bool from_state = false);
    static int compute_auxiliary(trm_ctx* c, const FieldSet& s);
    static int compute_tendencies(trm_ctx* c, const FieldSet& s);
    static int reset_tendencies(trm_ctx* c, const FieldSet& s);
    static int update_state(trm_ctx* c, const FieldSet& s, bool tendencies);
    static int explicit_step(trm_ctx* c, const FieldSet& s, double dt);
    static int closure_hydrology(trm_ctx* c, const FieldSet& s, bool with_psi, bool with_adjust = true);
    static int closure(trm_ctx* c, const FieldSet& s);
    static int invclosure(trm_ctx* c, const FieldSet& s);
    static int initialize(trm_ctx* c);
    static int average(trm_ctx* c, int field);
};
// vegetation and the vegetation-coupled surface kernel (trm_launch_vegetation.hip)
template <class NF> struct Veg {
    static int surface_veg(trm_ctx* c, const FieldSet& s, bool from_state, bool advance, double dt, bool store_paw = true);
    static int surface_veg_launch(trm_ctx* c, const View<NF>& v, const VegView<NF>& vv, const SurfaceVegArgs<NF>& a);
    static int vegetation(trm_ctx* c, const FieldSet& s, int mode, double dt, int nsteps, int finalize);   // k_vegetation<MODE>
    static int plant_available_water(trm_ctx* c, const FieldSet& s, bool store_paw);
    static int heun_average_0d(trm_ctx* c, const VegView<NF>& vs, const VegView<NF>& vg, double dt);
};
// the register-resident column programs k_column (trm_launch_column*.hip: one file per precision x program)
template <class NF, bool RICH, int PROG> struct ColumnLaunch { static int run(trm_ctx* c, const StepPlan& plan, double dt, int finalize, int nsteps); };
// the multi-step program with time averages accumulated in the launch (trm_launch_column_accum_*.hip)
template <class NF, bool RICH> struct ColumnAccumLaunch { static int run(trm_ctx* c, double dt, int finalize, int nsteps, const AccumArgs& acc); };
// ---- the derivative families of the heat-only fp64 run (trm_launch_derivative.inl) --------------------------------------------------
// What rides along with a tangent step or a backward sweep is a Ride (trm_kernels.hpp); RECORD: the launch is the record twin of its
// kernel, which samples the tangent record (k_column_tangent_record) or reads the attached temperature record (k_column_adjoint_record,
// k_column_adjoint_ckpt_record) -- the same preconditions and arguments plus the record's, the same TRM_INFO_LAST_PROGRAM.  The launchers,
// one explicit instantiation per ride in trm_launch_column_{tangent,adjoint,adjoint_ckpt}{,_record}{,_bc,_param,_series,_param_series}.hip
// (the two series records in trm_launch_column_adjoint_series.hip: the record carries no derivative, so both series rides share it)
constexpr bool NO_RECORD = false, WITH_RECORD = true;
template <Ride R, bool RECORD> int tangent_step(trm_ctx* c, double dt, int nsteps);
template <Ride R> int tangent_closure(trm_ctx* c);
template <bool STRIDED, bool SERIES> int adjoint_record(trm_ctx* c, double dt, int nsteps, int slot, int first, int every);
// (`first`: the taped position of the launch's first step, read with RECORD alone)
template <bool CKPT, Ride R, bool RECORD> int adjoint_backward(trm_ctx* c, double dt, int nsteps, int slot, int fold, int first);
// (the heat + Richards sweep: AdjointRichLaunch below)
template <bool PARAMS, bool RECORD> int adjoint_backward_rich(trm_ctx* c, double dt, int nsteps, int slot, int fold);
// k_column_tangent{,_record} / k_closure_tangent (fp64 NoFlow only); the closure knows the parameter seeds alone.  These choose the
// instantiation of the ride, with a record or without (ride_launch, trm_derivative_api.hip)
struct TangentLaunch {
    static int step(trm_ctx* c, double dt, int nsteps, Ride ride, bool record);
    static int closure(trm_ctx* c, Ride ride);
};
// k_column_tangent_rich / k_closure_tangent_rich (fp64 heat + Richards, state seeds alone: TRM_OPT_DERIVATIVE_RICHARDS), both in
// trm_launch_column_tangent_rich.hip
struct TangentRichLaunch {
    static int step(trm_ctx* c, double dt, int nsteps);
    static int closure(trm_ctx* c);
};
// The heat + Richards adjoint (fp64, final-state cotangents on the per-step tape alone: TRM_OPT_DERIVATIVE_RICHARDS_ADJOINT); `slot` is
// the tape slot of the launch's first step, and its taped position.  record: k_column_record_rich (trm_launch_column_adjoint_rich.hip).
// backward: the sweep, one device program behind four kernels -- `params`: with the hydraulic-parameter gradients, `record`: reading the
// attached soil-moisture record -- which chooses among the four instantiations of adjoint_backward_rich, one in each of
// trm_launch_column_adjoint_rich{,_param,_record,_param_record}.hip (trm_derivative_api.hip).  param_reduce: k_hyd_param_reduce, which
// ends a sweep with `params` (trm_launch_column_adjoint_rich_param.hip)
struct AdjointRichLaunch {
    static int record(trm_ctx* c, double dt, int nsteps, int slot);
    static int backward(trm_ctx* c, double dt, int nsteps, int slot, int fold, bool params, bool record);
    static int param_reduce(trm_ctx* c);
};
// the row of a TRM_HYDRAULIC_PARAM_* id in the result [TRM_HYDRAULIC_PARAM_COUNT][Nh], -1 for any other number (the thermal ids, which
// the hydraulic ones count on from, included)
inline int hyd_param_row(int which) {
    static_assert(TRM_HYDRAULIC_PARAM_K_SAT == TRM_THERMAL_PARAM_COUNT, "one id space with the thermal ids");
    const int row = which - TRM_HYDRAULIC_PARAM_K_SAT;
    return row >= 0 && row < TRM_HYDRAULIC_PARAM_COUNT ? row : -1;
}
// k_column_record / k_column_adjoint{,_record} (fp64 NoFlow only): `slot` is the tape slot of the launch's first step; k_param_reduce ends
// a sweep with parameter gradients on either tape (trm_launch_column_adjoint_param.hip)
struct AdjointLaunch {
    static int record(trm_ctx* c, double dt, int nsteps, int slot, bool series);
    static int backward(trm_ctx* c, double dt, int nsteps, int slot, int fold, Ride ride, bool record, int first);
    static int param_reduce(trm_ctx* c);
};
// the strided k_column_record / k_column_adjoint_ckpt{,_record}: the record stores before the steps `first`, `first + every`, ... of the
// launch into the slots from `slot` on; the backward launch pulls lam through the segment of `nsteps` steps whose checkpoint is in `slot`
struct CheckpointLaunch {
    static int record(trm_ctx* c, double dt, int nsteps, int slot, int first, int every, bool series);
    static int backward(trm_ctx* c, double dt, int nsteps, int slot, int fold, Ride ride, bool record, int first);
};
// The tape of trm_step_record as the host keeps it (trm_ctx::tape_dt, or tape_segs when checkpointed): bookkeeping alone, no HIP call
// (tests/derivative_preconditions.cpp).  Steps on the tape:
inline int taped_steps(const trm_ctx* c) {
    if (c->ckpt_interval == 0) return (int)c->tape_dt.size();
    return c->tape_segs.empty() ? 0 : c->tape_segs.back().first + c->tape_segs.back().len;
}
// the steps the open segment of a checkpointed tape still takes under `dt` (0: the next step opens a segment)
inline int open_segment_room(const trm_ctx* c, double dt) {
    if (c->tape_segs.empty() || c->tape_segs.back().dt != dt || c->tape_seg_closed) return 0;   // (closed: by an observation at its end)
    return c->ckpt_interval - c->tape_segs.back().len;
}
// slots taken, and the slots `nsteps` more steps under `dt` take: one each on the per-step tape; checkpointed, the steps the open segment
// has no room for, K to a slot
inline long long tape_slots_used(const trm_ctx* c) { return c->ckpt_interval ? (long long)c->tape_segs.size() : (long long)c->tape_dt.size(); }
inline long long tape_slots_needed(const trm_ctx* c, double dt, int nsteps) {
    const long long K = c->ckpt_interval, room = open_segment_room(c, dt);
    if (K == 0) return nsteps;
    return nsteps > room ? (nsteps - room + K - 1) / K : 0;
}
// `m` recorded steps under `dt` join the tape: they fill the open segment, then open segments of up to K steps in the next slots
inline void tape_append(trm_ctx* c, double dt, int m) {
    const int K = c->ckpt_interval;
    if (K == 0) {
        c->tape_dt.insert(c->tape_dt.end(), (size_t)m, dt);
        return;
    }
    int at = taped_steps(c);
    const int fill = std::min(open_segment_room(c, dt), m);
    if (fill > 0) c->tape_segs.back().len += fill;
    for (m -= fill, at += fill; m > 0; m -= std::min(K, m), at += K) {
        c->tape_segs.push_back({at, std::min(K, m), dt, (int)c->tape_segs.size()});
        c->tape_seg_closed = false;    // (a new segment is open)
    }
}
// Adjoint observations (trm_launch_observe.hip).  misfit: 1/2 w (T - T_obs)^2 of the stored temperature on the observed levels onto
// d_misfit, at registration.  inject: the observation's cotangent through the closure at U_p (`U_p` null: the context's U) onto lU
// (`lam`) and, with a parameter gradient open, through the heat capacity of that closure onto the per-cell parameter sums (`params`).
// Neither writes TRM_INFO_LAST_PROGRAM.
struct ObserveLaunch {
    static int misfit(trm_ctx* c, const trm_ctx::Observation& o);
    static int inject(trm_ctx* c, const trm_ctx::Observation& o, const double* U_p, bool lam, bool params);
};
// ---- the position table of a record (RecordTable; trm_ctx::rec, trm_ctx::trec) -- bookkeeping alone, no HIP call
// (tests/record_preconditions.cpp) ----
// row_of_level[Nz]: the row of the record's level list a level has, -1 for a level it does not observe
inline std::vector<int32_t> record_level_table(int Nz, const std::vector<int>& levels) {
    std::vector<int32_t> t((size_t)Nz, -1);
    for (size_t j = 0; j < levels.size(); ++j) t[(size_t)levels[j]] = (int32_t)j;
    return t;
}
// row_of_position[n + 1] of a run of n steps: the row of the record a position has, -1 without a sample.  Positions behind n have no
// entry (the sweep refuses them first, record_fits_tape)
inline std::vector<int32_t> record_position_table(int n, const std::vector<int>& positions) {
    std::vector<int32_t> t((size_t)n + 1, -1);
    for (size_t k = 0; k < positions.size(); ++k)
        if (positions[k] <= n) t[(size_t)positions[k]] = (int32_t)k;
    return t;
}
// What an attach checks of the caller's lists, in the words of the neighbouring calls: `counts` is what the positions count
// ("taped-step", "tangent-step")
inline int record_lists_ok(trm_ctx* c, int npos, const int32_t* positions, int nlevels, const int32_t* levels, const char* counts, const std::string& who) {
    for (int k = 0; k < npos; ++k)
        if (positions[k] < 0 || (k > 0 && positions[k] <= positions[k - 1]))
            return fail(c, TRM_EINVAL, who + ": the positions are " + counts + " counts >= 0, strictly increasing");
    for (int j = 0; j < nlevels; ++j)
        if (levels[j] < 0 || levels[j] >= c->Nz || (j > 0 && levels[j] <= levels[j - 1]))
            return fail(c, TRM_EINVAL, who + ": the levels are rows 0 ... " + std::to_string(c->Nz - 1) + " of the host layout, strictly increasing");
    return TRM_OK;
}
// what an attach leaves: the lists, no table yet
inline void record_table_attach(RecordTable& t, int npos, const int32_t* positions, int nlevels, const int32_t* levels) {
    t.positions.assign(positions, positions + npos);
    t.levels.assign(levels, levels + nlevels);
    t.npos = npos;
    t.nlevels = nlevels;
    t.entries = 0;
}
// the staging copy of the tables for the positions 0 ... last.  It replaces the one before: no upload of that may be in flight
inline void record_table_build(RecordTable& t, int Nz, int last) {
    t.host = record_level_table(Nz, t.levels);
    const std::vector<int32_t> rows = record_position_table(last, t.positions);
    t.host.insert(t.host.end(), rows.begin(), rows.end());
    t.entries = last + 1;
}
// the device tables as a launch whose first state is position `first` sees them
inline const int32_t* record_row_of_level(const RecordTable& t) { return (const int32_t*)t.d_tables; }
inline const int32_t* record_row_of_position(const RecordTable& t, int Nz, long long first) { return (const int32_t*)t.d_tables + Nz + first; }
// a launch of `nsteps` steps from position `first` reads the entries first ... first + nsteps: all inside the table
inline bool record_table_covers(const RecordTable& t, long long first, int nsteps) { return first >= 0 && nsteps >= 0 && first + nsteps < (long long)t.entries; }
inline int64_t record_table_bytes(const RecordTable& t, int Nz) { return ((int64_t)Nz + t.entries) * 4; }
// nothing attached.  The device tables are the caller's to free first (drop_table, trm_derivative_api.hip)
inline void record_table_drop(RecordTable& t) { t = RecordTable{}; }

// ---- attached records (trm_adjoint_observe_record*; trm_launch_record.hip) ----
// what the library holds for an attached record: the tables, the residuals and the misfit, and its copies of a host record
inline int64_t record_bytes(const trm_ctx* c) {
    if (c->rec.npos == 0) return 0;
    const int64_t cells = (int64_t)c->rec.npos * c->rec.nlevels * (int64_t)c->Nh * 8;
    const int64_t owned = c->d_rec_owned ? cells * (c->d_rec_weight ? 2 : 1) : 0;
    return owned + cells + (int64_t)c->Nh * 8 + record_table_bytes(c->rec, c->Nz);
}
// What an attach checks before it touches the device, in the words of the neighbouring calls.  `host_weight`: the weights of the host
// form (null: none given, or the device form, whose weights the library cannot read)
inline int record_attach_ok(trm_ctx* c, int npos, const int32_t* positions, int nlevels, const int32_t* levels, const void* observed, const double* host_weight,
                            const char* who) {
    const std::string w(who);
    if (!c->d_adj[0]) return fail(c, TRM_EINVAL, w + ": no adjoint is open (trm_adjoint_open)");
    if (npos < 1 || nlevels < 1 || !positions || !levels || !observed) return fail(c, TRM_EINVAL, w + ": bad argument (npos >= 1 positions, nlevels >= 1 levels, the observed temperatures)");
    if (int rc = record_lists_ok(c, npos, positions, nlevels, levels, "taped-step", w)) return rc;
    if (host_weight)
        for (size_t q = 0, end = (size_t)npos * (size_t)nlevels * (size_t)c->Nh; q < end; ++q)
            if (!(host_weight[q] >= 0.0)) return fail(c, TRM_EINVAL, w + ": a weight is negative or NaN");
    if (c->rec.npos) return fail(c, TRM_EINVAL, w + ": a record is attached already (trm_adjoint_record_detach)");
    if (!c->observations.empty())
        return fail(c, TRM_EINVAL, w + ": per-position observations are registered (trm_adjoint_observe, trm_adjoint_observe_misfit): the two paths do not mix");
    return TRM_OK;
}
// trm_adjoint_observe / trm_adjoint_observe_misfit while a record is attached
inline int record_excludes_observations(trm_ctx* c, const char* who) {
    if (c->rec.npos == 0) return TRM_OK;
    return fail(c, TRM_EINVAL, std::string(who) + ": a temperature record is attached (trm_adjoint_observe_record): the two paths do not mix");
}
// a sweep over a tape of n steps: every position of the record is on it
inline int record_fits_tape(trm_ctx* c, int n, const char* who) {
    if (c->rec.npos == 0 || c->rec.positions.back() <= n) return TRM_OK;
    return fail(c, TRM_EINVAL, std::string(who) + ": the attached record is longer than the tape: position " + std::to_string(c->rec.positions.back()) + " of " +
                                   std::to_string(n) + " taped steps");
}
// the residuals and the misfit are those of a sweep with this record
inline int record_results_ok(trm_ctx* c, const void* ptr, const char* who) {
    const std::string w(who);
    if (!c->d_adj[0]) return fail(c, TRM_EINVAL, w + ": no adjoint is open (trm_adjoint_open)");
    if (!ptr) return fail(c, TRM_EINVAL, w + ": bad argument");
    if (c->rec.npos == 0) return fail(c, TRM_EINVAL, w + ": no record is attached (trm_adjoint_observe_record)");
    if (!c->rec_swept) return fail(c, TRM_EINVAL, w + ": no sweep has run with this record (trm_adjoint_backward)");
    return TRM_OK;
}
// A heat + Richards context under TRM_OPT_DERIVATIVE_RICHARDS_ADJOINT: the calls its adjoint does not cover are refused before anything
// else happens.  `record_call`: the caller is one of the seven attached-record calls, which TRM_OPT_DERIVATIVE_RICHARDS_RECORD opens to such
// a context (a soil-moisture record, DESIGN 4.8 "Richards records"); with either option at 0 every call answers as without it
inline const char* const kRichardsTapeOnly = "on a Richards context: final-state cotangents on a per-step tape only";
inline bool richards_record_enabled(const trm_ctx* c) {
    return c->params.flow == TRM_FLOW_RICHARDS && c->opt_derivative_richards_adjoint && c->opt_derivative_richards_record;
}
inline int richards_tape_only(trm_ctx* c, const char* who, bool record_call = false) {
    if (c->params.flow != TRM_FLOW_RICHARDS || !c->opt_derivative_richards_adjoint) return TRM_OK;
    if (record_call && richards_record_enabled(c)) return TRM_OK;
    return fail(c, TRM_EUNSUPPORTED, std::string(who) + ": " + kRichardsTapeOnly);
}
// k_record_misfit, which sums the residuals a sweep wrote into the misfit per column (trm_launch_record.hip)
struct RecordLaunch {
    static int misfit(trm_ctx* c);
};
// ---- tangent records (trm_tangent_record_*) -- bookkeeping alone, no HIP call (tests/tangent_record_preconditions.cpp) ----
// The last position a record launch may reach: the record's last position -- or 1 for a record of position 0 alone, whose sample is the
// entry's of a launch that has a step to run (its table has two entries)
inline int tangent_record_limit(const std::vector<int>& positions) { return std::max(positions.back(), 1); }
// What an attach checks before it touches the device (the caller has checked that the derivatives cover the context)
inline int tangent_record_attach_ok(trm_ctx* c, int npos, const int32_t* positions, int nlevels, const int32_t* levels, const char* who) {
    const std::string w(who);
    if (!c->d_tan[0]) return fail(c, TRM_EINVAL, w + ": no tangent is open (trm_tangent_open)");
    if (npos < 1 || nlevels < 1 || !positions || !levels) return fail(c, TRM_EINVAL, w + ": bad argument (npos >= 1 positions, nlevels >= 1 levels)");
    if (int rc = record_lists_ok(c, npos, positions, nlevels, levels, "tangent-step", w)) return rc;
    if (c->trec.npos) return fail(c, TRM_EINVAL, w + ": a record is attached already (trm_tangent_record_detach)");
    return TRM_OK;
}
// the calls that need an attached record
inline int tangent_record_attached(trm_ctx* c, const char* who) {
    const std::string w(who);
    if (!c->d_tan[0]) return fail(c, TRM_EINVAL, w + ": no tangent is open (trm_tangent_open)");
    if (c->trec.npos == 0) return fail(c, TRM_EINVAL, w + ": no record is attached (trm_tangent_record_attach)");
    return TRM_OK;
}
// Of the next `m` tangent steps, the ones a record launch runs: those up to the last position (0: the launch samples nothing and is the
// record-free kernel's).  A launch never runs past the position table: the steps behind it are a launch of their own.
inline int tangent_record_steps(const trm_ctx* c, int m) {
    if (c->trec.npos == 0 || c->trec_position >= (long long)tangent_record_limit(c->trec.positions)) return 0;
    return (int)std::min<long long>(m, (long long)tangent_record_limit(c->trec.positions) - c->trec_position);
}
// what the library holds for a tangent record: both sample arrays and the tables
inline int64_t tangent_record_bytes(const trm_ctx* c) {
    if (c->trec.npos == 0) return 0;
    return 2 * (int64_t)c->trec.npos * c->trec.nlevels * (int64_t)c->Nh * 8 + record_table_bytes(c->trec, c->Nz);
}
// The chain rule between the ten thermal parameters (TRM_THERMAL_PARAM_*, the order of trm_params) and the eight numbers the kernels
// differentiate (make_dev_params): w[q] = d(derived number) / d(parameter q), with sk_i = sqrt(k_i), s0 = sqrt(k_mineral) frac_mineral +
// sqrt(k_organic) frac_organic, C0 = c_mineral frac_mineral + c_organic frac_organic.  Parameter q feeds derived number
// thermal_param_target(q).  Forward for seeds, transposed for gradients (k_param_reduce), with the same factors.
inline int thermal_param_target(int q) {
    const int to[10] = {0, 1, 2, 3, 3, 4, 5, 6, 7, 7};
    return to[q];
}
inline void thermal_param_chain(const trm_params& q, const trm::DevParams<double>& p, double w[10]) {
    w[0] = 1.0 / (2.0 * p.sk_water);
    w[1] = 1.0 / (2.0 * p.sk_ice);
    w[2] = 1.0 / (2.0 * p.sk_air);
    w[3] = p.frac_mineral / (2.0 * std::sqrt(q.k_mineral));
    w[4] = p.frac_organic / (2.0 * std::sqrt(q.k_organic));
    w[5] = w[6] = w[7] = 1.0;
    w[8] = p.frac_mineral;
    w[9] = p.frac_organic;
}
// k_materialize_closure (trm_launch_materialize.hip)
template <class NF> struct MaterializeLaunch { static int run(trm_ctx* c); };
// k_accumulate (trm_launch_average.hip)
template <class NF> struct AverageLaunch { static int accumulate(trm_ctx* c, const AccumBatch& b); };
// What a launcher's return code starts as: the callbacks of its dispatch (trm_dispatch.hpp) assign it the launch's; where none ran, no
// instance takes the values and the launcher refuses
constexpr int NO_INSTANCE = -1;
inline int launched(trm_ctx* c, int rc, const char* refusal) { return rc == NO_INSTANCE ? fail(c, TRM_EINVAL, refusal) : rc; }
// ---- one launch function per kernel template of the column program: it launches the instance and records TRM_INFO_LAST_PROGRAM from the
// instance's own template arguments, so the id cannot disagree with what ran
template <class NF, bool RICH, int H, int LPC, int DERIVE, int PROG, bool SEB = false, bool SERIES = false, bool STAGED = false, bool SCALAR_IN = true, int BCSIG = BCSIG_RUNTIME>
int run_column(trm_ctx* c, dim3 grid, dim3 block, const View<NF>& v, const DevParams<NF>& p, const ColumnArgs<NF>& a) {
    TRM_LAUNCH(c, (k_column<NF, RICH, H, LPC, DERIVE, PROG, SEB, SERIES, STAGED, SCALAR_IN, BCSIG>), grid, block, v, p, a);
    constexpr int family = PROG == PROG_EULER ? TRM_PROGRAM_COLUMN_EULER : PROG == PROG_HEUN ? TRM_PROGRAM_COLUMN_HEUN : TRM_PROGRAM_COLUMN_MULTI;
    c->last_program = program_id(family, H, LPC, DERIVE, STAGED, SCALAR_IN, BCSIG) | (SEB ? 1 << 25 : 0) | (SERIES ? 1 << 26 : 0);
    return TRM_OK;
}
// (the one exception: k_column_psi reports the id of the k_column signature instance it stands in for)
template <int H, int LPC, bool STAGED, bool SCALAR_IN, int BCSIG, int PSI>
int run_column_psi(trm_ctx* c, dim3 grid, dim3 block, const View<double>& v, const DevParams<double>& p, const ColumnArgs<double>& a) {
    TRM_LAUNCH(c, (k_column_psi<H, LPC, STAGED, SCALAR_IN, BCSIG, PSI>), grid, block, v, p, a);
    c->last_program = program_id(TRM_PROGRAM_COLUMN_EULER, H, LPC, DERIVE_T_LIQ, STAGED, SCALAR_IN, BCSIG);
    return TRM_OK;
}
// (the id of the PROG_MULTI instance of k_column with the same arguments + the bit of the accumulation in the launch)
template <class NF, bool RICH, int H, int LPC, bool SEB, bool SERIES>
int run_column_accum(trm_ctx* c, dim3 grid, dim3 block, const View<NF>& v, const DevParams<NF>& p, const ColumnArgs<NF>& a, const AccumArgs& acc) {
    TRM_LAUNCH(c, (k_column_accum<NF, RICH, H, LPC, SEB, SERIES>), grid, block, v, p, a, acc);
    c->last_program = program_id(TRM_PROGRAM_COLUMN_MULTI, H, LPC, DERIVE_NONE, 0, 1, BCSIG_RUNTIME) | (SEB ? 1 << 25 : 0) | (SERIES ? 1 << 26 : 0) | TRM_PROGRAM_AVERAGES_IN_LAUNCH;
    return TRM_OK;
}
template <int H, int LPC, int DERIVE, bool STAGED, bool SCALAR_IN, int PROG>
int run_column_land(trm_ctx* c, dim3 grid, dim3 block, const View<double>& v, const DevParams<double>& p, const ColumnArgs<double>& a, const FrontArgs& fa) {
    TRM_LAUNCH(c, (k_column_land<double, true, H, LPC, DERIVE, STAGED, SCALAR_IN, PROG>), grid, block, v, p, a, fa);
    c->last_program = program_id(TRM_PROGRAM_COLUMN_LAND, H, LPC, DERIVE, STAGED, SCALAR_IN, BCSIG_LAND) | (PROG << 25);
    return TRM_OK;
}
// The k_column instances with the boundary-condition signature compiled in (BCSIG, trm_kernels.hpp; fp64, the two compiled hydraulics), one
// explicit instantiation per signature of kSignatures (trm_dispatch.hpp).  Each run returns TRM_EINVAL where the values name no instance.
// ForwardEuler, with the derivation of T / liq or without it (trm_launch_column_sig_*.hip):
template <class NF, bool RICH, int SIG> struct ColumnSigLaunch {
    static int run(trm_ctx* c, dim3 grid, dim3 block, const View<NF>& v, const DevParams<NF>& p, const ColumnArgs<NF>& a, int derive, int staged, int scalar_in);
};
// the fp64 Richards instances that derive the pressure head at entry (k_column_psi<..., PSI_LAST | PSI_INTERIOR>, trm_launch_column_psi_f64_*.hip):
// `form` is PSI_LAST or PSI_INTERIOR, (staged, scalar_in) one of (0, 1), (1, 0)
template <int SIG> struct ColumnPsiLaunch {
    static int run(trm_ctx* c, dim3 grid, dim3 block, const View<double>& v, const DevParams<double>& p, const ColumnArgs<double>& a, int form, int staged, int scalar_in);
};
// the one-launch Heun program (trm_launch_column_sig_heun_*.hip)
template <class NF, bool RICH, int SIG> struct ColumnSigHeunLaunch {
    static int run(trm_ctx* c, dim3 grid, dim3 block, const View<NF>& v, const DevParams<NF>& p, const ColumnArgs<NF>& a);
};
// generic boundary kinds: k_step_wave (Euler) and k_heun_generic (trm_launch_generic*.hip)
template <class NF> struct GenericLaunch {
    static int step(trm_ctx* c, double dt, int finalize);
    static int heun(trm_ctx* c, double dt, int finalize);
};
// columns of 65 ... 256 levels, M levels per lane: k_column_deep (M = 2: trm_launch_deep_f64.hip / _f32.hip) and k_column_wide
// (M = 4: trm_launch_wide_f64.hip / _f32.hip)
template <class NF, int M> struct LevelsLaunch { static int run(trm_ctx* c, int prog, bool generic, double dt, int finalize, int nsteps); };
// the launch of the context's M (Policy::levels_per_lane: 2 or 4)
template <class NF> inline int levels_launch(trm_ctx* c, int prog, bool generic, double dt, int finalize, int nsteps = 1) {
    return Policy<NF>::levels_per_lane(c) == 4 ? LevelsLaunch<NF, 4>::run(c, prog, generic, dt, finalize, nsteps) : LevelsLaunch<NF, 2>::run(c, prog, generic, dt, finalize, nsteps);
}
// interleaved LandModel launches: k_land_euler (fp64, trm_launch_land.hip) / k_land_pk (fp32, trm_launch_packed.hip)
template <class NF> struct LandLaunch { static int run(trm_ctx* c, int qcol, int qsurf, double dt, int finalize, bool top_arrays); };
template <> int LandLaunch<double>::run(trm_ctx* c, int qcol, int qsurf, double dt, int finalize, bool top_arrays);
template <> int LandLaunch<float>::run(trm_ctx* c, int qcol, int qsurf, double dt, int finalize, bool top_arrays);
// the packed fp32 step k_step_pk (trm_launch_packed.hip)
struct PackedLaunch {
    static int step(trm_ctx* c, double dt, int finalize);
    static int step_land(trm_ctx* c, double dt, int finalize);      // k_step_pk_land: the surface processes in the launch
};
// The hand-off of a launch that carries its own surface processes (k_column_land, k_step_pk_land; defined in trm_context_api.hip):
// refused unless the top-cell arrays are current (the surface workgroups read them), then the granule buffer, the launch's epoch
// and the number of surface workgroups in front of the column workgroups.  `kernel` names the launch in the refusal.
int front_args(trm_ctx* c, const char* kernel, FrontArgs& fa);
// the LandModel's per-step launch with the surface processes in its first workgroups: k_column_land (fp64; trm_launch_column_land_*.hip)
struct FrontLaunch {
    static int run(trm_ctx* c, const StepPlan& plan, double dt, int finalize, bool heun = false);
    template <int H> static int run_hyd(trm_ctx* c, const StepPlan& plan, double dt, int finalize, bool heun);
};

// (measured: profiles/r04/coupling_exchange.log)
#ifndef TRM_SINGLE_STEP_PROGRAM_MAX_COLUMNS
#define TRM_SINGLE_STEP_PROGRAM_MAX_COLUMNS 0
#endif

// time averages: the fused path's slot of a field (trm_average.hpp), -1 for a field it does not carry, and back
constexpr int kAccumField[ACC_SLOTS] = {
    TRM_FIELD_INTERNAL_ENERGY, TRM_FIELD_SATURATION_WATER_ICE, TRM_FIELD_TEMPERATURE, TRM_FIELD_LIQUID_WATER_FRACTION, TRM_FIELD_PRESSURE_HEAD,
    TRM_FIELD_SURFACE_EXCESS_WATER, TRM_FIELD_WATER_TABLE, TRM_FIELD_SKIN_TEMPERATURE, TRM_FIELD_GROUND_HEAT_FLUX, TRM_FIELD_SURFACE_SHORTWAVE_UP,
    TRM_FIELD_SURFACE_LONGWAVE_UP, TRM_FIELD_SURFACE_NET_RADIATION, TRM_FIELD_SENSIBLE_HEAT_FLUX, TRM_FIELD_LATENT_HEAT_FLUX,
    TRM_FIELD_EVAPORATION_GROUND, TRM_FIELD_INFILTRATION, TRM_FIELD_SURFACE_RUNOFF};
inline int accum_slot(int field) {
    for (int s = 0; s < ACC_SLOTS; ++s) if (kAccumField[s] == field) return s;
    return -1;
}
inline int accum_field(int slot) { return kAccumField[slot]; }

// ---- the pure predicates of the step sequences (Ops, trm_step_api.hip) and the StepPlan they give: no HIP call (tests/step_plan_preconditions.cpp)
template <class NF> struct StepPolicy : Policy<NF> {
    using P = Policy<NF>;
    // the top-cell arrays (LandModel: T, sat, liq of the top cell, [Nh] each) can describe the state: they exist and no device
    // pointer to T / sat / liq has been handed out.  Every "the next surface evaluation may read the arrays" decision goes
    // through here -- a launch with TOP_ARRAYS on a context without them would read through a null pointer.
    static bool tops_current(const trm_ctx* c) { return c->d_top3 != nullptr && !c->top_escaped; }
    static bool averaging(const trm_ctx* c) {
        for (const auto& a : c->averages) if (a.field >= 0) return true;
        return false;
    }
    // The multi-step program accumulates in its own launch when it covers every open accumulator's field (the surface excess water
    // and the water table only under Richards: the NoFlow program does not carry them) -- columns of <= 64 levels.
    static bool averages_in_launch(const trm_ctx* c) {
        if (c->Nz > 64 || c->part >= 0) return false;
        for (const auto& a : c->averages) {
            if (a.field < 0) continue;
            const int s = accum_slot(a.field);
            if (s < 0 || (!P::richards(c) && (s == ACC_S || s == ACC_WT))) return false;
        }
        return true;
    }
    // A launch that reads neither T nor liq (StepPlan::derives_unread) may leave them unstored (ColumnArgs::store_closure = 0): nothing reads the arrays before the next flush_closure -- no
    // open time average of either (accumulate_after reads them), no tangent state, and on a LandModel the top-cell arrays are what the
    // surface processes read (fused_epilogue's included).
    static bool defer_closure_now(const trm_ctx* c, bool derives_unread) {
        if (!c->opt_defer_closure || c->d_tan[0] || !derives_unread) return false;
        for (const auto& a : c->averages)
            if (a.field == TRM_FIELD_TEMPERATURE || a.field == TRM_FIELD_LIQUID_WATER_FRACTION) return false;
        return !c->params.seb || tops_current(c);
    }
    // TRM_OPT_INTERIOR_STEPS: the context's per-step launch is one of the instances k_column_psi stands in for -- fp64, Richards, no
    // LandModel, one level per lane, every column, a compiled hydraulics and one of the non-LandModel signatures, T / liq derived --
    // and nothing reads a field between the launches of a call: no open time average (accumulate_after reads the arrays every step), no
    // tangent state, no device pointer handed out; and the stored pressure_head / water_table are a step launch's (psi_consistent).
    static bool interior_capable(const trm_ctx* c) {
        if (!std::is_same<NF, double>::value || !c->opt_interior || !c->psi_consistent || c->closure_escaped) return false;
        // 2, the library's rule: states within the Infinity Cache (the bound of Policy::scalar_inputs_now).  Beyond it the step gains more
        // (EXPERIMENTS R10.1), but bench.py's HBM-resident companion then reports a roofline fraction above 1 on its fixed 2 080 B per
        // column-step, which tests/test_gpu_full_size.py bounds: left to 1 until that yardstick is recalibrated
        if (c->opt_interior == 2 && (size_t)6 * (size_t)c->Nh * (size_t)c->Nzp * sizeof(NF) > ((size_t)256 << 20)) return false;
        if (!c->opt_write_kf) return false;      // (without TRM_OPT_WRITE_KF_EVERY_STEP the K array is the last finalizing launch's: left to the classic launches)
        if (!P::richards(c) || c->params.seb || P::coupled(c) || c->veg_mode == TRM_VEGETATION_STANDALONE) return false;
        if (c->opt_kernel != TRM_KERNEL_FUSED || P::levels_per_lane(c) != 1 || c->part >= 0 || P::generic_bcs(c)) return false;
        if (!c->opt_bc_signature || P::hyd(c) == HYD_GENERIC || !column_psi_supported(bc_signature_of(c))) return false;
        if (averaging(c) || c->d_tan[0]) return false;
        return P::template derive_now<true>(c) == DERIVE_T_LIQ;
    }
    // TRM_OPT_SURFACE_IN_LAUNCH: a per-step launch of this context can carry its own surface processes (k_column_land) -- a
    // bare-ground LandModel in fp64 on the branch-free program with the LandModel's boundary wiring, one level per lane, every
    // column in one launch, the top-cell arrays current (the surface workgroups read them).
    static bool surface_in_launch(const trm_ctx* c, bool heun = false) {
        if (c->opt_front == 0 || (heun && std::is_same<NF, float>::value)) return false;
        if (!c->params.seb || !P::richards(c) || P::coupled(c) || c->Nz > 64 || P::generic_bcs(c) || c->part >= 0) return false;
        if (c->opt_kernel != TRM_KERNEL_FUSED || !c->opt_bc_signature || bc_signature_of(c) != BCSIG_LAND) return false;
        if (P::hyd(c) != HYD_BC_LINEAR && P::hyd(c) != HYD_VG_N2) return false;
        if (!c->top_valid || !tops_current(c)) return false;
        const int d = heun ? DERIVE_NONE : P::template derive_now<true>(c);      // (the Heun program reads T / liq as stored)
        if (std::is_same<NF, float>::value ? !(P::packed_path(c) && (d == DERIVE_NONE || d == DERIVE_LIQ))         // k_step_pk_land
                                           : !(d == DERIVE_NONE || d == DERIVE_T_LIQ)) return false;             // k_column_land
        if (c->opt_front == 1) return true;
        // The library's rule (2).  What the single launch saves is the FIXED cost of the second launch (~3-4 us); the surface chain
        // itself is still evaluated, and the column waves of the first generation wait for it.  Measured, same box, pair -> one launch
        // (profiles/r05/exp3d_prio_sleep.log, exp4_packed_surface_in_launch.log, exp4b_in_launch_by_size.log): fp64 1 780 columns
        // 9.8 -> 7.1 us, 7 119 (the shard of BASELINE config 4) 11.1 -> 8.6, C4-VG shard 12.3 -> 9.2, 28 476 19.7 -> 19.3, N145
        // (56 951) 30.3 -> 29.6 ... 30.0; fp32 12 696 columns 15.2 -> 10.6, 50 782 29.5 -> 31.2, 203 125 108.6 -> 106.6, C5
        // (812 500) 425.4 -> 426.7, C5-VG 437.1 -> 451.0: a clear win where the step is launch-bound, nothing beyond.
        return c->Nh <= (std::is_same<NF, float>::value ? 32768 : 65536);
    }
    // TRM_OPT_SINGLE_STEP_PROGRAM: a bare-ground LandModel stepped ONE step per call (its inputs change every step: a coupled
    // atmosphere) takes the resident column program with the surface processes inline -- one launch instead of the
    // k_surface + k_column pair.  At N145 the pair wins by far (the inline surface balance runs on every lane of the column's
    // half-wave: C4 103.9 vs 34.1 us); on a shard of a few thousand columns the step is bound by launch latency and
    // the single launch wins.
    static bool single_step_program(const trm_ctx* c) {
        if (!c->params.seb || c->Nz > 64 || c->opt_single_step == 0) return false;
        if (c->opt_single_step == 1) return true;
        return c->Nh <= TRM_SINGLE_STEP_PROGRAM_MAX_COLUMNS;
    }
    // TRM_OPT_STEPS_PER_LAUNCH = 0: run!'s loop (model_integrator.jl:72-88) is exactly trm_step(ctx, dt, nsteps, 0), so the
    // resident-column program is what a plain call gets whenever it is legal.  Measured: 2.0-4.6 us per step
    // against 6.8-12 on N72 / 7 119-column shards, 12.3 against 24-26 at N145 -- and for fp32 contexts whose per-step path is
    // the packed kernel as well: C5 371 against 447-451 us, C5-VG 479 against 489, a 12 696-column fp32 shard 7.3 against 13.3
    // (r3: the rule used to keep the packed kernel there).
    static int auto_steps_per_launch(const trm_ctx*) { return 50; }
    // how many steps ONE launch of trm_step covers for this context: 1 unless the resident multi-step program applies
    static bool program_applies(const trm_ctx* c) {
        const bool fused = c->opt_kernel == TRM_KERNEL_FUSED && P::levels_per_lane(c) > 0;
        return fused && !P::generic_bcs(c) && !P::coupled(c) && c->veg_mode != TRM_VEGETATION_STANDALONE &&
               ((c->Nz <= 64 && P::series_fit_program(c)) || (P::levels_per_lane(c) == 2 && !c->params.seb && c->series.empty()));
    }
    // The plan of ONE fused launch of program `prog` (PROG_*) over the columns currently addressed, from the context and the two facts only Ops::step
    // knows: the launch is not its call's last (it may go interior); the one before it was interior (this one must derive psi at entry).
    static StepPlan plan_step(const trm_ctx* c, int prog, bool not_last, bool behind_interior) {
        StepPlan s;
        const bool rich = P::richards(c), in_launch = prog != PROG_MULTI && surface_in_launch(c, prog == PROG_HEUN);
        if (in_launch) s.route = ROUTE_SURFACE_IN_LAUNCH;
        else if (prog == PROG_MULTI && averaging(c) && averages_in_launch(c)) s.route = ROUTE_ACCUM_IN_LAUNCH;
        else if (P::levels_per_lane(c) > 1) s.route = ROUTE_LEVELS;
        else if (prog == PROG_EULER && P::packed_path(c)) s.route = ROUTE_PACKED;
        else if (prog != PROG_MULTI && P::generic_bcs(c)) s.route = ROUTE_GENERIC;
        if (prog == PROG_EULER && (s.route == ROUTE_COLUMN || (in_launch && std::is_same<NF, double>::value))) {      // (the form: k_column / fp64 k_column_land)
            s.derive = rich ? P::template derive_now<true>(c) : P::template derive_now<false>(c);
            s.sig = (c->opt_bc_signature && P::hyd(c) != HYD_GENERIC) ? bc_signature_of(c) : -1;
            if (s.derive == DERIVE_T_LIQ) s.staged = rich ? P::template staged_now<true>(c) : P::template staged_now<false>(c);
            if (s.derive == DERIVE_T_LIQ) s.scalar_in = rich ? P::template scalar_inputs_now<true>(c) : P::template scalar_inputs_now<false>(c);
            const bool has_instance = signature_has_instance(s.sig, rich);
            P::io_paths(!has_instance || s.sig == BCSIG_LAND, s.staged, s.scalar_in);
            s.derives_unread = s.derive == DERIVE_T_LIQ && c->part < 0;
            s.store_closure = defer_closure_now(c, s.derives_unread) ? 0 : 1;
            s.psi_step = !in_launch && rich;
        }
        // behind an interior launch the launch must derive the pressure head; it goes interior itself if it is not the call's last and defers
        s.check_entry = behind_interior ? 1 : 0;
        if (prog == PROG_EULER && (behind_interior || not_last)) {
            const bool capable = !in_launch && interior_capable(c);
            if (capable && not_last && !s.store_closure) s.psi_form = PSI_INTERIOR;
            else if (behind_interior && capable) s.psi_form = PSI_LAST;
            else if (behind_interior) s.refusal = "trm_step: the launch behind an interior launch cannot derive the pressure head";
        }
        return s;
    }
};

}  // namespace trmh
