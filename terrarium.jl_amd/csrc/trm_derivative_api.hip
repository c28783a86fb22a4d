// trm_derivative_api.hip -- the derivative entry points of the C ABI (include/terrarium_hip.h): forward-mode tangents (trm_tangent_*,
// trm_step_tangent; trm_column_tangent.hpp) and reverse-mode gradients (trm_adjoint_*, trm_step_record, trm_adjoint_backward;
// trm_column_adjoint.hpp) of the heat-only fp64 run, what they refuse, and the derivative buffers of the context.  Host code alone: the
// kernels are launched by the instantiations of trm_launch_derivative.inl, the transpositions by upload_3d / download_3d (trm_field_io_api.hip).
#include "trm_host.hpp"

using namespace trm;
using namespace trmh;

namespace trmh {
// The derivative launchers: each ride's instantiation lives in a translation unit of its own, the record twin's in another (trm_host.hpp,
// trm_launch_derivative.inl).  One selector: launch(ride constant, record constant) is the launcher's call; `refusal`: no instance
template <class F> static int ride_launch(trm_ctx* c, Ride ride, bool record, const char* refusal, F&& launch) {
    int rc = NO_INSTANCE;
    by_ride(ride, [&](auto r) { rc = record ? launch(r, std::true_type{}) : launch(r, std::false_type{}); });
    return launched(c, rc, refusal);
}
int TangentLaunch::step(trm_ctx* c, double dt, int nsteps, Ride ride, bool record) {
    return ride_launch(c, ride, record, record ? "k_column_tangent_record: a ride without an instance" : "k_column_tangent: a ride without an instance",
                       [&](auto r, auto rec) { return tangent_step<decltype(r)::value, decltype(rec)::value>(c, dt, nsteps); });
}
// k_closure_tangent reads no boundary value: it has the instances RIDE_NONE and RIDE_PARAM (trm_launch_column_tangent{,_param}.hip), and
// every other ride takes RIDE_NONE's
constexpr Ride closure_ride(Ride r) { return r == RIDE_PARAM ? RIDE_PARAM : RIDE_NONE; }
int TangentLaunch::closure(trm_ctx* c, Ride ride) {
    return ride_launch(c, ride, false, "k_closure_tangent: a ride without an instance", [&](auto r, auto) { return tangent_closure<closure_ride(decltype(r)::value)>(c); });
}
template <bool CKPT> static int backward_launch(trm_ctx* c, double dt, int nsteps, int slot, int fold, Ride ride, bool record, int first) {
    return ride_launch(c, ride, record, record ? "k_column_adjoint_record: a ride without an instance" : "k_column_adjoint: a ride without an instance", [&](auto r, auto rec) {
        return adjoint_backward<CKPT, decltype(r)::value, decltype(rec)::value>(c, dt, nsteps, slot, fold, first);
    });
}
int AdjointLaunch::record(trm_ctx* c, double dt, int nsteps, int slot, bool series) {
    return series ? adjoint_record<false, true>(c, dt, nsteps, slot, 0, 1) : adjoint_record<false, false>(c, dt, nsteps, slot, 0, 1);
}
int AdjointLaunch::backward(trm_ctx* c, double dt, int nsteps, int slot, int fold, Ride ride, bool record, int first) {
    return backward_launch<false>(c, dt, nsteps, slot, fold, ride, record, first);
}
int CheckpointLaunch::record(trm_ctx* c, double dt, int nsteps, int slot, int first, int every, bool series) {
    return series ? adjoint_record<true, true>(c, dt, nsteps, slot, first, every) : adjoint_record<true, false>(c, dt, nsteps, slot, first, every);
}
int CheckpointLaunch::backward(trm_ctx* c, double dt, int nsteps, int slot, int fold, Ride ride, bool record, int first) {
    return backward_launch<true>(c, dt, nsteps, slot, fold, ride, record, first);
}
// the heat + Richards sweep: every (params, record) has an instance
int AdjointRichLaunch::backward(trm_ctx* c, double dt, int nsteps, int slot, int fold, bool params, bool record) {
    auto launch = [&](auto par, auto rec) { return adjoint_backward_rich<decltype(par)::value, decltype(rec)::value>(c, dt, nsteps, slot, fold); };
    if (params) return record ? launch(std::true_type{}, std::true_type{}) : launch(std::true_type{}, std::false_type{});
    return record ? launch(std::false_type{}, std::true_type{}) : launch(std::false_type{}, std::false_type{});
}
}  // namespace trmh

namespace {
// ---- the derivative buffers of the context: plain pointers, null while closed.  Allocated and zeroed through the helpers below, freed by
// release() alone -- whole features by release_tangent / release_adjoint (trm_host.hpp: the close calls, failed opens, trm_destroy) ----
// `bytes` of device memory at q if it is null.  A failure leaves q null and no sticky HIP error; the caller reports it.
hipError_t alloc_if_null(double*& q, size_t bytes) {
    if (q) return hipSuccess;
    const hipError_t e = hipMalloc((void**)&q, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        q = nullptr;
    }
    return e;
}
// zeros on the context stream (a closed buffer: nothing)
int zero(trm_ctx* c, double* q, size_t bytes) {
    if (q) TRM_HIP(c, hipMemsetAsync(q, 0, bytes, c->stream));
    return TRM_OK;
}
// q allocated if null, and zeroed where this call allocates it or `rezero`; TRM_ENOMEM "<who>: <misfit>" if it does not fit
int ensure(trm_ctx* c, double*& q, size_t bytes, bool rezero, const std::string& who, const char* misfit) {
    const bool fresh = !q;
    if (alloc_if_null(q, bytes) != hipSuccess) return fail(c, TRM_ENOMEM, who + ": " + misfit);
    return fresh || rezero ? zero(c, q, bytes) : TRM_OK;
}
void release(double*& q) {
    if (q) (void)hipFree(q);
    q = nullptr;
}
template <size_t N> void release(double* (&a)[N]) {
    for (double*& q : a) release(q);
}
// every observation of the tape (trm_adjoint_observe*): a fresh tape has none
void drop_observations(trm_ctx* c) {
    for (auto& o : c->observations) release(o.d_data);
    c->observations.clear();
    c->tape_seg_closed = false;
}
// a record's position table, the device copy with it
void drop_table(RecordTable& t) {
    release(t.d_tables);
    record_table_drop(t);
}
// the attached record (trm_adjoint_observe_record*): its tables, outputs and copies; the caller's device arrays are the caller's
void drop_record(trm_ctx* c) {
    release(c->d_rec_owned);
    release(c->d_rec_out);
    drop_table(c->rec);
    c->d_rec_observed = c->d_rec_weight = nullptr;
    c->rec_swept = false;
}
// the tangent record (trm_tangent_record_attach): its samples and tables
void drop_tangent_record(trm_ctx* c) {
    release(c->d_trec);
    drop_table(c->trec);
    c->trec_position = 0;
}
void release_tape(trm_ctx* c) {
    drop_observations(c);
    drop_record(c);
    release(c->d_tape);
    c->tape_cap = 0;
    c->ckpt_interval = 0;
    c->tape_dt.clear();
    c->tape_segs.clear();
    c->tape_rows.clear();
    c->adj_stale = false;
}
size_t field_bytes(const trm_ctx* c) { return (size_t)c->Nh * (size_t)c->Nzp * sizeof(double); }      // a 3-D field, [Nh][Nzp]
size_t rows_bytes(const trm_ctx* c, long rows = 1) { return (size_t)rows * (size_t)c->Nh * sizeof(double); }   // [rows][Nh]
}  // namespace

namespace trmh {
void release_tangent(trm_ctx* c) {
    release(c->d_tan);
    release(c->d_tan_bc);
    release(c->d_tan_bcs);
    drop_tangent_record(c);
    std::fill(std::begin(c->tan_bcs_nt), std::end(c->tan_bcs_nt), 0L);
    c->tan_bc_seeded = false;
    std::fill(std::begin(c->tan_param), std::end(c->tan_param), 0.0);
    c->tan_param_seeded = false;
    c->tan_stale = false;
}
void release_adjoint(trm_ctx* c) {
    release(c->d_adj);
    release(c->d_adj_bc);
    release(c->d_adj_bcs);
    std::fill(std::begin(c->adj_bcs_nt), std::end(c->adj_bcs_nt), 0L);
    release(c->d_adj_param);
    release(c->d_adj_param_out);
    release(c->d_adj_hyd);
    release(c->d_adj_hyd_out);
    release(c->d_misfit);
    release_tape(c);
}
}  // namespace trmh

namespace {
// ---- what the derivatives cover, and what rides along ------------------------------------------------------------------------------
// what the tangent and adjoint programs cover: the heat-only fp64 SoilModel in columns of one level per lane
// `state_seeds`: the caller is one of the six calls that TRM_OPT_DERIVATIVE_RICHARDS opens to a heat + Richards context
bool richards(const trm_ctx* c) { return c->params.flow == TRM_FLOW_RICHARDS; }
const char* kRichardsStateSeedsOnly = "on a Richards context: state seeds only";
// `tape`: the caller is one of the per-step tape's calls that TRM_OPT_DERIVATIVE_RICHARDS_ADJOINT opens to such a context; with that
// option at 0 they answer as every other call does (the refusal of the others: richards_tape_only, trm_host.hpp)
const char* derivative_unsupported(const trm_ctx* c, bool state_seeds = false, bool tape = false) {
    if (c->precision != TRM_F64) return "fp64 contexts only";
    const bool taped = tape && c->opt_derivative_richards_adjoint;      // (independent of TRM_OPT_DERIVATIVE_RICHARDS)
    if (richards(c) && !taped && !c->opt_derivative_richards) return "the heat-only SoilModel (NoFlow) only";
    if (richards(c) && !taped && !state_seeds) return kRichardsStateSeedsOnly;
    if (c->params.seb || c->veg_mode != TRM_VEGETATION_OFF) return "not the LandModel or vegetation";
    if (c->Nz > 64) return "columns of at most 64 levels";
    return nullptr;
}
// TRM_OPT_DERIVATIVE_SERIES: the series the derivative kernels evaluate themselves -- boundary series of kind Value on temperature or
// Flux on internal energy, whole records, on the branch-free boundary kinds
const char* derivative_series_unsupported(const trm_ctx* c) {
    if (Policy<double>::generic_bcs(c))
        return "no time series with the generic boundary kinds (a Gradient condition on temperature off the branch-free kinds: that step reads its boundary values from memory)";
    for (const auto& sr : c->series) {
        if (!sr.is_bc) return "no input (forcing) time series: boundary series only";
        const int slot = Policy<double>::series_slot(c, sr);
        if (slot < SLOT_T_BOT || slot > SLOT_FU_TOP)
            return "a boundary series of kind Value on temperature or Flux on internal energy only (not of kind Gradient, not on another variable)";
        if (sr.windowed || sr.trimmed || sr.head != 0 || (long)sr.times.size() != sr.cap)
            return "no windowed or trimmed time series: the sweep needs every level the tape spans";
    }
    return nullptr;
}
// the series of a (boundary variable, side) pair, or null
const trm_ctx::Series* bc_series_of(const trm_ctx* c, int bc_var, int side) {
    for (const auto& sr : c->series)
        if (sr.is_bc && sr.var == bc_var && sr.side == side) return &sr;
    return nullptr;
}
// series the derivative launches of this context evaluate in-kernel (0: none attached)
int derivative_series_count(const trm_ctx* c) { return (int)c->series.size(); }
// Thermal parameters ride with a series only under TRM_OPT_DERIVATIVE_SERIES_PARAMS.  `params`: the caller has parameters in play.  The two
// setters (trm_tangent_param_set, trm_adjoint_param_open) pass TRM_OPT_DERIVATIVE_SERIES: without it the steps refuse the series itself, in
// their own words, and the setters say nothing.  The three step functions pass "seeds are set" / "gradients are open"; they have refused a
// series without TRM_OPT_DERIVATIVE_SERIES before they ask, and their series count is the context's.
int params_with_series_ok(trm_ctx* c, bool params, const char* who) {
    if (!params || c->series.empty() || c->opt_derivative_series_params) return TRM_OK;
    return fail(c, TRM_EUNSUPPORTED, std::string(who) + ": no thermal-parameter seeds or gradients together with a time series unless TRM_OPT_DERIVATIVE_SERIES_PARAMS is set");
}
// ... and what a step needs besides: constant inputs, no accumulation, the temperature halos of the heat-only programs
const char* derivative_step_unsupported(const trm_ctx* c, bool state_seeds = false, bool tape = false) {
    if (const char* why = derivative_unsupported(c, state_seeds, tape)) return why;
    if (richards(c)) {      // (k_column_tangent_rich: constant boundary values, the branch-free kinds)
        if (!c->series.empty()) return "no time series may be attached";
        if (c->opt_vwc_field) return "no per-cell vwc_forcing field";
        if (Policy<double>::generic_bcs(c)) return "on a Richards context: the branch-free boundary kinds only (no Value or Gradient condition on saturation, liquid fraction or pressure head, no Gradient on temperature)";
    }
    if (!c->series.empty()) {
        if (!c->opt_derivative_series) return "no time series may be attached";
        if (const char* why = derivative_series_unsupported(c)) return why;
    }
    for (const auto& a : c->averages)
        if (a.field >= 0) return "no time average may be open";
    if (c->opt_vwc_field) return "no per-cell vwc_forcing field";
    for (int side = 0; side < 2; ++side)
        if (c->bc_kind[TRM_BCV_LIQUID_WATER_FRACTION][side] == TRM_BC_VALUE || c->bc_kind[TRM_BCV_LIQUID_WATER_FRACTION][side] == TRM_BC_GRADIENT)
            return "no Value or Gradient condition on the liquid water fraction";
    return nullptr;
}
int refuse(trm_ctx* c, const char* who, const char* why, int code = TRM_EUNSUPPORTED) { return fail(c, code, std::string(who) + ": " + why); }
// what rides along with a tangent step / a backward sweep: series first (with the thermal parameters where they are seeded / open:
// TRM_OPT_DERIVATIVE_SERIES_PARAMS, the steps have refused them otherwise), then the thermal parameters, then the boundary values
Ride tangent_ride(const trm_ctx* c, int nser) {
    if (nser) return c->tan_param_seeded ? RIDE_PARAM_SERIES : RIDE_SERIES;
    return c->tan_param_seeded ? RIDE_PARAM : c->tan_bc_seeded ? RIDE_BC : RIDE_NONE;
}
Ride backward_ride(const trm_ctx* c, int nser) {
    if (nser) return c->d_adj_param_out ? RIDE_PARAM_SERIES : RIDE_SERIES;
    return c->d_adj_param_out ? RIDE_PARAM : c->d_adj_bc[0] ? RIDE_BC : RIDE_NONE;
}
// trm_step_tangent and trm_step_record issue the launches of trm_step(ctx, dt, nsteps, 1) on the multi-step program: up to
// TRM_OPT_STEPS_PER_LAUNCH steps each ...
int derivative_steps_per_launch(const trm_ctx* c) { return c->opt_steps_per_launch > 0 ? c->opt_steps_per_launch : StepPolicy<double>::auto_steps_per_launch(c); }
// ... and leave what a finalizing step leaves
int derivative_steps_done(trm_ctx* c) {
    c->closure_consistent = true;
    c->psi_consistent = false;
    c->tend_valid = true;      // (every launch stores the tendency of its last step, as a finalizing launch)
    c->top_valid = false;
    return finish(c, TRM_OK);
}
// ---- argument checks ---------------------------------------------------------------------------------------------------------------
// `open`: the pointer that is non-null while the feature is open; `feature`: subject and verb of the refusal; `opener`: the call that opens it
int require_open(trm_ctx* c, const void* open, const char* who, const char* feature, const char* opener) {
    return open ? TRM_OK : fail(c, TRM_EINVAL, std::string(who) + ": no " + feature + " open (" + opener + ")");
}
int tangent_open(trm_ctx* c, const char* who) { return require_open(c, c->d_tan[0], who, "tangent is", "trm_tangent_open"); }
// the tangent fields of the context: dU, dT, dliq, and on a Richards context dsat and dpsi
int tangent_fields(const trm_ctx* c) { return richards(c) ? TRM_TANGENT_PRESSURE_HEAD + 1 : TRM_TANGENT_LIQUID_WATER_FRACTION + 1; }
// a call the Richards tangent does not cover, on a context with one open
int richards_state_seeds_only(trm_ctx* c, const char* who) { return richards(c) ? fail(c, TRM_EUNSUPPORTED, std::string(who) + ": " + kRichardsStateSeedsOnly) : TRM_OK; }
int adjoint_open(trm_ctx* c, const char* who) { return require_open(c, c->d_adj[0], who, "adjoint is", "trm_adjoint_open"); }
// the cotangent fields of the context: wU, wT, wliq, and on a Richards context wsat and wpsi
int adjoint_fields(const trm_ctx* c) { return richards(c) ? TRM_ADJOINT_PRESSURE_HEAD + 1 : TRM_ADJOINT_LIQUID_WATER_FRACTION + 1; }
// the fields of a tape slot: U_k, and on a Richards context sat_k behind it
size_t tape_slot_fields(const trm_ctx* c) { return richards(c) ? 2 : 1; }
// ... and an index in [0, bound) with a non-null pointer (`hint`: what the index counts, appended to the refusal)
int which_ok(trm_ctx* c, int which, int bound, const void* ptr, const char* who, const char* hint = "") {
    return which >= 0 && which < bound && ptr ? TRM_OK : fail(c, TRM_EINVAL, std::string(who) + ": bad argument" + hint);
}
const char* kPairHint = " (internal energy or temperature, bottom or top)";
// the slot of a (boundary variable, side) pair in d_tan_bc / d_adj_bc, -1 for a pair the heat-only step reads no value of
int bc_pair_index(int bc_var, int side) {
    if (side != TRM_BOTTOM && side != TRM_TOP) return -1;
    if (bc_var == TRM_BCV_TEMPERATURE) return side == TRM_TOP ? 1 : 0;
    if (bc_var == TRM_BCV_INTERNAL_ENERGY) return side == TRM_TOP ? 3 : 2;
    return -1;
}
// the per-column calls of a pair: its slot; refused where a series drives the pair (`instead`: its seeds / gradient and the call that takes them)
int bc_pair_args(trm_ctx* c, int bc_var, int side, const void* ptr, const char* who, const char* instead, int& slot) {
    slot = bc_pair_index(bc_var, side);
    if (int rc = which_ok(c, slot, 4, ptr, who, kPairHint)) return rc;
    if (c->opt_derivative_series && bc_series_of(c, bc_var, side)) return refuse(c, who, (std::string("the pair is driven by a time series: ") + instead).c_str(), TRM_EINVAL);
    return TRM_OK;
}
// the per-node calls of a pair: its slot and its series
int bc_series_args(trm_ctx* c, int bc_var, int side, const char* who, int& slot, const trm_ctx::Series*& sr) {
    slot = bc_pair_index(bc_var, side);
    if (int rc = which_ok(c, slot, 4, c, who, kPairHint)) return rc;
    sr = bc_series_of(c, bc_var, side);
    if (!sr) return refuse(c, who, "the pair has no time series (trm_set_bc_series)", TRM_EINVAL);
    return TRM_OK;
}
// the square roots of the five conductivities have no derivative at 0
const char* thermal_params_not_differentiable(const trm_ctx* c) {
    const trm_params& q = c->params;
    if (!(q.k_water > 0.0 && q.k_ice > 0.0 && q.k_air > 0.0 && q.k_mineral > 0.0 && q.k_organic > 0.0))
        return "every thermal conductivity must be > 0 (sqrt has no derivative at 0)";
    return nullptr;
}
const char* kStaleTangent = ": the state has changed since the tangent was seeded: trm_tangent_upload a new dU first";
const char* kStaleTape = ": the state or a boundary condition has changed since the first taped step: trm_adjoint_open starts a new tape";

// ---- allocation of the optional buffers ------------------------------------------------------------------------------------------------
// the four boundary seed arrays, zeroed where this call allocates them
int alloc_tangent_bc_seeds(trm_ctx* c, const char* who) {
    for (double*& q : c->d_tan_bc)
        if (int rc = ensure(c, q, rows_bytes(c), false, who, "the seed arrays do not fit")) return rc;
    return TRM_OK;
}
// a [nt][Nh] array shaped like the series of a pair, zeroed where this call allocates it (a series of another length replaces it)
int alloc_series_shaped(trm_ctx* c, double*& q, long& have_nt, long nt, const char* who) {
    if (q && have_nt == nt) return TRM_OK;
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    release(q);
    have_nt = 0;
    if (int rc = ensure(c, q, rows_bytes(c, nt), false, who, "an array of the series' shape does not fit")) return rc;
    have_nt = nt;
    return TRM_OK;
}
// the four per-column accumulators, zeroed: all of them (trm_adjoint_bc_open) or the ones this call allocates (`only_new`: a sweep with
// series, which rides with the accumulating instances, opens them if nobody has)
int open_adjoint_bc(trm_ctx* c, bool only_new, const char* who) {
    for (double*& q : c->d_adj_bc)
        if (int rc = ensure(c, q, rows_bytes(c), !only_new, who, "the accumulators do not fit")) {
            release(c->d_adj_bc);
            return rc;
        }
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    return TRM_OK;
}
// trm_adjoint_open (`interval` 0: `capacity` slots, one per step) and trm_adjoint_open_checkpointed (`capacity` checkpoint slots)
int open_adjoint(trm_ctx* c, int capacity, int interval, const std::string& who) {
    if (interval)
        if (int rc = richards_tape_only(c, who.c_str())) return rc;
    if (const char* why = derivative_unsupported(c, false, interval == 0)) return refuse(c, who.c_str(), why);
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    const size_t bytes = field_bytes(c), slot_bytes = bytes * tape_slot_fields(c);
    if (capacity != c->tape_cap || interval != c->ckpt_interval) {
        release_tape(c);
        if (alloc_if_null(c->d_tape, (size_t)capacity * slot_bytes) != hipSuccess) {
            const bool was_open = c->d_adj[0] != nullptr;
            release_adjoint(c);
            return fail(c, TRM_ENOMEM, who + ": a tape of " + std::to_string(capacity) + (interval ? " checkpoints x " : " steps x ") + std::to_string(slot_bytes) +
                                           " bytes does not fit" + (was_open ? " (the adjoint that was open is closed)" : ""));
        }
        c->tape_cap = capacity;
        c->ckpt_interval = interval;
    }
    for (int f = 0; f < adjoint_fields(c); ++f)
        if (int rc = ensure(c, c->d_adj[f], bytes, true, who, "the cotangent fields do not fit")) {
            release_adjoint(c);
            return rc;
        }
    // (opening again keeps open boundary gradients, node gradients and parameter gradients, zero)
    int rc = TRM_OK;
    for (double* q : c->d_adj_bc) if (!rc) rc = zero(c, q, rows_bytes(c));
    for (int s = 0; s < 4; ++s) if (!rc) rc = zero(c, c->d_adj_bcs[s], rows_bytes(c, c->adj_bcs_nt[s]));
    for (double* q : c->d_adj_param) if (!rc) rc = zero(c, q, bytes);
    if (!rc) rc = zero(c, c->d_adj_param_out, rows_bytes(c, TRM_THERMAL_PARAM_COUNT));
    for (double* q : c->d_adj_hyd) if (!rc) rc = zero(c, q, bytes);
    if (!rc) rc = zero(c, c->d_adj_hyd_out, rows_bytes(c, TRM_HYDRAULIC_PARAM_COUNT));
    if (!rc) rc = zero(c, c->d_misfit, rows_bytes(c));
    if (rc) return rc;
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    drop_observations(c);
    drop_record(c);
    c->tape_dt.clear();        // (a fresh tape)
    c->tape_segs.clear();
    c->tape_rows.clear();
    c->adj_stale = false;
    return TRM_OK;
}
// ---- the arguments of the gradient getters --------------------------------------------------------------------------------------------
// the per-column gradient of a pair
int adjoint_bc_args(trm_ctx* c, int bc_var, int side, const void* ptr, const char* who, int& slot) {
    if (int rc = adjoint_open(c, who)) return rc;
    if (int rc = require_open(c, c->d_adj_bc[0], who, "boundary gradients are", "trm_adjoint_bc_open")) return rc;
    return bc_pair_args(c, bc_var, side, ptr, who, "its gradient has the series' shape (trm_adjoint_bc_series_download)", slot);
}
// the node accumulator of a seriesed pair (zeros until a sweep has run)
int adjoint_bc_series_args(trm_ctx* c, int bc_var, int side, const void* ptr, const char* who, int& slot, long& nt) {
    if (int rc = adjoint_open(c, who)) return rc;
    const trm_ctx::Series* sr = nullptr;
    if (int rc = bc_series_args(c, bc_var, side, who, slot, sr)) return rc;
    if (int rc = which_ok(c, 0, 1, ptr, who)) return rc;
    nt = sr->cap;
    return alloc_series_shaped(c, c->d_adj_bcs[slot], c->adj_bcs_nt[slot], nt, who);
}
// a parameter gradient: `row` its num_columns doubles -- a thermal parameter's, or on a Richards context with the hydraulic-parameter
// gradients open (TRM_OPT_DERIVATIVE_RICHARDS_PARAMS) one of the seven TRM_HYDRAULIC_PARAM_* ids', which count on from the thermal ones
int adjoint_param_args(trm_ctx* c, int which, const void* ptr, const char* who, double*& row) {
    if (int rc = adjoint_open(c, who)) return rc;
    if (richards(c) && c->d_adj_hyd_out) {
        const int at = hyd_param_row(which);
        if (int rc = which_ok(c, at, TRM_HYDRAULIC_PARAM_COUNT, ptr, who, " (TRM_HYDRAULIC_PARAM_*)")) return rc;
        row = c->d_adj_hyd_out + (size_t)at * (size_t)c->Nh;
        return TRM_OK;
    }
    if (int rc = require_open(c, c->d_adj_param_out, who, "parameter gradients are", "trm_adjoint_param_open")) return rc;
    if (int rc = which_ok(c, which, TRM_THERMAL_PARAM_COUNT, ptr, who, " (TRM_THERMAL_PARAM_*)")) return rc;
    row = c->d_adj_param_out + (size_t)which * (size_t)c->Nh;
    return TRM_OK;
}
// TRM_OPT_DERIVATIVE_RICHARDS_PARAMS takes effect together with TRM_OPT_DERIVATIVE_RICHARDS_ADJOINT alone, on a Richards context
bool hydraulic_params_enabled(const trm_ctx* c) { return richards(c) && c->opt_derivative_richards_adjoint && c->opt_derivative_richards_params; }
// trm_adjoint_param_open there: the seven per-cell accumulators and the per-column results, zero; no boundary accumulators
int open_hydraulic_params(trm_ctx* c, const char* who) {
    if (const char* why = derivative_unsupported(c, false, true)) return refuse(c, who, why);
    if (int rc = adjoint_open(c, who)) return rc;
    if (c->ckpt_interval != 0) return refuse(c, who, kRichardsTapeOnly);
    int rc = TRM_OK;
    for (double*& q : c->d_adj_hyd)
        if (!rc) rc = ensure(c, q, field_bytes(c), true, who, "the accumulators do not fit");
    if (!rc) rc = ensure(c, c->d_adj_hyd_out, rows_bytes(c, TRM_HYDRAULIC_PARAM_COUNT), true, who, "the accumulators do not fit");
    if (rc) {
        release(c->d_adj_hyd);
        release(c->d_adj_hyd_out);
        return rc;
    }
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    return TRM_OK;
}
// ---- adjoint observations ------------------------------------------------------------------------------------------------------------
// the level list of an observation: rows of the host layout, strictly increasing
int observed_levels_ok(trm_ctx* c, int nlevels, const int32_t* levels, const char* who) {
    if (nlevels < 1 || !levels) return fail(c, TRM_EINVAL, std::string(who) + ": bad argument (nlevels >= 1 levels)");
    for (int j = 0; j < nlevels; ++j)
        if (levels[j] < 0 || levels[j] >= c->Nz || (j > 0 && levels[j] <= levels[j - 1]))
            return fail(c, TRM_EINVAL, std::string(who) + ": the levels are rows 0 ... " + std::to_string(c->Nz - 1) + " of the host layout, strictly increasing");
    return TRM_OK;
}
// An observation of the state the context holds now joins the tape at position taped_steps: its arrays ([nlevels][Nh] doubles each; a
// null one is left out) and the level list go to the device in one allocation.  Checkpointed: it closes the open segment.
int register_observation(trm_ctx* c, int kind, int nlevels, const int32_t* levels, const void* first, const void* second, const char* who) {
    trm_ctx::Observation o{taped_steps(c), kind, nlevels, second ? 2 : 1, nullptr};
    const size_t array_bytes = rows_bytes(c, nlevels);
    if (alloc_if_null(o.d_data, (size_t)o.bytes(c->Nh)) != hipSuccess) return fail(c, TRM_ENOMEM, std::string(who) + ": the observation does not fit");
    const void* src[2] = {first, second};
    hipError_t e = hipSuccess;
    for (int a = 0; a < o.arrays && e == hipSuccess; ++a)
        e = hipMemcpyAsync(o.d_data + (size_t)a * (size_t)nlevels * (size_t)c->Nh, src[a], array_bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync((void*)o.levels(c->Nh), levels, (size_t)nlevels * sizeof(int32_t), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        release(o.d_data);
        return fail(c, TRM_EHIP, std::string(who) + ": " + hipGetErrorString(e));
    }
    c->observations.push_back(o);
    if (c->ckpt_interval && !c->tape_segs.empty()) c->tape_seg_closed = true;
    return TRM_OK;
}
// what both registrations check first
int observe_args(trm_ctx* c, int nlevels, const int32_t* levels, const void* host, const char* who) {
    if (int rc = richards_tape_only(c, who)) return rc;
    if (int rc = adjoint_open(c, who)) return rc;
    if (int rc = record_excludes_observations(c, who)) return rc;
    if (int rc = observed_levels_ok(c, nlevels, levels, who)) return rc;
    if (int rc = which_ok(c, 0, 1, host, who)) return rc;
    if (c->adj_stale) return fail(c, TRM_ESTALE, std::string(who) + kStaleTape);
    return TRM_OK;
}
bool observed(const trm_ctx* c, int position) {
    for (const auto& o : c->observations)
        if (o.position == position) return true;
    return false;
}
// trm_adjoint_backward walks the per-step tape in blocks of up to `spl` taped steps that share one dt, newest block first: the first step
// of the block that ends below `end`.  A block also ends at an observed position: its cotangent enters lam between two launches (a
// Richards context has none: observe_args)
int tape_block_begin(const trm_ctx* c, int end, int spl) {
    int begin = end;
    while (begin > 0 && end - begin < spl && c->tape_dt[(size_t)begin - 1] == c->tape_dt[(size_t)end - 1] && !(begin < end && observed(c, begin))) --begin;
    return begin;
}
// The observations of taped position p, in registration order (trm_adjoint_backward: in front of the launch whose newest step is p - 1,
// behind the last launch for p = 0).  U_p: tape slot p, the checkpoint of the segment that starts at p, the context's U for p = n.
int inject_observations(trm_ctx* c, int p, bool lam, bool params) {
    if (c->observations.empty()) return TRM_OK;
    const double* U_p = nullptr;
    if (p != taped_steps(c)) {
        const size_t slot_elems = (size_t)c->Nh * (size_t)c->Nzp;
        if (!c->ckpt_interval) U_p = c->d_tape + (size_t)p * slot_elems;
        for (const auto& seg : c->tape_segs)
            if (seg.first == p) U_p = c->d_tape + (size_t)seg.slot * slot_elems;
        if (!U_p && observed(c, p)) return fail(c, TRM_EINVAL, "trm_adjoint_backward: an observed position is no checkpoint");
    }
    for (const auto& o : c->observations)
        if (o.position == p)
            if (int rc = ObserveLaunch::inject(c, o, U_p, lam, params)) return rc;
    return TRM_OK;
}
// ---- attached records ------------------------------------------------------------------------------------------------------------------
// The record joins the open adjoint: the level table, the residuals and the misfit are the library's; `observed` / `weight` are host arrays
// the library copies once (`device` false) or device arrays it keeps by pointer
int attach_record(trm_ctx* c, int npos, const int32_t* positions, int nlevels, const int32_t* levels, const void* observed, const void* weight, bool device, const char* who) {
    if (int rc = richards_tape_only(c, who, true)) return rc;
    if (int rc = record_attach_ok(c, npos, positions, nlevels, levels, observed, device ? nullptr : (const double*)weight, who)) return rc;
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    const size_t cells = (size_t)npos * (size_t)nlevels * (size_t)c->Nh, cell_bytes = cells * sizeof(double);
    const std::string w(who);
    int rc = ensure(c, c->d_rec_out, cell_bytes + rows_bytes(c), true, w, "the residuals do not fit");
    if (!rc && !device) rc = ensure(c, c->d_rec_owned, cell_bytes * (weight ? 2 : 1), false, w, "the record does not fit");
    if (!rc) {
        hipError_t e = hipSuccess;
        if (!device) {
            e = hipMemcpyAsync(c->d_rec_owned, observed, cell_bytes, hipMemcpyHostToDevice, c->stream);
            if (e == hipSuccess && weight) e = hipMemcpyAsync(c->d_rec_owned + cells, weight, cell_bytes, hipMemcpyHostToDevice, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        }
        if (e != hipSuccess) rc = fail(c, TRM_EHIP, w + ": " + hipGetErrorString(e));
    }
    if (rc) {
        drop_record(c);
        return rc;
    }
    c->d_rec_observed = device ? (const double*)observed : c->d_rec_owned;
    c->d_rec_weight = !weight ? nullptr : device ? (const double*)weight : c->d_rec_owned + cells;
    record_table_attach(c->rec, npos, positions, nlevels, levels);     // (the tables go up with the first sweep: they depend on the steps the tape holds then)
    c->rec_swept = false;
    return TRM_OK;
}
// The staged tables of a record (record_table_build) to the device, on the context's stream.  The caller waits for the stream before the
// staging copy changes again
int upload_table(trm_ctx* c, RecordTable& t, const std::string& who) {
    const size_t bytes = t.host.size() * sizeof(int32_t);
    if (alloc_if_null(t.d_tables, (bytes + 7) / 8 * 8) != hipSuccess) return fail(c, TRM_ENOMEM, who + ": the record's tables do not fit");
    const hipError_t e = hipMemcpyAsync(t.d_tables, t.host.data(), bytes, hipMemcpyHostToDevice, c->stream);
    return e == hipSuccess ? TRM_OK : fail(c, TRM_EHIP, who + ": " + hipGetErrorString(e));
}
// row_of_level and row_of_position of a tape of n steps, in front of a sweep's first launch; a sweep over the count of the sweep before
// finds them in place
int record_tables(trm_ctx* c, int n, const char* who) {
    if (c->rec.entries == n + 1 && c->rec.d_tables) return TRM_OK;
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    release(c->rec.d_tables);
    record_table_build(c->rec, c->Nz, n);
    const int rc = upload_table(c, c->rec, who);
    if (rc) c->rec.entries = 0;
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    return rc;
}
}  // namespace

extern "C" {

// ---- forward-mode tangents of the heat-only step (trm_column_tangent.hpp) ---------------------------------------------------
int trm_tangent_open(trm_ctx* c) {
    TRM_ENTER_HEUN(c);
    if (const char* why = derivative_unsupported(c, true)) return refuse(c, "trm_tangent_open", why);
    const size_t bytes = field_bytes(c);
    int rc = TRM_OK;
    for (int f = 0; f < tangent_fields(c); ++f) {
        double*& q = c->d_tan[f];
        if (const hipError_t e = alloc_if_null(q, bytes)) {
            release_tangent(c);
            return fail(c, TRM_EHIP, std::string("hipMalloc((void**)&q, bytes): ") + hipGetErrorString(e));
        }
        if (!rc) rc = zero(c, q, bytes);
    }
    for (double* q : c->d_tan_bc) if (!rc) rc = zero(c, q, rows_bytes(c));
    for (int s = 0; s < 4; ++s) if (!rc) rc = zero(c, c->d_tan_bcs[s], rows_bytes(c, c->tan_bcs_nt[s]));
    if (rc) return rc;
    c->tan_bc_seeded = false;
    std::fill(std::begin(c->tan_param), std::end(c->tan_param), 0.0);
    c->tan_param_seeded = false;
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    drop_tangent_record(c);    // (a new tangent has no record)
    c->tan_stale = false;      // (a zero seed: zero tangents)
    return TRM_OK;
}
int trm_tangent_close(trm_ctx* c) {
    TRM_ENTER_HEUN(c);
    if (!c->d_tan[0]) return fail(c, TRM_EINVAL, "trm_tangent_close: no tangent is open");
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    release_tangent(c);
    return TRM_OK;
}
int trm_tangent_bc_series_upload(trm_ctx* c, int bc_var, int side, int nt, const void* host) {
    TRM_ENTER_HEUN(c);
    const char* who = "trm_tangent_bc_series_upload";
    if (int rc = tangent_open(c, who)) return rc;
    if (int rc = richards_state_seeds_only(c, who)) return rc;
    int slot = -1;
    const trm_ctx::Series* sr = nullptr;
    if (int rc = bc_series_args(c, bc_var, side, who, slot, sr)) return rc;
    if (int rc = which_ok(c, 0, 1, host, who)) return rc;
    if ((long)nt != sr->cap || (long)sr->times.size() != sr->cap)
        return fail(c, TRM_EINVAL, "trm_tangent_bc_series_upload: nt must be the levels of the pair's series (" + std::to_string(sr->times.size()) + ")");
    if (int rc = alloc_tangent_bc_seeds(c, who)) return rc;
    if (int rc = alloc_series_shaped(c, c->d_tan_bcs[slot], c->tan_bcs_nt[slot], nt, who)) return rc;
    TRM_HIP(c, hipMemcpyAsync(c->d_tan_bcs[slot], host, rows_bytes(c, nt), hipMemcpyHostToDevice, c->stream));
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    return TRM_OK;             // (seeds are not state: tan_stale stays as it is)
}
int trm_tangent_bc_upload(trm_ctx* c, int bc_var, int side, const void* host) {
    TRM_ENTER_HEUN(c);
    const char* who = "trm_tangent_bc_upload";
    if (int rc = tangent_open(c, who)) return rc;
    if (int rc = richards_state_seeds_only(c, who)) return rc;
    int slot = -1;
    if (int rc = bc_pair_args(c, bc_var, side, host, who, "its seeds have the series' shape (trm_tangent_bc_series_upload)", slot)) return rc;
    if (int rc = alloc_tangent_bc_seeds(c, who)) return rc;
    TRM_HIP(c, hipMemcpyAsync(c->d_tan_bc[slot], host, rows_bytes(c), hipMemcpyHostToDevice, c->stream));
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    c->tan_bc_seeded = true;   // (seeds are not state: tan_stale stays as it is)
    return TRM_OK;
}
int trm_tangent_param_set(trm_ctx* c, const double seed[TRM_THERMAL_PARAM_COUNT]) {
    TRM_ENTER_HEUN(c);
    const char* who = "trm_tangent_param_set";
    // (a context the tangent does not cover has none open: it is told why, not to open one)
    if (const char* why = derivative_unsupported(c)) return refuse(c, who, why);
    if (int rc = tangent_open(c, who)) return rc;
    if (int rc = which_ok(c, 0, 1, seed, who)) return rc;
    if (int rc = params_with_series_ok(c, c->opt_derivative_series != 0, who)) return rc;
    if (const char* why = thermal_params_not_differentiable(c)) return refuse(c, who, why, TRM_EINVAL);
    if (int rc = alloc_tangent_bc_seeds(c, who)) return rc;
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    // the chain rule to the eight numbers the kernels hold (thermal_param_chain): a sum per derived number, in the order of trm_params
    double w[TRM_THERMAL_PARAM_COUNT];
    thermal_param_chain(c->params, launch_args<double>(c).p, w);
    std::fill(std::begin(c->tan_param), std::end(c->tan_param), 0.0);
    for (int q = 0; q < TRM_THERMAL_PARAM_COUNT; ++q) c->tan_param[thermal_param_target(q)] += w[q] * seed[q];
    c->tan_param_seeded = true;   // (seeds are not state: tan_stale stays as it is)
    return TRM_OK;
}
int trm_tangent_upload(trm_ctx* c, int which, const void* host) {
    TRM_ENTER_HEUN(c);
    if (int rc = tangent_open(c, "trm_tangent_upload")) return rc;
    if (int rc = which_ok(c, which, tangent_fields(c), host, "trm_tangent_upload")) return rc;
    // (a Richards context takes its two seeds: dT, dliq and dpsi are the closure's)
    if (richards(c) && which != TRM_TANGENT_INTERNAL_ENERGY && which != TRM_TANGENT_SATURATION) return which_ok(c, -1, 0, host, "trm_tangent_upload");
    if (int rc = upload_3d<double>(c, (const double*)host, c->d_tan[which])) return rc;
    if (which == TRM_TANGENT_INTERNAL_ENERGY) c->tan_stale = false;
    return TRM_OK;
}
int trm_tangent_download(trm_ctx* c, int which, void* host) {
    TRM_ENTER_HEUN(c);
    if (int rc = tangent_open(c, "trm_tangent_download")) return rc;
    if (int rc = which_ok(c, which, tangent_fields(c), host, "trm_tangent_download")) return rc;
    if (which != TRM_TANGENT_INTERNAL_ENERGY && which != TRM_TANGENT_SATURATION && c->tan_stale) return fail(c, TRM_ESTALE, std::string("trm_tangent_download") + kStaleTangent);
    return download_3d<double>(c, c->d_tan[which], (double*)host);
}
int trm_tangent_device_ptr(trm_ctx* c, int which, void** dev, int64_t* pitch_elems) {
    TRM_ENTER_HEUN(c);
    if (int rc = tangent_open(c, "trm_tangent_device_ptr")) return rc;
    if (int rc = which_ok(c, which, tangent_fields(c), dev, "trm_tangent_device_ptr")) return rc;
    if (int rc = which_ok(c, 0, 1, pitch_elems, "trm_tangent_device_ptr")) return rc;
    *dev = c->d_tan[which];
    *pitch_elems = c->Nzp;
    return TRM_OK;
}
int trm_tangent_closure(trm_ctx* c) {
    TRM_ENTER_HEUN(c);
    if (int rc = tangent_open(c, "trm_tangent_closure")) return rc;
    if (const char* why = derivative_unsupported(c, true)) return refuse(c, "trm_tangent_closure", why);
    if (c->tan_stale) return fail(c, TRM_ESTALE, std::string("trm_tangent_closure") + kStaleTangent);
    if (richards(c)) return finish(c, TangentRichLaunch::closure(c));
    return finish(c, TangentLaunch::closure(c, tangent_ride(c, 0)));
}
int trm_step_tangent(trm_ctx* c, double dt, int nsteps) {
    TRM_ENTER(c);
    const char* who = "trm_step_tangent";
    if (int rc = tangent_open(c, who)) return rc;
    if (nsteps < 0) return fail(c, TRM_EINVAL, "trm_step_tangent: nsteps < 0");
    if (const char* why = derivative_step_unsupported(c, true)) return refuse(c, who, why);
    const int nser = derivative_series_count(c);
    if (int rc = params_with_series_ok(c, c->tan_param_seeded, who)) return rc;
    if (c->tan_stale) return fail(c, TRM_ESTALE, std::string(who) + kStaleTangent);
    if (richards(c)) {      // (state seeds alone: no ride, no record, no series -- the launches of trm_step's multi-step program)
        bc_changed(c);
        const int spl = derivative_steps_per_launch(c);
        for (int n = 0, m; n < nsteps; n += m) {
            m = std::min(spl, nsteps - n);
            int rc = Unfused<double>::update_inputs(c, c->state, c->time);
            if (!rc) rc = TangentRichLaunch::step(c, dt, m);
            if (rc) return rc;
            c->derivative_series = 0;
            tick(c, dt, m);
        }
        return derivative_steps_done(c);
    }
    if (nser) {   // series ride with the boundary-seeded instances: the per-column seeds, and zeros for a series nobody has seeded
        if (int rc = alloc_tangent_bc_seeds(c, who)) return rc;
        for (const auto& sr : c->series) {
            const int slot = bc_pair_index(sr.var, sr.side);
            if (int rc = alloc_series_shaped(c, c->d_tan_bcs[slot], c->tan_bcs_nt[slot], sr.cap, who)) return rc;
        }
    }
    bc_changed(c);             // (a state-changing call for an open tape)
    const int spl = derivative_steps_per_launch(c);
    const Ride ride = tangent_ride(c, nser);
    for (int n = 0, m; n < nsteps; n += m) {
        m = std::min(spl, nsteps - n);
        // (a tangent record: the launch ends at its last position at the latest; the steps behind it sample nothing and are the
        // record-free kernel's)
        const int recorded = tangent_record_steps(c, m);
        if (recorded) m = recorded;
        int rc = nser ? Unfused<double>::upload_series_rows(c, dt, m) : Unfused<double>::update_inputs(c, c->state, c->time);
        if (!rc) rc = TangentLaunch::step(c, dt, m, ride, recorded != 0);
        if (rc) return rc;
        c->derivative_series = nser;
        if (c->trec.npos) c->trec_position += m;
        tick(c, dt, m);
    }
    return derivative_steps_done(c);
}

// ---- tangent records: T and dT sampled inside the tangent launches (trm_column_tangent_record.hpp) ----------------------------------
int trm_tangent_record_attach(trm_ctx* c, int npos, const int32_t* positions, int nlevels, const int32_t* levels) {
    TRM_ENTER_HEUN(c);
    const char* who = "trm_tangent_record_attach";
    // (a context the tangent does not cover has none open: it is told why, not to open one)
    if (const char* why = derivative_unsupported(c)) return refuse(c, who, why);
    if (int rc = tangent_record_attach_ok(c, npos, positions, nlevels, levels, who)) return rc;
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    const std::string w(who);
    record_table_attach(c->trec, npos, positions, nlevels, levels);
    record_table_build(c->trec, c->Nz, tangent_record_limit(c->trec.positions));
    const size_t cell_bytes = rows_bytes(c, (long)npos * nlevels);
    int rc = TRM_OK;
    for (double*& q : c->d_trec)
        if (!rc && alloc_if_null(q, cell_bytes) != hipSuccess) rc = fail(c, TRM_ENOMEM, w + ": the samples do not fit");
    if (!rc) rc = upload_table(c, c->trec, w);
    if (!rc) {
        hipError_t e = hipSuccess;
        for (double* q : c->d_trec)
            if (e == hipSuccess) e = hipMemsetAsync(q, 0xFF, cell_bytes, c->stream);    // (every byte set: a NaN)
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) rc = fail(c, TRM_EHIP, w + ": " + hipGetErrorString(e));
    }
    if (rc) {
        drop_tangent_record(c);
        return rc;
    }
    c->trec_position = 0;
    return TRM_OK;
}
int trm_tangent_record_rewind(trm_ctx* c) {
    TRM_ENTER_HEUN(c);
    if (int rc = tangent_record_attached(c, "trm_tangent_record_rewind")) return rc;
    for (double* q : c->d_trec) TRM_HIP(c, hipMemsetAsync(q, 0xFF, rows_bytes(c, (long)c->trec.npos * c->trec.nlevels), c->stream));
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    c->trec_position = 0;
    return TRM_OK;
}
int trm_tangent_record_detach(trm_ctx* c) {
    TRM_ENTER_HEUN(c);
    if (int rc = tangent_record_attached(c, "trm_tangent_record_detach")) return rc;
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    drop_tangent_record(c);
    return TRM_OK;
}
int trm_tangent_record_download(trm_ctx* c, int which, void* host) {
    TRM_ENTER_HEUN(c);
    const char* who = "trm_tangent_record_download";
    if (int rc = tangent_record_attached(c, who)) return rc;
    if (int rc = which_ok(c, which, TRM_TANGENT_RECORD_TANGENT + 1, host, who, " (TRM_TANGENT_RECORD_*)")) return rc;
    TRM_HIP(c, hipMemcpyAsync(host, c->d_trec[which], rows_bytes(c, (long)c->trec.npos * c->trec.nlevels), hipMemcpyDeviceToHost, c->stream));
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    return TRM_OK;
}
int trm_tangent_record_device_ptr(trm_ctx* c, int which, void** dev) {
    TRM_ENTER_HEUN(c);
    const char* who = "trm_tangent_record_device_ptr";
    if (int rc = tangent_record_attached(c, who)) return rc;
    if (int rc = which_ok(c, which, TRM_TANGENT_RECORD_TANGENT + 1, dev, who, " (TRM_TANGENT_RECORD_*)")) return rc;
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    *dev = c->d_trec[which];
    return TRM_OK;
}
int trm_tangent_record_info(const trm_ctx* c, int* npos, int* nlevels, int64_t* position, int64_t* bytes) {
    if (!c) return TRM_EINVAL;
    if (int rc = tangent_open(const_cast<trm_ctx*>(c), "trm_tangent_record_info")) return rc;
    if (npos) *npos = c->trec.npos;
    if (nlevels) *nlevels = c->trec.nlevels;
    if (position) *position = c->trec_position;
    if (bytes) *bytes = tangent_record_bytes(c);
    return TRM_OK;
}

// ---- reverse-mode gradients of the heat-only run (trm_column_adjoint.hpp) -----------------------------------------------------
int trm_adjoint_open(trm_ctx* c, int capacity_steps) {
    TRM_ENTER_HEUN(c);
    if (capacity_steps < 1) return fail(c, TRM_EINVAL, "trm_adjoint_open: capacity_steps < 1");
    return open_adjoint(c, capacity_steps, 0, "trm_adjoint_open");
}
int trm_adjoint_open_checkpointed(trm_ctx* c, int capacity_slots, int interval) {
    TRM_ENTER_HEUN(c);
    if (capacity_slots < 1) return fail(c, TRM_EINVAL, "trm_adjoint_open_checkpointed: capacity_slots < 1");
    if (interval < 1 || interval > TRM_ADJOINT_MAX_INTERVAL)
        return fail(c, TRM_EINVAL, "trm_adjoint_open_checkpointed: the interval is 1 ... " + std::to_string(TRM_ADJOINT_MAX_INTERVAL));
    return open_adjoint(c, capacity_slots, interval, "trm_adjoint_open_checkpointed");
}
int trm_adjoint_checkpoints(const trm_ctx* c, int* interval, int* slots_used, int* slots_capacity) {
    if (!c) return TRM_EINVAL;
    if (int rc = adjoint_open(const_cast<trm_ctx*>(c), "trm_adjoint_checkpoints")) return rc;
    if (interval) *interval = c->ckpt_interval;
    if (slots_used) *slots_used = (int)tape_slots_used(c);
    if (slots_capacity) *slots_capacity = c->tape_cap;
    return TRM_OK;
}
int trm_adjoint_close(trm_ctx* c) {
    TRM_ENTER_HEUN(c);
    if (!c->d_adj[0]) return fail(c, TRM_EINVAL, "trm_adjoint_close: no adjoint is open");
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    release_adjoint(c);
    return TRM_OK;
}
int trm_adjoint_bc_open(trm_ctx* c) {
    TRM_ENTER_HEUN(c);
    if (int rc = richards_tape_only(c, "trm_adjoint_bc_open")) return rc;
    if (int rc = adjoint_open(c, "trm_adjoint_bc_open")) return rc;
    return open_adjoint_bc(c, false, "trm_adjoint_bc_open");
}
int trm_adjoint_bc_series_download(trm_ctx* c, int bc_var, int side, int nt, void* host) {
    TRM_ENTER_HEUN(c);
    int slot = -1;
    long have = 0;
    if (int rc = adjoint_bc_series_args(c, bc_var, side, host, "trm_adjoint_bc_series_download", slot, have)) return rc;
    if ((long)nt != have) return fail(c, TRM_EINVAL, "trm_adjoint_bc_series_download: nt must be the levels of the pair's series (" + std::to_string(have) + ")");
    TRM_HIP(c, hipMemcpyAsync(host, c->d_adj_bcs[slot], rows_bytes(c, nt), hipMemcpyDeviceToHost, c->stream));
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    return TRM_OK;
}
int trm_adjoint_bc_series_device_ptr(trm_ctx* c, int bc_var, int side, void** dev, int* nt) {
    TRM_ENTER_HEUN(c);
    int slot = -1;
    long have = 0;
    if (int rc = which_ok(c, 0, 1, nt, "trm_adjoint_bc_series_device_ptr")) return rc;
    if (int rc = adjoint_bc_series_args(c, bc_var, side, dev, "trm_adjoint_bc_series_device_ptr", slot, have)) return rc;
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    *dev = c->d_adj_bcs[slot];
    *nt = (int)have;
    return TRM_OK;
}
int trm_adjoint_bc_download(trm_ctx* c, int bc_var, int side, void* host) {
    TRM_ENTER_HEUN(c);
    int slot = -1;
    if (int rc = adjoint_bc_args(c, bc_var, side, host, "trm_adjoint_bc_download", slot)) return rc;
    TRM_HIP(c, hipMemcpyAsync(host, c->d_adj_bc[slot], rows_bytes(c), hipMemcpyDeviceToHost, c->stream));
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    return TRM_OK;
}
int trm_adjoint_bc_device_ptr(trm_ctx* c, int bc_var, int side, void** dev) {
    TRM_ENTER_HEUN(c);
    int slot = -1;
    if (int rc = adjoint_bc_args(c, bc_var, side, dev, "trm_adjoint_bc_device_ptr", slot)) return rc;
    *dev = c->d_adj_bc[slot];
    return TRM_OK;
}
int trm_adjoint_param_open(trm_ctx* c) {
    TRM_ENTER_HEUN(c);
    const char* who = "trm_adjoint_param_open";
    if (hydraulic_params_enabled(c)) return open_hydraulic_params(c, who);
    if (int rc = richards_tape_only(c, who)) return rc;
    // (a context the adjoint does not cover has none open: it is told why, not to open one)
    if (const char* why = derivative_unsupported(c)) return refuse(c, who, why);
    if (int rc = adjoint_open(c, who)) return rc;
    if (const char* why = thermal_params_not_differentiable(c)) return refuse(c, who, why, TRM_EINVAL);
    if (int rc = params_with_series_ok(c, c->opt_derivative_series != 0, who)) return rc;
    if (int rc = trm_adjoint_bc_open(c)) return rc;   // (the accumulating instances carry both)
    int rc = TRM_OK;
    for (double*& q : c->d_adj_param)
        if (!rc) rc = ensure(c, q, field_bytes(c), true, who, "the accumulators do not fit");
    if (!rc) rc = ensure(c, c->d_adj_param_out, rows_bytes(c, TRM_THERMAL_PARAM_COUNT), true, who, "the accumulators do not fit");
    if (rc) {
        release(c->d_adj_param);
        release(c->d_adj_param_out);
        return rc;
    }
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    return TRM_OK;
}
int trm_adjoint_param_download(trm_ctx* c, int which, void* host) {
    TRM_ENTER_HEUN(c);
    double* row = nullptr;
    if (int rc = adjoint_param_args(c, which, host, "trm_adjoint_param_download", row)) return rc;
    TRM_HIP(c, hipMemcpyAsync(host, row, rows_bytes(c), hipMemcpyDeviceToHost, c->stream));
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    return TRM_OK;
}
int trm_adjoint_param_device_ptr(trm_ctx* c, int which, void** dev) {
    TRM_ENTER_HEUN(c);
    double* row = nullptr;
    if (int rc = adjoint_param_args(c, which, dev, "trm_adjoint_param_device_ptr", row)) return rc;
    *dev = row;
    return TRM_OK;
}
int trm_adjoint_upload(trm_ctx* c, int which, const void* host) {
    TRM_ENTER_HEUN(c);
    if (int rc = adjoint_open(c, "trm_adjoint_upload")) return rc;
    if (int rc = which_ok(c, which, adjoint_fields(c), host, "trm_adjoint_upload")) return rc;
    return upload_3d<double>(c, (const double*)host, c->d_adj[which]);
}
int trm_adjoint_download(trm_ctx* c, int which, void* host) {
    TRM_ENTER_HEUN(c);
    if (int rc = adjoint_open(c, "trm_adjoint_download")) return rc;
    if (int rc = which_ok(c, which, adjoint_fields(c), host, "trm_adjoint_download")) return rc;
    return download_3d<double>(c, c->d_adj[which], (double*)host);
}
int trm_adjoint_device_ptr(trm_ctx* c, int which, void** dev, int64_t* pitch_elems) {
    TRM_ENTER_HEUN(c);
    if (int rc = adjoint_open(c, "trm_adjoint_device_ptr")) return rc;
    if (int rc = which_ok(c, which, adjoint_fields(c), dev, "trm_adjoint_device_ptr")) return rc;
    if (int rc = which_ok(c, 0, 1, pitch_elems, "trm_adjoint_device_ptr")) return rc;
    *dev = c->d_adj[which];
    *pitch_elems = c->Nzp;
    return TRM_OK;
}
int trm_adjoint_tape(const trm_ctx* c, int* recorded, int* capacity) {
    if (!c) return TRM_EINVAL;
    if (int rc = adjoint_open(const_cast<trm_ctx*>(c), "trm_adjoint_tape")) return rc;
    if (recorded) *recorded = taped_steps(c);
    if (capacity) *capacity = (int)std::min<long long>((long long)c->tape_cap * std::max(c->ckpt_interval, 1), std::numeric_limits<int>::max());
    return TRM_OK;
}
int trm_step_record(trm_ctx* c, double dt, int nsteps) {
    TRM_ENTER(c);
    const char* who = "trm_step_record";
    if (int rc = adjoint_open(c, who)) return rc;
    if (nsteps < 0) return fail(c, TRM_EINVAL, "trm_step_record: nsteps < 0");
    const int K = c->ckpt_interval;
    const long long need = tape_slots_needed(c, dt, nsteps), used = tape_slots_used(c);
    if (need > c->tape_cap - used)
        return fail(c, TRM_EINVAL, "trm_step_record: " + std::to_string(nsteps) + (K ? " steps need " + std::to_string(need) + " checkpoints (" : " steps do not fit the tape (") +
                                       std::to_string(used) + " of " + std::to_string(c->tape_cap) + " slots taken)");
    if (const char* why = derivative_step_unsupported(c, false, true)) return refuse(c, who, why);
    const int nser = derivative_series_count(c);
    if (int rc = params_with_series_ok(c, c->d_adj_param_out != nullptr, who)) return rc;
    if (c->adj_stale) return fail(c, TRM_ESTALE, std::string(who) + kStaleTape);
    if (nsteps > 0) c->tan_stale = true;       // (a state-changing call for an open tangent)
    const int spl = derivative_steps_per_launch(c);
    if (richards(c)) {      // (final-state cotangents alone: no series, no ride -- the launches of trm_step's multi-step program)
        for (int n = 0, m; n < nsteps; n += m) {
            m = std::min(spl, nsteps - n);
            int rc = Unfused<double>::update_inputs(c, c->state, c->time);
            if (!rc) rc = AdjointRichLaunch::record(c, dt, m, (int)c->tape_dt.size());
            if (rc) {
                c->adj_stale = taped_steps(c) > 0;
                return rc;
            }
            c->derivative_series = 0;
            tape_append(c, dt, m);
            tick(c, dt, m);
        }
        return derivative_steps_done(c);
    }
    for (int n = 0, m; n < nsteps; n += m) {
        m = std::min(spl, nsteps - n);
        // (with series: the rows of the launch's steps stay with the tape, [taped step][series])
        const size_t rows_before = c->tape_rows.size();
        int rc = nser ? Unfused<double>::upload_series_rows(c, dt, m, &c->tape_rows) : Unfused<double>::update_inputs(c, c->state, c->time);
        // (checkpointed: the launch stores before its steps room, room + K, ... -- the starts of the segments it opens)
        if (!rc) rc = K ? CheckpointLaunch::record(c, dt, m, (int)c->tape_segs.size(), open_segment_room(c, dt), K, nser != 0) : AdjointLaunch::record(c, dt, m, (int)c->tape_dt.size(), nser != 0);
        if (rc) {
            c->tape_rows.resize(rows_before);
            c->adj_stale = taped_steps(c) > 0;
            return rc;
        }
        c->derivative_series = nser;
        tape_append(c, dt, m);
        tick(c, dt, m);
    }
    return derivative_steps_done(c);
}
int trm_adjoint_backward(trm_ctx* c) {
    TRM_ENTER(c);
    const char* who = "trm_adjoint_backward";
    if (int rc = adjoint_open(c, who)) return rc;
    if (const char* why = derivative_step_unsupported(c, false, true)) return refuse(c, who, why);
    const int nser = derivative_series_count(c);
    if (int rc = params_with_series_ok(c, c->d_adj_param_out != nullptr, who)) return rc;
    if (c->adj_stale) return fail(c, TRM_ESTALE, std::string(who) + kStaleTape);
    // An attached record (trm_adjoint_observe_record; on a Richards context the soil-moisture record of TRM_OPT_DERIVATIVE_RICHARDS_RECORD)
    // is read inside the launches: no position of it is a launch boundary.  A record longer than the tape is refused here, in front of
    // everything the sweep does
    const bool rec = c->rec.npos > 0;
    if (int rc = record_fits_tape(c, taped_steps(c), who)) return rc;
    if (rec)
        if (int rc = record_tables(c, taped_steps(c), who)) return rc;
    if (richards(c)) {
        // one launch per block of the tape (tape_block_begin), newest block first; the first launch folds the cotangents of T, liq and psi
        // in (an empty tape: that launch alone).  With the hydraulic-parameter gradients open the launches carry their sums, and
        // k_hyd_param_reduce ends the sweep
        const bool hyd = c->d_adj_hyd_out != nullptr;
        const int spl = derivative_steps_per_launch(c);
        int end = (int)c->tape_dt.size(), fold = 1;
        do {
            const int begin = tape_block_begin(c, end, spl);
            const double dt_block = end > 0 ? c->tape_dt[(size_t)end - 1] : 0.0;
            if (int rc = AdjointRichLaunch::backward(c, dt_block, end - begin, begin, fold, hyd, rec)) {
                c->adj_stale = true;       // (lam is part way down the tape)
                return rc;
            }
            c->derivative_series = 0;
            end = begin;
            fold = 0;
        } while (end > 0);
        if (rec) {                 // (the residuals the launches wrote, summed in front of k_hyd_param_reduce)
            const int rc = RecordLaunch::misfit(c);
            c->rec_swept = rc == TRM_OK;
            if (rc) {
                c->adj_stale = true;
                return rc;
            }
        }
        c->tape_dt.clear();
        c->adj_stale = false;
        return finish(c, hyd ? AdjointRichLaunch::param_reduce(c) : TRM_OK);
    }
    if (nser) {
        // series ride with the accumulating instances: the per-column accumulators if nobody has opened them, and the node accumulators,
        // zero in front of the sweep's first launch; every launch gets the rows the record kept for its steps
        if (c->tape_rows.size() != (size_t)taped_steps(c) * (size_t)nser)
            return fail(c, TRM_ESTALE, "trm_adjoint_backward: the tape was recorded without the series the context holds now: trm_adjoint_open starts a new tape");
        if (int rc = open_adjoint_bc(c, true, who)) return rc;
        for (const auto& sr : c->series) {
            const int slot = bc_pair_index(sr.var, sr.side);
            if (int rc = alloc_series_shaped(c, c->d_adj_bcs[slot], c->adj_bcs_nt[slot], sr.cap, who)) return rc;
            if (int rc = zero(c, c->d_adj_bcs[slot], rows_bytes(c, sr.cap))) return rc;
        }
    }
    // (the rows of taped steps [first, first + n), uploaded in front of the launch that walks them)
    auto kept_rows = [&](int first, int n) { return Unfused<double>::upload_series_rows(c, 0.0, n, nullptr, c->tape_rows.data() + (size_t)first * (size_t)nser); };
    const Ride ride = backward_ride(c, nser);
    // Observations (trm_adjoint_observe*): those of position p enter in front of the launch whose newest step is p - 1.  The launch that
    // folds starts its boundary and parameter sums from 0, so the observations of p = n give lam their share in front of it and the
    // parameter sums theirs behind it; those of p = 0 < n follow the last launch.
    const int n = taped_steps(c);
    int rc = TRM_OK, fold = 1;
    if (c->ckpt_interval) {   // one launch per segment, newest first; the first launch folds (an empty tape: that launch alone, no step)
        size_t s = c->tape_segs.size();
        do {
            const trm_ctx::TapeSegment seg = s > 0 ? c->tape_segs[s - 1] : trm_ctx::TapeSegment{0, 0, 0.0, 0};
            rc = inject_observations(c, seg.first + seg.len, true, !fold);   // (a segment ends at every observed position)
            if (!rc) rc = nser ? kept_rows(seg.first, seg.len) : TRM_OK;
            if (!rc) rc = CheckpointLaunch::backward(c, seg.dt, seg.len, seg.slot, fold, ride, rec, seg.first);
            if (!rc && fold) rc = inject_observations(c, n, false, true);
            if (rc) break;
            c->derivative_series = nser;
            fold = 0;
            if (s > 0) --s;
        } while (s > 0);
    } else {
        // one launch per block of the tape (tape_block_begin), newest block first; the first launch folds the cotangents of T and liq in
        // (an empty tape: that launch alone)
        const int spl = derivative_steps_per_launch(c);
        int end = (int)c->tape_dt.size();
        do {
            const int begin = tape_block_begin(c, end, spl);
            const double dt_block = end > 0 ? c->tape_dt[(size_t)end - 1] : 0.0;
            rc = inject_observations(c, end, true, !fold);
            if (!rc) rc = nser ? kept_rows(begin, end - begin) : TRM_OK;
            if (!rc) rc = AdjointLaunch::backward(c, dt_block, end - begin, begin, fold, ride, rec, begin);
            if (!rc && fold) rc = inject_observations(c, n, false, true);
            if (rc) break;
            c->derivative_series = nser;
            end = begin;
            fold = 0;
        } while (end > 0);
    }
    if (!rc && n > 0) rc = inject_observations(c, 0, true, true);
    if (!rc && rec) {          // (the residuals the launches wrote, summed in front of k_param_reduce)
        rc = RecordLaunch::misfit(c);
        c->rec_swept = rc == TRM_OK;
    }
    if (rc) {
        c->adj_stale = true;       // (lam is part way down the tape)
        return rc;
    }
    if (!c->observations.empty()) {   // (the launches above read them)
        TRM_HIP(c, hipStreamSynchronize(c->stream));
        drop_observations(c);
    }
    if (int rc0 = zero(c, c->d_misfit, rows_bytes(c))) return rc0;
    c->tape_segs.clear();
    c->tape_dt.clear();
    c->tape_rows.clear();
    c->adj_stale = false;
    return finish(c, c->d_adj_param_out ? AdjointLaunch::param_reduce(c) : TRM_OK);
}

// ---- adjoint observations: cotangents at taped positions (trm_launch_observe.hip) ----------------------------------------------------
int trm_adjoint_observe(trm_ctx* c, int which, int nlevels, const int32_t* levels, const void* host) {
    TRM_ENTER_HEUN(c);
    const char* who = "trm_adjoint_observe";
    if (int rc = observe_args(c, nlevels, levels, host, who)) return rc;
    if (int rc = which_ok(c, which, TRM_ADJOINT_LIQUID_WATER_FRACTION + 1, host, who, " (TRM_ADJOINT_*)")) return rc;
    return register_observation(c, which, nlevels, levels, host, nullptr, who);
}
int trm_adjoint_observe_misfit(trm_ctx* c, int nlevels, const int32_t* levels, const void* observed, const void* weight) {
    TRM_ENTER_HEUN(c);
    const char* who = "trm_adjoint_observe_misfit";
    if (int rc = observe_args(c, nlevels, levels, observed, who)) return rc;
    if (weight) {
        const double* w = (const double*)weight;
        for (size_t q = 0, end = (size_t)nlevels * (size_t)c->Nh; q < end; ++q)
            if (!(w[q] >= 0.0)) return fail(c, TRM_EINVAL, "trm_adjoint_observe_misfit: a weight is negative or NaN");
    }
    if (int rc = ensure(c, c->d_misfit, rows_bytes(c), false, who, "the misfit accumulator does not fit")) return rc;
    if (int rc = register_observation(c, trm_ctx::OBSERVE_MISFIT, nlevels, levels, observed, weight, who)) return rc;
    if (int rc = ObserveLaunch::misfit(c, c->observations.back())) return rc;
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    return TRM_OK;
}
int trm_adjoint_misfit_download(trm_ctx* c, void* host) {
    TRM_ENTER_HEUN(c);
    const char* who = "trm_adjoint_misfit_download";
    if (int rc = adjoint_open(c, who)) return rc;
    if (int rc = which_ok(c, 0, 1, host, who)) return rc;
    if (!c->d_misfit) {        // (no misfit observation yet)
        std::fill((double*)host, (double*)host + c->Nh, 0.0);
        return TRM_OK;
    }
    TRM_HIP(c, hipMemcpyAsync(host, c->d_misfit, rows_bytes(c), hipMemcpyDeviceToHost, c->stream));
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    return TRM_OK;
}
int trm_adjoint_misfit_device_ptr(trm_ctx* c, void** dev) {
    TRM_ENTER_HEUN(c);
    const char* who = "trm_adjoint_misfit_device_ptr";
    if (int rc = adjoint_open(c, who)) return rc;
    if (int rc = which_ok(c, 0, 1, dev, who)) return rc;
    if (int rc = ensure(c, c->d_misfit, rows_bytes(c), false, who, "the misfit accumulator does not fit")) return rc;
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    *dev = c->d_misfit;
    return TRM_OK;
}
// ---- attached records: a temperature record read inside the backward launches (trm_launch_record.hip) -------------------------------
int trm_adjoint_observe_record(trm_ctx* c, int npos, const int32_t* positions, int nlevels, const int32_t* levels, const void* observed, const void* weight) {
    TRM_ENTER_HEUN(c);
    return attach_record(c, npos, positions, nlevels, levels, observed, weight, false, "trm_adjoint_observe_record");
}
int trm_adjoint_observe_record_device(trm_ctx* c, int npos, const int32_t* positions, int nlevels, const int32_t* levels, const void* d_observed, const void* d_weight) {
    TRM_ENTER_HEUN(c);
    return attach_record(c, npos, positions, nlevels, levels, d_observed, d_weight, true, "trm_adjoint_observe_record_device");
}
int trm_adjoint_record_detach(trm_ctx* c) {
    TRM_ENTER_HEUN(c);
    const char* who = "trm_adjoint_record_detach";
    if (int rc = richards_tape_only(c, who, true)) return rc;
    if (int rc = adjoint_open(c, who)) return rc;
    if (c->rec.npos == 0) return fail(c, TRM_EINVAL, std::string(who) + ": no record is attached (trm_adjoint_observe_record)");
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    drop_record(c);
    return TRM_OK;
}
int trm_adjoint_record_residual_download(trm_ctx* c, void* host) {
    TRM_ENTER_HEUN(c);
    if (int rc = richards_tape_only(c, "trm_adjoint_record_residual_download", true)) return rc;
    if (int rc = record_results_ok(c, host, "trm_adjoint_record_residual_download")) return rc;
    TRM_HIP(c, hipMemcpyAsync(host, c->d_rec_out, rows_bytes(c, (long)c->rec.npos * c->rec.nlevels), hipMemcpyDeviceToHost, c->stream));
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    return TRM_OK;
}
int trm_adjoint_record_residual_device_ptr(trm_ctx* c, void** dev) {
    TRM_ENTER_HEUN(c);
    if (int rc = richards_tape_only(c, "trm_adjoint_record_residual_device_ptr", true)) return rc;
    if (int rc = record_results_ok(c, dev, "trm_adjoint_record_residual_device_ptr")) return rc;
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    *dev = c->d_rec_out;
    return TRM_OK;
}
int trm_adjoint_record_misfit_download(trm_ctx* c, void* host) {
    TRM_ENTER_HEUN(c);
    if (int rc = richards_tape_only(c, "trm_adjoint_record_misfit_download", true)) return rc;
    if (int rc = record_results_ok(c, host, "trm_adjoint_record_misfit_download")) return rc;
    TRM_HIP(c, hipMemcpyAsync(host, c->d_rec_out + (size_t)c->rec.npos * (size_t)c->rec.nlevels * (size_t)c->Nh, rows_bytes(c), hipMemcpyDeviceToHost, c->stream));
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    return TRM_OK;
}
int trm_adjoint_record_info(const trm_ctx* c, int* npos, int* nlevels, int64_t* bytes) {
    if (!c) return TRM_EINVAL;
    if (int rc = richards_tape_only(const_cast<trm_ctx*>(c), "trm_adjoint_record_info", true)) return rc;
    if (int rc = adjoint_open(const_cast<trm_ctx*>(c), "trm_adjoint_record_info")) return rc;
    if (npos) *npos = c->rec.npos;
    if (nlevels) *nlevels = c->rec.nlevels;
    if (bytes) *bytes = record_bytes(c);
    return TRM_OK;
}
int trm_adjoint_observations(const trm_ctx* c, int* count, int64_t* bytes) {
    if (!c) return TRM_EINVAL;
    if (int rc = adjoint_open(const_cast<trm_ctx*>(c), "trm_adjoint_observations")) return rc;
    int64_t sum = 0;
    for (const auto& o : c->observations) sum += o.bytes(c->Nh);
    if (count) *count = (int)c->observations.size();
    if (bytes) *bytes = sum;
    return TRM_OK;
}

}  // extern "C"
