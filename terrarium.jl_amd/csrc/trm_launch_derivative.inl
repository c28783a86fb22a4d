// trm_launch_derivative.inl -- the launches of the two derivative families of the heat-only fp64 SoilModel run: k_column_tangent
// (trm_column_tangent.hpp), k_column_record / k_column_adjoint (trm_column_adjoint.hpp) and k_column_adjoint_ckpt
// (trm_column_adjoint_ckpt.hpp), each with what rides along (Ride, trm_kernels.hpp), and their record twins: k_column_tangent_record
// (trm_column_tangent_record.hpp; DESIGN 4.7 "Tangent records"), k_column_adjoint_record and k_column_adjoint_ckpt_record (DESIGN 4.8
// "Attached records").  A sweep and its record twin are the two wrappers of one device program (adjoint_program,
// adjoint_ckpt_program <.., RECORD>); the two tangent kernels are two bodies.  Behind them the heat + Richards families:
// k_column_tangent_rich, k_column_record_rich and the four wrappers of adjoint_rich_program <.., PARAMS, RECORD>.  Included by the
// trm_launch_column_tangent*.hip and trm_launch_column_adjoint*.hip files, each of which
// instantiates the launcher of one family and ride, with a record or without.
#include "trm_host.hpp"
#include "trm_column_adjoint_ckpt.hpp"
#include "trm_column_tangent_record.hpp"
#include "trm_column_tangent_rich.hpp"
#include "trm_column_adjoint_rich.hpp"

namespace trmh {

// ---- what a ride is called in a refusal ----------------------------------------------------------------------------------------------
inline std::string ride_name(const char* kernel, Ride r, bool tangent) {
    const char* seeds[] = {"", " (boundary seeds)", " (parameter seeds)", " (series)", " (series, parameter seeds)"};
    const char* grads[] = {"", " (boundary gradients)", " (parameter gradients)", " (series)", " (series, parameter gradients)"};
    return std::string(kernel) + (tangent ? seeds : grads)[r];
}

// ---- the argument fillers ----------------------------------------------------------------------------------------------------------
// the halo form trm_step would take; the series instances refuse the generic kinds (series_ok)
inline int generic_halos(trm_ctx* c, bool series) { return !series && Policy<double>::generic_bcs(c) ? 1 : 0; }

inline void fill_tangent(trm_ctx* c, TangentFields& ta, bool series) {
    ta.dU = c->d_tan[TRM_TANGENT_INTERNAL_ENERGY];
    ta.dT = c->d_tan[TRM_TANGENT_TEMPERATURE];
    ta.dliq = c->d_tan[TRM_TANGENT_LIQUID_WATER_FRACTION];
    ta.generic = generic_halos(c, series);
}
// the seeds of the boundary values, and of the thermal parameters or the seriesed pairs behind them
template <Ride R> void fill_tangent_seeds(const trm_ctx* c, TangentArgs<R>& ta) {
    if constexpr (ride_has_bc(R)) {
        ta.sTb = c->d_tan_bc[0];
        ta.sTt = c->d_tan_bc[1];
        ta.sUb = c->d_tan_bc[2];
        ta.sUt = c->d_tan_bc[3];
    }
    if constexpr (ride_has_params(R)) {
        const double* s = c->tan_param;
        ta.s = ParamSeeds{s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7]};
    }
    if constexpr (ride_has_series(R))
        for (int s = 0; s < 4; ++s) ta.sn[s] = c->d_tan_bcs[s];
}
// the cotangent fields and the tape; `slot`: the tape slot of the first step of the launch, or the segment's checkpoint
inline void fill_cotangent(trm_ctx* c, TapeFields& aa, int slot, int fold, bool series) {
    aa.lU = c->d_adj[TRM_ADJOINT_INTERNAL_ENERGY];
    aa.lT = c->d_adj[TRM_ADJOINT_TEMPERATURE];
    aa.lliq = c->d_adj[TRM_ADJOINT_LIQUID_WATER_FRACTION];
    aa.slot_elems = (long long)c->Nh * (long long)c->Nzp;
    aa.tape = c->d_tape + (size_t)slot * (size_t)aa.slot_elems;
    aa.generic = generic_halos(c, series);
    aa.fold = fold;
}
inline BcGradPtrs bc_grad_ptrs(const trm_ctx* c) { return BcGradPtrs{c->d_adj_bc[0], c->d_adj_bc[1], c->d_adj_bc[2], c->d_adj_bc[3]}; }
inline SeriesGradPtrs series_grad_ptrs(const trm_ctx* c) { return SeriesGradPtrs{{c->d_adj_bcs[0], c->d_adj_bcs[1], c->d_adj_bcs[2], c->d_adj_bcs[3]}}; }
inline ParamGradPtrs param_grad_ptrs(const trm_ctx* c) {
    ParamGradPtrs g;
    for (int q = 0; q < 8; ++q) g.g[q] = c->d_adj_param[q];
    return g;
}
// what rides along a backward launch on either tape
template <bool CKPT, Ride R> void fill_gradients(const trm_ctx* c, SweepArgs<CKPT, R>& aa) {
    if constexpr (ride_has_bc(R)) aa.g = bc_grad_ptrs(c);
    if constexpr (ride_has_params(R)) aa.pg = param_grad_ptrs(c);
    if constexpr (ride_has_series(R)) aa.sg = series_grad_ptrs(c);
}

// ---- the preconditions -------------------------------------------------------------------------------------------------------------
// the per-step tape: the launch's steps are the slots [slot, slot + nsteps)
inline int tape_range_ok(trm_ctx* c, int nsteps, int slot, const std::string& who) {
    if (slot < 0 || nsteps < 0 || slot + nsteps > c->tape_cap) return fail(c, TRM_EINVAL, who + ": the launch leaves the tape");
    return TRM_OK;
}
// a segment of the checkpointed tape: its checkpoint is in `slot`
inline int segment_range_ok(trm_ctx* c, int nsteps, int slot, const std::string& who) {
    if (slot < 0 || nsteps < 0 || nsteps > TRM_ADJOINT_MAX_INTERVAL || slot >= c->tape_cap) return fail(c, TRM_EINVAL, who + ": the launch leaves the tape");
    return TRM_OK;
}
// the strided record: its stores are the slots from `slot` on
inline int strided_stores_ok(trm_ctx* c, int nsteps, int& slot, int first, int every, const std::string& who) {
    if (slot < 0 || nsteps < 0 || first < 0 || every < 1) return fail(c, TRM_EINVAL, who + ": bad launch");
    const int stores = first < nsteps ? (nsteps - first + every - 1) / every : 0;
    if (slot + stores > c->tape_cap) return fail(c, TRM_EINVAL, who + ": the launch leaves the tape");
    if (stores == 0) slot = 0;     // (no store: any address inside the tape)
    return TRM_OK;
}
// accumulators / seed arrays present
template <size_t N> int arrays_ok(trm_ctx* c, double* const (&arrays)[N], const std::string& who, const char* what) {
    for (const double* q : arrays)
        if (!q) return fail(c, TRM_EINVAL, who + ": no " + what);
    return TRM_OK;
}
// what every series launch needs: the table, rows for its steps, the branch-free boundary kinds ...
inline int series_rows_ok(trm_ctx* c, int nsteps, const std::string& who) {
    if (!c->d_series_table || (nsteps > 0 && !c->d_series_rows) || Policy<double>::generic_bcs(c))
        return fail(c, TRM_EINVAL, who + ": no series rows, or the generic boundary kinds");
    return TRM_OK;
}
// ... and one that carries derivatives: node arrays (d_tan_bcs / d_adj_bcs, `nt` nodes each) of the shape of every series
inline int series_nodes_ok(trm_ctx* c, double* const (&nodes)[4], const long (&nt)[4], const std::string& who, const char* what) {
    for (const auto& sr : c->series) {
        const int slot = Policy<double>::series_slot(c, sr);
        if (slot < SLOT_T_BOT || slot > SLOT_FU_TOP || !nodes[slot] || nt[slot] != sr.cap) return fail(c, TRM_EINVAL, who + ": a series without " + what + " of its shape");
    }
    return TRM_OK;
}
// the accumulators a backward launch with ride R needs
template <Ride R> int gradients_ok(trm_ctx* c, int nsteps, const std::string& who) {
    if constexpr (ride_has_series(R))
        if (int rc = series_rows_ok(c, nsteps, who)) return rc;
    if constexpr (ride_has_bc(R))
        if (int rc = arrays_ok(c, c->d_adj_bc, who, ride_has_params(R) ? "boundary accumulators" : "accumulators")) return rc;
    if constexpr (ride_has_params(R))
        if (int rc = arrays_ok(c, c->d_adj_param, who, "accumulators")) return rc;
    if constexpr (ride_has_series(R))
        if (int rc = series_nodes_ok(c, c->d_adj_bcs, c->adj_bcs_nt, who, "an accumulator")) return rc;
    return TRM_OK;
}
// the seed arrays a tangent launch with ride R needs (the parameter seeds travel by value)
template <Ride R> int tangent_seeds_ok(trm_ctx* c, int nsteps, const std::string& who) {
    if constexpr (ride_has_bc(R))
        if (int rc = arrays_ok(c, c->d_tan_bc, who, ride_has_params(R) ? "boundary seed arrays" : "seed arrays")) return rc;
    if constexpr (ride_has_series(R)) {
        if (int rc = series_rows_ok(c, nsteps, who)) return rc;
        if (int rc = series_nodes_ok(c, c->d_tan_bcs, c->tan_bcs_nt, who, "seeds")) return rc;
    }
    return TRM_OK;
}

// ---- the records a RECORD launch carries as its fifth kernel argument -------------------------------------------------------------
// the attached temperature record as a backward launch whose first step is taped position `first` sees it
inline RecordArgs record_args(const trm_ctx* c, int first) {
    RecordArgs r;
    r.row_of_level = record_row_of_level(c->rec);
    r.row_of_position = record_row_of_position(c->rec, c->Nz, first);
    r.observed = c->d_rec_observed;
    r.weight = c->d_rec_weight;
    r.residual = c->d_rec_out;
    r.nlevels = c->rec.nlevels;
    return r;
}
// the tables are those of this tape, and the launch's positions first ... first + nsteps are inside them
inline int record_launch_ok(trm_ctx* c, int nsteps, int first, const std::string& who) {
    if (c->rec.npos < 1 || !c->rec.d_tables || !c->d_rec_observed || !c->d_rec_out || c->rec.entries < 1)
        return fail(c, TRM_EINVAL, who + ": no record is attached, or its tables are not built");
    if (!record_table_covers(c->rec, first, nsteps)) return fail(c, TRM_EINVAL, who + ": the launch leaves the record's position table");
    return TRM_OK;
}
// the tangent record as a launch whose first state is position `start` of the record's count sees it
inline TangentRecordArgs tangent_record_args(const trm_ctx* c, long long start) {
    TangentRecordArgs r;
    r.row_of_level = record_row_of_level(c->trec);
    r.row_of_position = record_row_of_position(c->trec, c->Nz, start);
    r.T = c->d_trec[TRM_TANGENT_RECORD_TEMPERATURE];
    r.dT = c->d_trec[TRM_TANGENT_RECORD_TANGENT];
    r.nlevels = c->trec.nlevels;
    r.sample_entry = start == 0 ? 1 : 0;
    return r;
}
// the tables and the sample arrays are those of the attached record, and the launch's positions trec_position ... trec_position + nsteps
// are inside the position table (the caller clips a launch to it: tangent_record_steps)
inline int tangent_record_launch_ok(trm_ctx* c, int nsteps, const std::string& who) {
    if (c->trec.npos < 1 || c->trec.nlevels < 1 || c->trec.positions.empty() || !c->trec.d_tables || !c->d_trec[0] || !c->d_trec[1])
        return fail(c, TRM_EINVAL, who + ": no record is attached, or its tables are not built");
    if ((int)c->trec.positions.size() != c->trec.npos || (int)c->trec.levels.size() != c->trec.nlevels || c->trec.nlevels > c->Nz)
        return fail(c, TRM_EINVAL, who + ": the sample arrays do not have the attached shape");
    if (!record_table_covers(c->trec, c->trec_position, nsteps)) return fail(c, TRM_EINVAL, who + ": the launch leaves the record's position table");
    return TRM_OK;
}

// ---- the dispatch over (hydraulics instance, lanes per column): launch(H, LPC), both std::integral_constant -----------------------
template <class F> int by_instance(trm_ctx* c, F&& launch) {
    int rc = TRM_OK;
    by_hyd(Policy<double>::hyd(c), [&](auto H) { by_lanes(c->Nz, [&](auto LPC) { rc = launch(H, LPC); }); });
    return rc;
}
// TRM_INFO_LAST_PROGRAM of a derivative launch: the instance and the family bits (trm_host.hpp)
inline int derivative_program_id(int family, int hyd, int lpc, int generic, int bits) {
    return program_id(family, hyd, lpc, DERIVE_NONE, 0, 0, -1) | (generic ? PROGRAM_GENERIC_HALOS : 0) | bits;
}

// ---- one launch function per kernel template ----------------------------------------------------------------------------------------
template <Ride R, bool RECORD> int tangent_step(trm_ctx* c, double dt, int nsteps) {
    const std::string who = ride_name(RECORD ? "k_column_tangent_record" : "k_column_tangent", R, true);
    if (int rc = tangent_seeds_ok<R>(c, nsteps, who)) return rc;
    if constexpr (RECORD)
        if (int rc = tangent_record_launch_ok(c, nsteps, who)) return rc;
    const LaunchArgs<double>& la = launch_args<double>(c);
    const ColumnArgs<double> a = column_args<double>(c, dt, 1, nsteps, PROG_EULER);
    TangentArgs<R> ta;
    fill_tangent(c, ta, ride_has_series(R));
    fill_tangent_seeds(c, ta);
    const TangentRecordArgs r = RECORD ? tangent_record_args(c, c->trec_position) : TangentRecordArgs{};
    return by_instance(c, [&](auto h, auto lpc) {
        constexpr int H = decltype(h)::value, LPC = decltype(lpc)::value;
        if constexpr (RECORD) hipLaunchKernelGGL((k_column_tangent_record<H, LPC, R>), column_grid(c, LPC), dim3(TRM_STEP_BLOCK), 0, c->stream, la.state, la.p, a, ta, r);
        else hipLaunchKernelGGL((k_column_tangent<H, LPC, R>), column_grid(c, LPC), dim3(TRM_STEP_BLOCK), 0, c->stream, la.state, la.p, a, ta);
        TRM_HIP(c, hipGetLastError());
        c->last_program = derivative_program_id(TRM_PROGRAM_COLUMN_TANGENT, H, LPC, ta.generic,
                                                (ride_has_bc(R) ? PROGRAM_BC_SEEDS : 0) | (ride_has_params(R) ? (int)TRM_PROGRAM_PARAMETERS : 0));
        return (int)TRM_OK;
    });
}

// trm_tangent_closure: with the heat-capacity term of the parameter seeds (RIDE_PARAM) or without (RIDE_NONE); the closure reads no
// boundary value, so these two are the only instances and every other ride takes RIDE_NONE's (closure_ride, trm_derivative_api.hip)
template <Ride R> int tangent_closure(trm_ctx* c) {
    static_assert(R == RIDE_NONE || R == RIDE_PARAM, "k_closure_tangent has these two instances");
    const LaunchArgs<double>& la = launch_args<double>(c);
    const size_t cells = (size_t)c->Nh * (size_t)c->Nzp;
    TangentArgs<R> ta;
    fill_tangent(c, ta, false);
    fill_tangent_seeds(c, ta);
    hipLaunchKernelGGL((k_closure_tangent<R>), dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, c->stream, la.state, la.p, ta);
    TRM_HIP(c, hipGetLastError());
    return TRM_OK;
}

// ---- the heat + Richards tangent (k_column_tangent_rich, trm_column_tangent_rich.hpp; TRM_OPT_DERIVATIVE_RICHARDS): state seeds alone, no
// ride.  Templates so that only the translation unit that instantiates them (trm_launch_column_tangent_rich.hip) holds the kernels.
// The preconditions: a Richards context, the branch-free boundary kinds (the generic halos are not part of the kernel), the five fields
inline int tangent_rich_ok(trm_ctx* c, const std::string& who) {
    if (c->params.flow != TRM_FLOW_RICHARDS) return fail(c, TRM_EINVAL, who + ": a Richards context only");
    if (Policy<double>::generic_bcs(c)) return fail(c, TRM_EINVAL, who + ": the generic boundary kinds");
    return arrays_ok(c, c->d_tan, who, "tangent fields");
}
inline RichTangentArgs rich_tangent_args(const trm_ctx* c) {
    return RichTangentArgs{c->d_tan[TRM_TANGENT_INTERNAL_ENERGY], c->d_tan[TRM_TANGENT_SATURATION], c->d_tan[TRM_TANGENT_TEMPERATURE],
                           c->d_tan[TRM_TANGENT_LIQUID_WATER_FRACTION], c->d_tan[TRM_TANGENT_PRESSURE_HEAD]};
}
template <class = void> int tangent_step_rich(trm_ctx* c, double dt, int nsteps) {
    const std::string who = "k_column_tangent_rich";
    if (int rc = tangent_rich_ok(c, who)) return rc;
    if (nsteps < 0) return fail(c, TRM_EINVAL, who + ": bad launch");
    const LaunchArgs<double>& la = launch_args<double>(c);
    const ColumnArgs<double> a = column_args<double>(c, dt, 1, nsteps, PROG_MULTI);
    const RichTangentArgs ta = rich_tangent_args(c);
    return by_instance(c, [&](auto h, auto lpc) {
        constexpr int H = decltype(h)::value, LPC = decltype(lpc)::value;
        hipLaunchKernelGGL((k_column_tangent_rich<H, LPC>), column_grid(c, LPC), dim3(TRM_STEP_BLOCK), 0, c->stream, la.state, la.p, a, ta);
        TRM_HIP(c, hipGetLastError());
        c->last_program = derivative_program_id(TRM_PROGRAM_COLUMN_TANGENT_RICHARDS, H, LPC, 0, 0);
        return (int)TRM_OK;
    });
}
template <class = void> int tangent_closure_rich(trm_ctx* c) {
    if (int rc = tangent_rich_ok(c, "k_closure_tangent_rich")) return rc;
    const LaunchArgs<double>& la = launch_args<double>(c);
    const size_t cells = (size_t)c->Nh * (size_t)c->Nzp;
    const RichTangentArgs ta = rich_tangent_args(c);
    int rc = TRM_OK;
    by_hyd(Policy<double>::hyd(c), [&](auto h) {
        hipLaunchKernelGGL((k_closure_tangent_rich<decltype(h)::value>), dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, c->stream, la.state, la.p, ta);
        if (hipGetLastError() != hipSuccess) rc = fail(c, TRM_EHIP, "k_closure_tangent_rich: the launch failed");
    });
    return rc;
}

// ---- the heat + Richards adjoint (k_column_record_rich / k_column_adjoint_rich, trm_column_adjoint_rich.hpp;
// TRM_OPT_DERIVATIVE_RICHARDS_ADJOINT): final-state cotangents on the per-step tape, no ride.  Templates so that only the translation units
// that instantiate them (trm_launch_column_adjoint_rich*.hip) hold the kernels.  A slot holds two fields, U_k and sat_k.
// The preconditions: a Richards context, the branch-free boundary kinds, the five cotangent fields, the launch's slots inside the tape
inline int adjoint_rich_ok(trm_ctx* c, int nsteps, int slot, const std::string& who) {
    if (c->params.flow != TRM_FLOW_RICHARDS) return fail(c, TRM_EINVAL, who + ": a Richards context only");
    if (Policy<double>::generic_bcs(c)) return fail(c, TRM_EINVAL, who + ": the generic boundary kinds");
    if (int rc = arrays_ok(c, c->d_adj, who, "cotangent fields")) return rc;
    if (!c->d_tape || c->ckpt_interval != 0) return fail(c, TRM_EINVAL, who + ": no per-step tape");
    return tape_range_ok(c, nsteps, slot, who);
}
inline long long rich_slot_elems(const trm_ctx* c) { return (long long)c->Nh * (long long)c->Nzp; }
inline RichTapeArgs rich_tape_args(const trm_ctx* c, int slot) { return RichTapeArgs{c->d_tape + (size_t)slot * 2 * (size_t)rich_slot_elems(c), rich_slot_elems(c)}; }
inline RichSweepArgs rich_sweep_args(const trm_ctx* c, int slot, int fold) {
    return RichSweepArgs{c->d_adj[TRM_ADJOINT_INTERNAL_ENERGY], c->d_adj[TRM_ADJOINT_SATURATION], c->d_adj[TRM_ADJOINT_TEMPERATURE],
                         c->d_adj[TRM_ADJOINT_LIQUID_WATER_FRACTION], c->d_adj[TRM_ADJOINT_PRESSURE_HEAD], rich_tape_args(c, slot).tape, rich_slot_elems(c), fold};
}
template <class = void> int adjoint_record_rich(trm_ctx* c, double dt, int nsteps, int slot) {
    const std::string who = "k_column_record_rich";
    if (int rc = adjoint_rich_ok(c, nsteps, slot, who)) return rc;
    const LaunchArgs<double>& la = launch_args<double>(c);
    const ColumnArgs<double> a = column_args<double>(c, dt, 1, nsteps, PROG_MULTI);
    const RichTapeArgs aa = rich_tape_args(c, slot);
    return by_instance(c, [&](auto h, auto lpc) {
        constexpr int H = decltype(h)::value, LPC = decltype(lpc)::value;
        hipLaunchKernelGGL((k_column_record_rich<H, LPC>), column_grid(c, LPC), dim3(TRM_STEP_BLOCK), 0, c->stream, la.state, la.p, a, aa);
        TRM_HIP(c, hipGetLastError());
        c->last_program = derivative_program_id(TRM_PROGRAM_COLUMN_ADJOINT_RICHARDS, H, LPC, 0, 0);
        return (int)TRM_OK;
    });
}

// ---- the hydraulic-parameter gradients (TRM_OPT_DERIVATIVE_RICHARDS_PARAMS, trm_adjoint_param_open on such a context): the seven
// per-cell accumulators beside the sweep, and k_hyd_param_reduce, which ends it (trm_launch_column_adjoint_rich_param.hip)
inline HydParamPtrs hyd_param_ptrs(const trm_ctx* c) {
    HydParamPtrs g;
    for (int q = 0; q < HP_COUNT; ++q) g.g[q] = c->d_adj_hyd[q];
    return g;
}
static_assert(TRM_HYDRAULIC_PARAM_COUNT == HP_COUNT, "hyd_param_row (trm_host.hpp) counts the kernel's sums");
inline int hyd_params_ok(trm_ctx* c, const std::string& who) {
    if (!c->d_adj_hyd_out) return fail(c, TRM_EINVAL, who + ": no accumulators");
    return arrays_ok(c, c->d_adj_hyd, who, "accumulators");
}
template <class = void> int adjoint_rich_param_reduce(trm_ctx* c) {
    if (c->params.flow != TRM_FLOW_RICHARDS) return fail(c, TRM_EINVAL, "k_hyd_param_reduce: a Richards context only");
    if (int rc = hyd_params_ok(c, "k_hyd_param_reduce")) return rc;
    hipLaunchKernelGGL((k_hyd_param_reduce<HydParamPtrs>), dim3((unsigned)((c->Nh + 255) / 256)), dim3(256), 0, c->stream, hyd_param_ptrs(c), c->d_adj_hyd_out,
                       (long long)c->Nh, c->Nz, c->Nzp);
    TRM_HIP(c, hipGetLastError());
    return TRM_OK;
}

// ---- the backward sweep: the four wrappers of adjoint_rich_program (trm_column_adjoint_rich.hpp).  PARAMS: with the hydraulic-parameter
// gradients (k_column_adjoint_rich_params); RECORD: reading the attached soil-moisture record (k_column_adjoint_rich_record,
// k_column_adjoint_rich_params_record; TRM_OPT_DERIVATIVE_RICHARDS_RECORD) -- on the per-step tape the taped position of the launch's
// first step is its slot.  One explicit instantiation in each of trm_launch_column_adjoint_rich{,_param,_record,_param_record}.hip.
// The preconditions: the sweep's, the accumulators and their result, record_launch_ok.  TRM_INFO_LAST_PROGRAM knows of no record
template <bool PARAMS, bool RECORD> int adjoint_backward_rich(trm_ctx* c, double dt, int nsteps, int slot, int fold) {
    const std::string who = std::string(RECORD ? "k_column_adjoint_rich_record" : "k_column_adjoint_rich") + (PARAMS ? " (parameter gradients)" : "");
    if (int rc = adjoint_rich_ok(c, nsteps, slot, who)) return rc;
    if constexpr (PARAMS)
        if (int rc = hyd_params_ok(c, who)) return rc;
    if constexpr (RECORD)
        if (int rc = record_launch_ok(c, nsteps, slot, who)) return rc;
    const LaunchArgs<double>& la = launch_args<double>(c);
    const ColumnArgs<double> a = column_args<double>(c, dt, 1, nsteps, PROG_MULTI);
    const RichSweepArgs aa = rich_sweep_args(c, slot, fold);
    const HydParamPtrs hp = PARAMS ? hyd_param_ptrs(c) : HydParamPtrs{};
    const RecordArgs r = RECORD ? record_args(c, slot) : RecordArgs{};
    return by_instance(c, [&](auto h, auto lpc) {
        constexpr int H = decltype(h)::value, LPC = decltype(lpc)::value;
        const dim3 grid = column_grid(c, LPC), block(TRM_STEP_BLOCK);
        if constexpr (PARAMS && RECORD) hipLaunchKernelGGL((k_column_adjoint_rich_params_record<H, LPC>), grid, block, 0, c->stream, la.state, la.p, a, aa, hp, r);
        else if constexpr (PARAMS) hipLaunchKernelGGL((k_column_adjoint_rich_params<H, LPC>), grid, block, 0, c->stream, la.state, la.p, a, aa, hp);
        else if constexpr (RECORD) hipLaunchKernelGGL((k_column_adjoint_rich_record<H, LPC>), grid, block, 0, c->stream, la.state, la.p, a, aa, r);
        else hipLaunchKernelGGL((k_column_adjoint_rich<H, LPC>), grid, block, 0, c->stream, la.state, la.p, a, aa);
        TRM_HIP(c, hipGetLastError());
        c->last_program = derivative_program_id(TRM_PROGRAM_COLUMN_ADJOINT_RICHARDS, H, LPC, 0, PARAMS ? (int)TRM_PROGRAM_PARAMETERS : 0);
        return (int)TRM_OK;
    });
}

// k_column_record on the per-step tape (`slot`: of the launch's first step) or STRIDED on the checkpointed one (the stores before the
// steps first, first + every, ... go into the slots from `slot` on); SERIES: with the boundary series evaluated in the launch
template <bool STRIDED, bool SERIES> int adjoint_record(trm_ctx* c, double dt, int nsteps, int slot, int first, int every) {
    const std::string who = std::string(STRIDED ? "k_column_record (strided)" : "k_column_record") + (SERIES ? " (series)" : "");
    if (int rc = STRIDED ? strided_stores_ok(c, nsteps, slot, first, every, who) : tape_range_ok(c, nsteps, slot, who)) return rc;
    if constexpr (SERIES)
        if (int rc = series_rows_ok(c, nsteps, who)) return rc;
    const LaunchArgs<double>& la = launch_args<double>(c);
    const ColumnArgs<double> a = column_args<double>(c, dt, 1, nsteps, PROG_EULER);
    TapeArgs<STRIDED> aa;
    fill_cotangent(c, aa, slot, 0, SERIES);
    if constexpr (STRIDED) {
        aa.first = first;
        aa.every = every;
    }
    return by_instance(c, [&](auto h, auto lpc) {
        constexpr int H = decltype(h)::value, LPC = decltype(lpc)::value;
        hipLaunchKernelGGL((k_column_record<H, LPC, STRIDED, SERIES>), column_grid(c, LPC), dim3(TRM_STEP_BLOCK), 0, c->stream, la.state, la.p, a, aa);
        TRM_HIP(c, hipGetLastError());
        c->last_program = derivative_program_id(TRM_PROGRAM_COLUMN_ADJOINT, H, LPC, aa.generic, STRIDED ? PROGRAM_CHECKPOINTED : 0);
        return (int)TRM_OK;
    });
}

// the backward launch of a block of the per-step tape (k_column_adjoint) or, CKPT, of one segment of the checkpointed tape
// (k_column_adjoint_ckpt: the segment's states in dynamic LDS, 2 KiB per step and workgroup); RECORD: their twins that read the attached
// temperature record, `first` the taped position of the launch's first step
template <bool CKPT, Ride R, bool RECORD> int adjoint_backward(trm_ctx* c, double dt, int nsteps, int slot, int fold, int first) {
    const std::string who = ride_name(CKPT ? (RECORD ? "k_column_adjoint_ckpt_record" : "k_column_adjoint_ckpt") : (RECORD ? "k_column_adjoint_record" : "k_column_adjoint"), R, false);
    if (int rc = CKPT ? segment_range_ok(c, nsteps, slot, who) : tape_range_ok(c, nsteps, slot, who)) return rc;
    if (int rc = gradients_ok<R>(c, nsteps, who)) return rc;
    if constexpr (RECORD)
        if (int rc = record_launch_ok(c, nsteps, first, who)) return rc;
    const LaunchArgs<double>& la = launch_args<double>(c);
    const ColumnArgs<double> a = column_args<double>(c, dt, 1, nsteps, PROG_EULER);
    SweepArgs<CKPT, R> aa;
    fill_cotangent(c, aa, slot, fold, ride_has_series(R));
    fill_gradients(c, aa);
    if constexpr (CKPT) {
        aa.first = 0;
        aa.every = 1;
    }
    const RecordArgs r = RECORD ? record_args(c, first) : RecordArgs{};
    const int bits = PROGRAM_BACKWARD | (CKPT ? PROGRAM_CHECKPOINTED : 0) | (ride_has_bc(R) ? PROGRAM_BC_GRADIENT : 0) | (ride_has_params(R) ? (int)TRM_PROGRAM_PARAMETERS : 0);
    const size_t lds = CKPT ? (size_t)nsteps * TRM_STEP_BLOCK * sizeof(double) : 0;
    return by_instance(c, [&](auto h, auto lpc) {
        constexpr int H = decltype(h)::value, LPC = decltype(lpc)::value;
        const dim3 grid = column_grid(c, LPC), block(TRM_STEP_BLOCK);
        if constexpr (CKPT && RECORD) hipLaunchKernelGGL((k_column_adjoint_ckpt_record<H, LPC, R>), grid, block, lds, c->stream, la.state, la.p, a, aa, r);
        else if constexpr (CKPT) hipLaunchKernelGGL((k_column_adjoint_ckpt<H, LPC, R>), grid, block, lds, c->stream, la.state, la.p, a, aa);
        else if constexpr (RECORD) hipLaunchKernelGGL((k_column_adjoint_record<H, LPC, R>), grid, block, lds, c->stream, la.state, la.p, a, aa, r);
        else hipLaunchKernelGGL((k_column_adjoint<H, LPC, R>), grid, block, lds, c->stream, la.state, la.p, a, aa);
        TRM_HIP(c, hipGetLastError());
        c->last_program = derivative_program_id(TRM_PROGRAM_COLUMN_ADJOINT, H, LPC, aa.generic, bits);
        return (int)TRM_OK;
    });
}

}  // namespace trmh
