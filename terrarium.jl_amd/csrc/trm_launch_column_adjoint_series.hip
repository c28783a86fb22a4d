// trm_launch_column_adjoint_series.hip -- the launches of k_column_record<HYD, LPC, STRIDED, .., true> (both tapes) and
// k_column_adjoint<HYD, LPC, true, AdjointSeriesArgs, false, true> (both lanes-per-column layouts; trm_column_adjoint.hpp,
// trm_series_derivative.hpp): the record and the backward sweep of the per-step tape with boundary time series evaluated in the launch
// and the gradients delivered per node of the series (TRM_OPT_DERIVATIVE_SERIES, trm_adjoint_bc_series_download).
#include "trm_host.hpp"
// (this translation unit's copy of the non-template kernel of trm_column_tangent.hpp gets a name of its own)
#define k_closure_tangent k_closure_tangent_in_adjoint_series_unit
#include "trm_column_tangent.hpp"
#undef k_closure_tangent
#include "trm_column_adjoint_ckpt.hpp"

namespace trmh {

namespace {
template <int H, int LPC> int launch_record_series(trm_ctx* c, double dt, int nsteps, int slot) {
    const LaunchArgs<double>& la = launch_args<double>(c);
    const ColumnArgs<double> a = column_args<double>(c, dt, 1, nsteps, PROG_EULER);
    AdjointArgs aa;
    aa.lU = c->d_adj[TRM_ADJOINT_INTERNAL_ENERGY];
    aa.lT = c->d_adj[TRM_ADJOINT_TEMPERATURE];
    aa.lliq = c->d_adj[TRM_ADJOINT_LIQUID_WATER_FRACTION];
    aa.slot_elems = (long long)c->Nh * (long long)c->Nzp;
    aa.tape = c->d_tape + (size_t)slot * (size_t)aa.slot_elems;
    aa.generic = 0;
    aa.fold = 0;
    hipLaunchKernelGGL((k_column_record<H, LPC, false, AdjointArgs, true>), column_grid(c, LPC), dim3(TRM_STEP_BLOCK), 0, c->stream, la.state, la.p, a, aa);
    TRM_HIP(c, hipGetLastError());
    c->last_program = program_id(TRM_PROGRAM_COLUMN_ADJOINT, H, LPC, DERIVE_NONE, 0, 0, -1);
    return TRM_OK;
}
template <int H, int LPC> int launch_record_strided_series(trm_ctx* c, double dt, int nsteps, int slot, int first, int every) {
    const LaunchArgs<double>& la = launch_args<double>(c);
    const ColumnArgs<double> a = column_args<double>(c, dt, 1, nsteps, PROG_EULER);
    CheckpointArgs ca;
    ca.lU = c->d_adj[TRM_ADJOINT_INTERNAL_ENERGY];
    ca.lT = c->d_adj[TRM_ADJOINT_TEMPERATURE];
    ca.lliq = c->d_adj[TRM_ADJOINT_LIQUID_WATER_FRACTION];
    ca.slot_elems = (long long)c->Nh * (long long)c->Nzp;
    ca.tape = c->d_tape + (size_t)slot * (size_t)ca.slot_elems;
    ca.generic = 0;
    ca.fold = 0;
    ca.first = first;
    ca.every = every;
    hipLaunchKernelGGL((k_column_record<H, LPC, true, CheckpointArgs, true>), column_grid(c, LPC), dim3(TRM_STEP_BLOCK), 0, c->stream, la.state, la.p, a, ca);
    TRM_HIP(c, hipGetLastError());
    c->last_program = program_id(TRM_PROGRAM_COLUMN_ADJOINT, H, LPC, DERIVE_NONE, 0, 0, -1) | 1 << 27;
    return TRM_OK;
}
template <int H, int LPC> int launch_adjoint_series(trm_ctx* c, double dt, int nsteps, int slot, int fold) {
    const LaunchArgs<double>& la = launch_args<double>(c);
    const ColumnArgs<double> a = column_args<double>(c, dt, 1, nsteps, PROG_EULER);
    AdjointSeriesArgs aa;
    aa.lU = c->d_adj[TRM_ADJOINT_INTERNAL_ENERGY];
    aa.lT = c->d_adj[TRM_ADJOINT_TEMPERATURE];
    aa.lliq = c->d_adj[TRM_ADJOINT_LIQUID_WATER_FRACTION];
    aa.slot_elems = (long long)c->Nh * (long long)c->Nzp;
    aa.tape = c->d_tape + (size_t)slot * (size_t)aa.slot_elems;
    aa.generic = 0;
    aa.fold = fold;
    aa.g = BcGradPtrs{c->d_adj_bc[0], c->d_adj_bc[1], c->d_adj_bc[2], c->d_adj_bc[3]};
    aa.sg = SeriesGradPtrs{{c->d_adj_bcs[0], c->d_adj_bcs[1], c->d_adj_bcs[2], c->d_adj_bcs[3]}};
    hipLaunchKernelGGL((k_column_adjoint<H, LPC, true, AdjointSeriesArgs, false, true>), column_grid(c, LPC), dim3(TRM_STEP_BLOCK), 0, c->stream, la.state, la.p, a, aa);
    TRM_HIP(c, hipGetLastError());
    c->last_program = program_id(TRM_PROGRAM_COLUMN_ADJOINT, H, LPC, DERIVE_NONE, 0, 0, -1) | 1 << 26 | 1 << 30;
    return TRM_OK;
}
}  // namespace

// what every series launch of the adjoint needs: the table, rows for its steps, the branch-free boundary kinds
int series_launch_ok(trm_ctx* c, int nsteps, const char* who) {
    if (!c->d_series_table || (nsteps > 0 && !c->d_series_rows) || Policy<double>::generic_bcs(c))
        return fail(c, TRM_EINVAL, std::string(who) + " (series): no series rows, or the generic boundary kinds");
    return TRM_OK;
}
// ... and a backward launch: the per-column accumulators and a node accumulator of its shape for every series
int series_accumulators_ok(trm_ctx* c, const char* who) {
    for (const double* q : c->d_adj_bc)
        if (!q) return fail(c, TRM_EINVAL, std::string(who) + " (series): no accumulators");
    for (const auto& sr : c->series) {
        const int slot = Policy<double>::series_slot(c, sr);
        if (slot < SLOT_T_BOT || slot > SLOT_FU_TOP || !c->d_adj_bcs[slot] || c->adj_bcs_nt[slot] != sr.cap)
            return fail(c, TRM_EINVAL, std::string(who) + " (series): a series without an accumulator of its shape");
    }
    return TRM_OK;
}

int AdjointLaunch::record_series(trm_ctx* c, double dt, int nsteps, int slot) {
    if (slot < 0 || nsteps < 0 || slot + nsteps > c->tape_cap) return fail(c, TRM_EINVAL, "k_column_record (series): the launch leaves the tape");
    if (int rc = series_launch_ok(c, nsteps, "k_column_record")) return rc;
    int rc = TRM_OK;
    using NF = double;
    const bool deep = c->Nz > 32;
    TRM_BY_HYD(c, rc = deep ? (launch_record_series<H, 64>(c, dt, nsteps, slot)) : (launch_record_series<H, 32>(c, dt, nsteps, slot)));
    return rc;
}

int CheckpointLaunch::record_series(trm_ctx* c, double dt, int nsteps, int slot, int first, int every) {
    if (slot < 0 || nsteps < 0 || first < 0 || every < 1) return fail(c, TRM_EINVAL, "k_column_record (strided, series): bad launch");
    const int stores = first < nsteps ? (nsteps - first + every - 1) / every : 0;
    if (slot + stores > c->tape_cap) return fail(c, TRM_EINVAL, "k_column_record (strided, series): the launch leaves the tape");
    if (stores == 0) slot = 0;     // (no store: any address inside the tape)
    if (int rc = series_launch_ok(c, nsteps, "k_column_record (strided)")) return rc;
    int rc = TRM_OK;
    using NF = double;
    const bool deep = c->Nz > 32;
    TRM_BY_HYD(c, rc = deep ? (launch_record_strided_series<H, 64>(c, dt, nsteps, slot, first, every))
                            : (launch_record_strided_series<H, 32>(c, dt, nsteps, slot, first, every)));
    return rc;
}

int AdjointLaunch::backward_series(trm_ctx* c, double dt, int nsteps, int slot, int fold) {
    if (slot < 0 || nsteps < 0 || slot + nsteps > c->tape_cap) return fail(c, TRM_EINVAL, "k_column_adjoint (series): the launch leaves the tape");
    if (int rc = series_launch_ok(c, nsteps, "k_column_adjoint")) return rc;
    if (int rc = series_accumulators_ok(c, "k_column_adjoint")) return rc;
    int rc = TRM_OK;
    using NF = double;
    const bool deep = c->Nz > 32;
    TRM_BY_HYD(c, rc = deep ? (launch_adjoint_series<H, 64>(c, dt, nsteps, slot, fold)) : (launch_adjoint_series<H, 32>(c, dt, nsteps, slot, fold)));
    return rc;
}

}  // namespace trmh
