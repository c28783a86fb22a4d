// trm_launch_column_adjoint_ckpt_series.hip -- the launches of k_column_adjoint_ckpt<HYD, LPC, true, CheckpointSeriesArgs, false, true>
// (both lanes-per-column layouts; trm_column_adjoint_ckpt.hpp, trm_series_derivative.hpp): the backward sweep of the checkpointed tape
// with boundary time series evaluated in the launch and the gradients delivered per node of the series.
#include "trm_host.hpp"
// (this translation unit's copy of the non-template kernel of trm_column_tangent.hpp gets a name of its own)
#define k_closure_tangent k_closure_tangent_in_adjoint_ckpt_series_unit
#include "trm_column_tangent.hpp"
#undef k_closure_tangent
#include "trm_column_adjoint_ckpt.hpp"

namespace trmh {

int series_launch_ok(trm_ctx* c, int nsteps, const char* who);      // (trm_launch_column_adjoint_series.hip)
int series_accumulators_ok(trm_ctx* c, const char* who);

namespace {
template <int H, int LPC> int launch_checkpoint_series(trm_ctx* c, double dt, int nsteps, int slot, int fold) {
    const LaunchArgs<double>& la = launch_args<double>(c);
    const ColumnArgs<double> a = column_args<double>(c, dt, 1, nsteps, PROG_EULER);
    CheckpointSeriesArgs ca;
    ca.lU = c->d_adj[TRM_ADJOINT_INTERNAL_ENERGY];
    ca.lT = c->d_adj[TRM_ADJOINT_TEMPERATURE];
    ca.lliq = c->d_adj[TRM_ADJOINT_LIQUID_WATER_FRACTION];
    ca.slot_elems = (long long)c->Nh * (long long)c->Nzp;
    ca.tape = c->d_tape + (size_t)slot * (size_t)ca.slot_elems;
    ca.generic = 0;
    ca.fold = fold;
    ca.first = 0;
    ca.every = 1;
    ca.g = BcGradPtrs{c->d_adj_bc[0], c->d_adj_bc[1], c->d_adj_bc[2], c->d_adj_bc[3]};
    ca.sg = SeriesGradPtrs{{c->d_adj_bcs[0], c->d_adj_bcs[1], c->d_adj_bcs[2], c->d_adj_bcs[3]}};
    // the segment's states in dynamic LDS: 2 KiB per step and workgroup, as the launch without series
    const size_t lds = (size_t)nsteps * TRM_STEP_BLOCK * sizeof(double);
    hipLaunchKernelGGL((k_column_adjoint_ckpt<H, LPC, true, CheckpointSeriesArgs, false, true>), column_grid(c, LPC), dim3(TRM_STEP_BLOCK), lds, c->stream, la.state, la.p, a, ca);
    TRM_HIP(c, hipGetLastError());
    c->last_program = program_id(TRM_PROGRAM_COLUMN_ADJOINT, H, LPC, DERIVE_NONE, 0, 0, -1) | 1 << 26 | 1 << 27 | 1 << 30;
    return TRM_OK;
}
}  // namespace

int CheckpointLaunch::backward_series(trm_ctx* c, double dt, int nsteps, int slot, int fold) {
    if (slot < 0 || nsteps < 0 || nsteps > TRM_ADJOINT_MAX_INTERVAL || slot >= c->tape_cap)
        return fail(c, TRM_EINVAL, "k_column_adjoint_ckpt (series): the launch leaves the tape");
    if (int rc = series_launch_ok(c, nsteps, "k_column_adjoint_ckpt")) return rc;
    if (int rc = series_accumulators_ok(c, "k_column_adjoint_ckpt")) return rc;
    int rc = TRM_OK;
    using NF = double;
    const bool deep = c->Nz > 32;
    TRM_BY_HYD(c, rc = deep ? (launch_checkpoint_series<H, 64>(c, dt, nsteps, slot, fold)) : (launch_checkpoint_series<H, 32>(c, dt, nsteps, slot, fold)));
    return rc;
}

}  // namespace trmh
