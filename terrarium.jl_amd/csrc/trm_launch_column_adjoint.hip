// trm_launch_column_adjoint.hip -- the launches of k_column_record<HYD, LPC> and k_column_adjoint<HYD, LPC> (both lanes-per-column
// layouts; trm_column_adjoint.hpp): reverse-mode gradients of the heat-only fp64 SoilModel run.
#include "trm_host.hpp"
#include "trm_column_adjoint.hpp"

namespace trmh {

namespace {
// `slot`: the tape slot of the first step of the launch
AdjointArgs adjoint_args(const trm_ctx* c, int slot, int fold) {
    AdjointArgs aa;
    aa.lU = c->d_adj[TRM_ADJOINT_INTERNAL_ENERGY];
    aa.lT = c->d_adj[TRM_ADJOINT_TEMPERATURE];
    aa.lliq = c->d_adj[TRM_ADJOINT_LIQUID_WATER_FRACTION];
    aa.slot_elems = (long long)c->Nh * (long long)c->Nzp;
    aa.tape = c->d_tape + (size_t)slot * (size_t)aa.slot_elems;
    aa.generic = Policy<double>::generic_bcs(c) ? 1 : 0;
    aa.fold = fold;
    return aa;
}

template <int H, int LPC, bool BACKWARD> int launch_adjoint(trm_ctx* c, double dt, int nsteps, int slot, int fold) {
    const LaunchArgs<double>& la = launch_args<double>(c);
    const ColumnArgs<double> a = column_args<double>(c, dt, 1, nsteps, PROG_EULER);
    const AdjointArgs aa = adjoint_args(c, slot, fold);
    if (BACKWARD) hipLaunchKernelGGL((k_column_adjoint<H, LPC>), column_grid(c, LPC), dim3(TRM_STEP_BLOCK), 0, c->stream, la.state, la.p, a, aa);
    else hipLaunchKernelGGL((k_column_record<H, LPC>), column_grid(c, LPC), dim3(TRM_STEP_BLOCK), 0, c->stream, la.state, la.p, a, aa);
    TRM_HIP(c, hipGetLastError());
    c->last_program = program_id(TRM_PROGRAM_COLUMN_ADJOINT, H, LPC, DERIVE_NONE, 0, 0, -1) | (aa.generic ? 1 << 25 : 0) | (BACKWARD ? 1 << 26 : 0);
    return TRM_OK;
}
}  // namespace

int AdjointLaunch::record(trm_ctx* c, double dt, int nsteps, int slot) {
    if (slot < 0 || nsteps < 0 || slot + nsteps > c->tape_cap) return fail(c, TRM_EINVAL, "k_column_record: the launch leaves the tape");
    int rc = TRM_OK;
    using NF = double;
    const bool deep = c->Nz > 32;
    TRM_BY_HYD(c, rc = deep ? (launch_adjoint<H, 64, false>(c, dt, nsteps, slot, 0)) : (launch_adjoint<H, 32, false>(c, dt, nsteps, slot, 0)));
    return rc;
}

int AdjointLaunch::backward(trm_ctx* c, double dt, int nsteps, int slot, int fold) {
    if (slot < 0 || nsteps < 0 || slot + nsteps > c->tape_cap) return fail(c, TRM_EINVAL, "k_column_adjoint: the launch leaves the tape");
    int rc = TRM_OK;
    using NF = double;
    const bool deep = c->Nz > 32;
    TRM_BY_HYD(c, rc = deep ? (launch_adjoint<H, 64, true>(c, dt, nsteps, slot, fold)) : (launch_adjoint<H, 32, true>(c, dt, nsteps, slot, fold)));
    return rc;
}

}  // namespace trmh
