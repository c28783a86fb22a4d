// trm_launch_column_adjoint_param.hip -- the launches of k_column_adjoint<HYD, LPC, true, AdjointParamArgs, true> (both lanes-per-column
// layouts) and k_param_reduce (trm_column_adjoint.hpp): the backward sweep of the per-step tape with the boundary and the thermal
// parameter gradients riding along (trm_adjoint_param_open), and the reduction that ends a sweep on either tape.
#include "trm_host.hpp"
// (this translation unit's copy of the non-template kernel of trm_column_tangent.hpp gets a name of its own)
#define k_closure_tangent k_closure_tangent_in_adjoint_param_unit
#include "trm_column_tangent.hpp"
#undef k_closure_tangent
#include "trm_column_adjoint.hpp"

namespace trmh {

namespace {
template <int H, int LPC> int launch_adjoint_param(trm_ctx* c, double dt, int nsteps, int slot, int fold) {
    const LaunchArgs<double>& la = launch_args<double>(c);
    const ColumnArgs<double> a = column_args<double>(c, dt, 1, nsteps, PROG_EULER);
    AdjointParamArgs aa;
    aa.lU = c->d_adj[TRM_ADJOINT_INTERNAL_ENERGY];
    aa.lT = c->d_adj[TRM_ADJOINT_TEMPERATURE];
    aa.lliq = c->d_adj[TRM_ADJOINT_LIQUID_WATER_FRACTION];
    aa.slot_elems = (long long)c->Nh * (long long)c->Nzp;
    aa.tape = c->d_tape + (size_t)slot * (size_t)aa.slot_elems;
    aa.generic = Policy<double>::generic_bcs(c) ? 1 : 0;
    aa.fold = fold;
    aa.g = BcGradPtrs{c->d_adj_bc[0], c->d_adj_bc[1], c->d_adj_bc[2], c->d_adj_bc[3]};
    for (int q = 0; q < 8; ++q) aa.pg.g[q] = c->d_adj_param[q];
    hipLaunchKernelGGL((k_column_adjoint<H, LPC, true, AdjointParamArgs, true>), column_grid(c, LPC), dim3(TRM_STEP_BLOCK), 0, c->stream, la.state, la.p, a,
                       aa);
    TRM_HIP(c, hipGetLastError());
    c->last_program =
        program_id(TRM_PROGRAM_COLUMN_ADJOINT, H, LPC, DERIVE_NONE, 0, 0, -1) | (aa.generic ? 1 << 25 : 0) | 1 << 26 | 1 << 30 | TRM_PROGRAM_PARAMETERS;
    return TRM_OK;
}
}  // namespace

int AdjointLaunch::backward_param(trm_ctx* c, double dt, int nsteps, int slot, int fold) {
    if (slot < 0 || nsteps < 0 || slot + nsteps > c->tape_cap) return fail(c, TRM_EINVAL, "k_column_adjoint (parameter gradients): the launch leaves the tape");
    for (const double* q : c->d_adj_bc)
        if (!q) return fail(c, TRM_EINVAL, "k_column_adjoint (parameter gradients): no boundary accumulators");
    for (const double* q : c->d_adj_param)
        if (!q) return fail(c, TRM_EINVAL, "k_column_adjoint (parameter gradients): no accumulators");
    int rc = TRM_OK;
    using NF = double;
    const bool deep = c->Nz > 32;
    TRM_BY_HYD(c, rc = deep ? (launch_adjoint_param<H, 64>(c, dt, nsteps, slot, fold)) : (launch_adjoint_param<H, 32>(c, dt, nsteps, slot, fold)));
    return rc;
}

int AdjointLaunch::param_reduce(trm_ctx* c) {
    if (!c->d_adj_param_out) return fail(c, TRM_EINVAL, "k_param_reduce: no accumulators");
    ParamGradPtrs g;
    for (int q = 0; q < 8; ++q) {
        if (!c->d_adj_param[q]) return fail(c, TRM_EINVAL, "k_param_reduce: no accumulators");
        g.g[q] = c->d_adj_param[q];
    }
    ParamChain ch;
    thermal_param_chain(c->params, launch_args<double>(c).p, ch.w);
    hipLaunchKernelGGL((k_param_reduce<ParamGradPtrs>), dim3((unsigned)((c->Nh + 255) / 256)), dim3(256), 0, c->stream, g, ch, c->d_adj_param_out,
                       (long long)c->Nh, c->Nz, c->Nzp);
    TRM_HIP(c, hipGetLastError());
    return TRM_OK;
}

}  // namespace trmh
