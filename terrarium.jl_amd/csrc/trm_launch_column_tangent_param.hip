// trm_launch_column_tangent_param.hip -- the launches of k_column_tangent<HYD, LPC, true, TangentParamArgs, true> (both lanes-per-column
// layouts) and k_closure_tangent_param (trm_column_tangent.hpp): the forward-mode tangents with seeds on the thermal parameters
// (trm_tangent_param_set); the boundary seeds ride along, zero unless trm_tangent_bc_upload has set them.
#include "trm_host.hpp"
// (this translation unit's copy of the non-template kernel of trm_column_tangent.hpp gets a name of its own, as in trm_column_adjoint.hpp)
#define k_closure_tangent k_closure_tangent_in_tangent_param_unit
#include "trm_column_tangent.hpp"
#undef k_closure_tangent

namespace trmh {

namespace {
TangentParamArgs tangent_param_args(const trm_ctx* c) {
    TangentParamArgs ta;
    ta.dU = c->d_tan[TRM_TANGENT_INTERNAL_ENERGY];
    ta.dT = c->d_tan[TRM_TANGENT_TEMPERATURE];
    ta.dliq = c->d_tan[TRM_TANGENT_LIQUID_WATER_FRACTION];
    ta.generic = Policy<double>::generic_bcs(c) ? 1 : 0;
    ta.sTb = c->d_tan_bc[0];
    ta.sTt = c->d_tan_bc[1];
    ta.sUb = c->d_tan_bc[2];
    ta.sUt = c->d_tan_bc[3];
    const double* s = c->tan_param;
    ta.s = ParamSeeds{s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7]};
    return ta;
}

template <int H, int LPC> int launch_tangent_param(trm_ctx* c, double dt, int nsteps) {
    const LaunchArgs<double>& la = launch_args<double>(c);
    const ColumnArgs<double> a = column_args<double>(c, dt, 1, nsteps, PROG_EULER);
    const TangentParamArgs ta = tangent_param_args(c);
    hipLaunchKernelGGL((k_column_tangent<H, LPC, true, TangentParamArgs, true>), column_grid(c, LPC), dim3(TRM_STEP_BLOCK), 0, c->stream, la.state, la.p, a,
                       ta);
    TRM_HIP(c, hipGetLastError());
    c->last_program = program_id(TRM_PROGRAM_COLUMN_TANGENT, H, LPC, DERIVE_NONE, 0, 0, -1) | (ta.generic ? 1 << 25 : 0) | 1 << 26 | TRM_PROGRAM_PARAMETERS;
    return TRM_OK;
}
}  // namespace

int TangentLaunch::step_param(trm_ctx* c, double dt, int nsteps) {
    for (const double* q : c->d_tan_bc)
        if (!q) return fail(c, TRM_EINVAL, "k_column_tangent (parameter seeds): no boundary seed arrays");
    int rc = TRM_OK;
    using NF = double;
    const bool deep = c->Nz > 32;
    TRM_BY_HYD(c, rc = deep ? (launch_tangent_param<H, 64>(c, dt, nsteps)) : (launch_tangent_param<H, 32>(c, dt, nsteps)));
    return rc;
}

int TangentLaunch::closure_param(trm_ctx* c) {
    const LaunchArgs<double>& la = launch_args<double>(c);
    const size_t cells = (size_t)c->Nh * (size_t)c->Nzp;
    hipLaunchKernelGGL((k_closure_tangent_param<TangentParamArgs>), dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, c->stream, la.state, la.p,
                       tangent_param_args(c));
    TRM_HIP(c, hipGetLastError());
    return TRM_OK;
}

}  // namespace trmh
