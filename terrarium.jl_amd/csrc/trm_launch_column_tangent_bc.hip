// trm_launch_column_tangent_bc.hip -- the launches of k_column_tangent<HYD, LPC, true, TangentBcArgs> (both lanes-per-column layouts;
// trm_column_tangent.hpp): the forward-mode tangents with seeds on the boundary values (trm_tangent_bc_upload).
#include "trm_host.hpp"
// (this translation unit's copy of the non-template kernel of trm_column_tangent.hpp gets a name of its own, as in trm_column_adjoint.hpp)
#define k_closure_tangent k_closure_tangent_in_tangent_bc_unit
#include "trm_column_tangent.hpp"
#undef k_closure_tangent

namespace trmh {

namespace {
template <int H, int LPC> int launch_tangent_bc(trm_ctx* c, double dt, int nsteps) {
    const LaunchArgs<double>& la = launch_args<double>(c);
    const ColumnArgs<double> a = column_args<double>(c, dt, 1, nsteps, PROG_EULER);
    TangentBcArgs ta;
    ta.dU = c->d_tan[TRM_TANGENT_INTERNAL_ENERGY];
    ta.dT = c->d_tan[TRM_TANGENT_TEMPERATURE];
    ta.dliq = c->d_tan[TRM_TANGENT_LIQUID_WATER_FRACTION];
    ta.generic = Policy<double>::generic_bcs(c) ? 1 : 0;
    ta.sTb = c->d_tan_bc[0];
    ta.sTt = c->d_tan_bc[1];
    ta.sUb = c->d_tan_bc[2];
    ta.sUt = c->d_tan_bc[3];
    hipLaunchKernelGGL((k_column_tangent<H, LPC, true, TangentBcArgs>), column_grid(c, LPC), dim3(TRM_STEP_BLOCK), 0, c->stream, la.state, la.p, a, ta);
    TRM_HIP(c, hipGetLastError());
    c->last_program = program_id(TRM_PROGRAM_COLUMN_TANGENT, H, LPC, DERIVE_NONE, 0, 0, -1) | (ta.generic ? 1 << 25 : 0) | 1 << 26;
    return TRM_OK;
}
}  // namespace

int TangentLaunch::step_bc(trm_ctx* c, double dt, int nsteps) {
    for (const double* q : c->d_tan_bc)
        if (!q) return fail(c, TRM_EINVAL, "k_column_tangent (boundary seeds): no seed arrays");
    int rc = TRM_OK;
    using NF = double;
    const bool deep = c->Nz > 32;
    TRM_BY_HYD(c, rc = deep ? (launch_tangent_bc<H, 64>(c, dt, nsteps)) : (launch_tangent_bc<H, 32>(c, dt, nsteps)));
    return rc;
}

}  // namespace trmh
