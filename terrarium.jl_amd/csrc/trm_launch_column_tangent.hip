// trm_launch_column_tangent.hip -- the launches of k_column_tangent<HYD, LPC> (both lanes-per-column layouts) and k_closure_tangent
// (trm_column_tangent.hpp): forward-mode tangents of the heat-only fp64 SoilModel step.
#include "trm_host.hpp"
#include "trm_column_tangent.hpp"

namespace trmh {

namespace {
TangentArgs tangent_args(const trm_ctx* c) {
    TangentArgs ta;
    ta.dU = c->d_tan[TRM_TANGENT_INTERNAL_ENERGY];
    ta.dT = c->d_tan[TRM_TANGENT_TEMPERATURE];
    ta.dliq = c->d_tan[TRM_TANGENT_LIQUID_WATER_FRACTION];
    ta.generic = Policy<double>::generic_bcs(c) ? 1 : 0;
    return ta;
}

template <int H, int LPC> int launch_tangent(trm_ctx* c, double dt, int nsteps) {
    const LaunchArgs<double>& la = launch_args<double>(c);
    const ColumnArgs<double> a = column_args<double>(c, dt, 1, nsteps, PROG_EULER);
    const TangentArgs ta = tangent_args(c);
    hipLaunchKernelGGL((k_column_tangent<H, LPC>), column_grid(c, LPC), dim3(TRM_STEP_BLOCK), 0, c->stream, la.state, la.p, a, ta);
    TRM_HIP(c, hipGetLastError());
    c->last_program = program_id(TRM_PROGRAM_COLUMN_TANGENT, H, LPC, DERIVE_NONE, 0, 0, -1) | (ta.generic ? 1 << 25 : 0);
    return TRM_OK;
}
}  // namespace

int TangentLaunch::step(trm_ctx* c, double dt, int nsteps) {
    int rc = TRM_OK;
    using NF = double;
    const bool deep = c->Nz > 32;
    TRM_BY_HYD(c, rc = deep ? (launch_tangent<H, 64>(c, dt, nsteps)) : (launch_tangent<H, 32>(c, dt, nsteps)));
    return rc;
}

int TangentLaunch::closure(trm_ctx* c) {
    const LaunchArgs<double>& la = launch_args<double>(c);
    const size_t cells = (size_t)c->Nh * (size_t)c->Nzp;
    hipLaunchKernelGGL(k_closure_tangent, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, c->stream, la.state, la.p, tangent_args(c));
    TRM_HIP(c, hipGetLastError());
    return TRM_OK;
}

}  // namespace trmh
