// trm_launch_column_tangent_series.hip -- the launches of k_column_tangent<HYD, LPC, true, TangentSeriesArgs, false, true> (both
// lanes-per-column layouts; trm_column_tangent.hpp, trm_series_derivative.hpp): the forward-mode tangents with boundary time series
// evaluated in the launch and seeds shaped like the series (TRM_OPT_DERIVATIVE_SERIES, trm_tangent_bc_series_upload).
#include "trm_host.hpp"
// (this translation unit's copy of the non-template kernel of trm_column_tangent.hpp gets a name of its own, as in trm_column_adjoint.hpp)
#define k_closure_tangent k_closure_tangent_in_tangent_series_unit
#include "trm_column_tangent.hpp"
#undef k_closure_tangent

namespace trmh {

namespace {
template <int H, int LPC> int launch_tangent_series(trm_ctx* c, double dt, int nsteps) {
    const LaunchArgs<double>& la = launch_args<double>(c);
    const ColumnArgs<double> a = column_args<double>(c, dt, 1, nsteps, PROG_EULER);
    TangentSeriesArgs ta;
    ta.dU = c->d_tan[TRM_TANGENT_INTERNAL_ENERGY];
    ta.dT = c->d_tan[TRM_TANGENT_TEMPERATURE];
    ta.dliq = c->d_tan[TRM_TANGENT_LIQUID_WATER_FRACTION];
    ta.generic = 0;
    ta.sTb = c->d_tan_bc[0];
    ta.sTt = c->d_tan_bc[1];
    ta.sUb = c->d_tan_bc[2];
    ta.sUt = c->d_tan_bc[3];
    for (int s = 0; s < 4; ++s) ta.sn[s] = c->d_tan_bcs[s];
    hipLaunchKernelGGL((k_column_tangent<H, LPC, true, TangentSeriesArgs, false, true>), column_grid(c, LPC), dim3(TRM_STEP_BLOCK), 0, c->stream, la.state, la.p, a, ta);
    TRM_HIP(c, hipGetLastError());
    c->last_program = program_id(TRM_PROGRAM_COLUMN_TANGENT, H, LPC, DERIVE_NONE, 0, 0, -1) | 1 << 26;
    return TRM_OK;
}
}  // namespace

int TangentLaunch::step_series(trm_ctx* c, double dt, int nsteps) {
    for (const double* q : c->d_tan_bc)
        if (!q) return fail(c, TRM_EINVAL, "k_column_tangent (series): no seed arrays");
    if (!c->d_series_table || (nsteps > 0 && !c->d_series_rows) || Policy<double>::generic_bcs(c))
        return fail(c, TRM_EINVAL, "k_column_tangent (series): no series rows, or the generic boundary kinds");
    for (const auto& sr : c->series) {
        const int slot = Policy<double>::series_slot(c, sr);
        if (slot < SLOT_T_BOT || slot > SLOT_FU_TOP || !c->d_tan_bcs[slot] || c->tan_bcs_nt[slot] != sr.cap)
            return fail(c, TRM_EINVAL, "k_column_tangent (series): a series without seeds of its shape");
    }
    int rc = TRM_OK;
    using NF = double;
    const bool deep = c->Nz > 32;
    TRM_BY_HYD(c, rc = deep ? (launch_tangent_series<H, 64>(c, dt, nsteps)) : (launch_tangent_series<H, 32>(c, dt, nsteps)));
    return rc;
}

}  // namespace trmh
