// trm_launch_column_accum.inl -- the launch of k_column_accum<NF, RICH, ...> (trm_column.hpp): the resident multi-step program with
// time averages accumulated in the launch.  Included by the trm_launch_column_accum_*.hip files, each of which instantiates its
// share of ColumnAccumLaunch<NF, RICH>.
#include "trm_host.hpp"

namespace trmh {

template <class NF, bool RICH, int H, int LPC> static int launch_column_accum(trm_ctx* c, double dt, int finalize, int nsteps, const AccumArgs& acc) {
    const View<NF>& v = state_view<NF>(c);
    const DevParams<NF>& p = launch_args<NF>(c).p;
    const ColumnArgs<NF> a = column_args<NF>(c, dt, finalize, nsteps, PROG_MULTI);
    const dim3 grid = column_grid(c, LPC), block(TRM_STEP_BLOCK);
    const bool series = !c->series.empty();
    // (the same instance choice as the PROG_MULTI launch of trm_launch_column.inl, and the same TRM_INFO_LAST_PROGRAM + the bit of
    // the accumulation in the launch)
    const int pid = program_id(TRM_PROGRAM_COLUMN_MULTI, H, LPC, DERIVE_NONE, 0, 1, -1) | (c->params.seb ? 1 << 25 : 0) | (series ? 1 << 26 : 0) |
                    TRM_PROGRAM_BIT_AVERAGES_IN_LAUNCH;
    if (c->params.seb && series) hipLaunchKernelGGL((k_column_accum<NF, RICH, H, LPC, true, true>), grid, block, 0, c->stream, v, p, a, acc);
    else if (c->params.seb) hipLaunchKernelGGL((k_column_accum<NF, RICH, H, LPC, true, false>), grid, block, 0, c->stream, v, p, a, acc);
    else if (series) hipLaunchKernelGGL((k_column_accum<NF, RICH, H, LPC, false, true>), grid, block, 0, c->stream, v, p, a, acc);
    else hipLaunchKernelGGL((k_column_accum<NF, RICH, H, LPC, false, false>), grid, block, 0, c->stream, v, p, a, acc);
    TRM_HIP(c, hipGetLastError());
    c->last_program = pid;
    return TRM_OK;
}

template <class NF, bool RICH> int ColumnAccumLaunch<NF, RICH>::run(trm_ctx* c, double dt, int finalize, int nsteps, const AccumArgs& acc) {
    int rc = TRM_OK;
    const bool deep = c->Nz > 32;
    TRM_BY_HYD(c, rc = deep ? (launch_column_accum<NF, RICH, H, 64>(c, dt, finalize, nsteps, acc)) : (launch_column_accum<NF, RICH, H, 32>(c, dt, finalize, nsteps, acc)));
    return rc;
}

}  // namespace trmh
