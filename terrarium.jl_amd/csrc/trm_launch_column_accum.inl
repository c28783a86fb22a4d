// trm_launch_column_accum.inl -- the launch of k_column_accum<NF, RICH, ...> (trm_column.hpp): the resident multi-step program with
// time averages accumulated in the launch.  Included by the trm_launch_column_accum_*.hip files, each of which instantiates its
// share of ColumnAccumLaunch<NF, RICH>.
#pragma once
#include "trm_host.hpp"

namespace trmh {

template <class NF, bool RICH> int ColumnAccumLaunch<NF, RICH>::run(trm_ctx* c, double dt, int finalize, int nsteps, const AccumArgs& acc) {
    const View<NF>& v = state_view<NF>(c);
    const DevParams<NF>& p = launch_args<NF>(c).p;
    const ColumnArgs<NF> a = column_args<NF>(c, dt, finalize, nsteps, PROG_MULTI);
    int rc = NO_INSTANCE;
    by_hyd(Policy<NF>::hyd(c), [&](auto H) { by_lanes(c->Nz, [&](auto LPC) {
        by_bool(c->params.seb != 0, [&](auto SEB) { by_bool(!c->series.empty(), [&](auto SERIES) {
            rc = run_column_accum<NF, RICH, H(), LPC(), SEB(), SERIES()>(c, column_grid(c, LPC()), dim3(TRM_STEP_BLOCK), v, p, a, acc);
        }); });
    }); });
    return launched(c, rc, "k_column_accum: no instance for this launch");
}

}  // namespace trmh
