// trm_launch_column_land.inl -- the launch of k_column_land (trm_column.hpp): ONE launch per ForwardEuler step of a bare-ground LandModel
// (fp64, Richards, the LandModel's boundary signature compiled in) with the 0-D surface processes in its first workgroups
// (TRM_OPT_SURFACE_IN_LAUNCH).  Included by trm_launch_column_land_{bc,vg}.hip, one hydraulics instance each.
#pragma once
#include "trm_host.hpp"

namespace trmh {

template <int H> int FrontLaunch::run_hyd(trm_ctx* c, const StepPlan& plan, double dt, int finalize, bool heun) {
    using NF = double;
    const LaunchArgs<NF>& la = launch_args<NF>(c);
    FrontArgs fa;
    if (int rc = front_args(c, "k_column_land", fa)) return rc;
    ColumnArgs<NF> a = column_args<NF>(c, dt, finalize, 1, heun ? PROG_HEUN : PROG_EULER);
    if (!heun) a.store_closure = plan.store_closure;      // (0: a deriving instance alone)
    if (!heun && plan.derive != DERIVE_NONE && plan.derive != DERIVE_T_LIQ) return fail(c, TRM_EINVAL, "k_column_land: no instance for this derivation mode");
    int rc = NO_INSTANCE;
    by_lanes(c->Nz, [&](auto LPC) {
        dim3 grid = column_grid(c, LPC());
        grid.x += (unsigned)fa.chain_blocks;
        const dim3 block(TRM_STEP_BLOCK);
        // the one-launch Heun program, and ForwardEuler without the derivation: T / liq read as stored, direct stores, scalar inputs
        if (heun) rc = run_column_land<H, LPC(), DERIVE_NONE, false, true, PROG_HEUN>(c, grid, block, la.state, la.p, a, fa);
        else if (plan.derive == DERIVE_NONE) rc = run_column_land<H, LPC(), DERIVE_NONE, false, true, PROG_EULER>(c, grid, block, la.state, la.p, a, fa);
        else by_io(plan.staged, plan.scalar_in, [&](auto ST, auto SC) { rc = run_column_land<H, LPC(), DERIVE_T_LIQ, ST(), SC(), PROG_EULER>(c, grid, block, la.state, la.p, a, fa); });
    });
    return launched(c, rc, "k_column_land: no instance for this (staged, scalar_in) pair");
}

}  // namespace trmh
