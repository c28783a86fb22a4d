// trm_launch_column.inl -- the launch of k_column<NF, RICH, ., ., ., PROG, ...> (trm_column.hpp) for one (precision, flow scheme,
// program): included by the trm_launch_column_*.hip files, each of which instantiates its share of ColumnLaunch<NF, RICH, PROG>.
#pragma once
#include "trm_host.hpp"

namespace trmh {

template <class NF, bool RICH, int H, int LPC, int PROG> static int launch_column(trm_ctx* c, const StepPlan& plan, double dt, int finalize, int nsteps) {
    using P = Policy<NF>;
    constexpr bool F64 = std::is_same<NF, double>::value;
    const View<NF>& v = state_view<NF>(c);
    const DevParams<NF>& p = launch_args<NF>(c).p;
    ColumnArgs<NF> a = column_args<NF>(c, dt, finalize, nsteps, PROG);
    const dim3 grid = column_grid(c, LPC), block(TRM_STEP_BLOCK);
    const int derive = PROG == PROG_EULER ? plan.derive : P::template derive_now<RICH>(c);     // (ForwardEuler: the plan's instance; for this kernel DERIVE_NONE or DERIVE_T_LIQ)
    if (derive != DERIVE_NONE && derive != DERIVE_T_LIQ) return fail(c, TRM_EINVAL, "k_column: no instance for this derivation mode");
    int rc = TRM_OK;
    if constexpr (PROG == PROG_MULTI) {
        by_bool(c->params.seb != 0, [&](auto SEB) { by_bool(!c->series.empty(), [&](auto SERIES) {
            rc = run_column<NF, RICH, H, LPC, DERIVE_NONE, PROG_MULTI, SEB(), SERIES()>(c, grid, block, v, p, a);
        }); });
        return rc;
    } else if constexpr (PROG == PROG_EULER) {
        // the context's boundary kinds as a signature; the instantiated ones take the program with the kinds compiled in (fp64; with
        // the derivation of T / liq or without it); every instance below stores pressure_head / water_table as column_closure forms them, or is interior
        const int sig = plan.sig, staged = plan.staged, scalar_in = plan.scalar_in;
        a.store_closure = plan.store_closure;      // (0: a deriving instance alone)
        if (plan.psi_form != PSI_STORED) {
            // TRM_OPT_INTERIOR_STEPS: the instance that derives the pressure head at entry stands in for the signature instance this launch would otherwise be
            if constexpr (F64 && RICH && H != HYD_GENERIC) {
                a.check_entry = plan.check_entry;
                if (derive == DERIVE_T_LIQ && by_psi_signature(sig, [&](auto SIG) { rc = ColumnPsiLaunch<SIG()>::run(c, grid, block, v, p, a, plan.psi_form, staged, scalar_in); })) return rc;
            }
            return fail(c, TRM_EINVAL, "k_column_psi: no instance for this launch");
        }
        if constexpr (F64) {
            if (by_signature<RICH>(sig, [&](auto SIG) { rc = ColumnSigLaunch<NF, RICH, SIG()>::run(c, grid, block, v, p, a, derive, staged, scalar_in); })) return rc;
        }
        // the kinds read at run time.  Without the derivation: direct stores, scalar inputs
        if (derive == DERIVE_NONE) return run_column<NF, RICH, H, LPC, DERIVE_NONE, PROG_EULER>(c, grid, block, v, p, a);
        // with it (every large or HBM-resident fp64 state): how the per-column outputs leave / inputs arrive; fp32 off the packed kernel
        // derives only on request: one instance
        if constexpr (!F64) return run_column<NF, RICH, H, LPC, DERIVE_T_LIQ, PROG_EULER>(c, grid, block, v, p, a);
        else if (by_io(staged, scalar_in, [&](auto ST, auto SC) { rc = run_column<NF, RICH, H, LPC, DERIVE_T_LIQ, PROG_EULER, false, false, ST(), SC()>(c, grid, block, v, p, a); })) return rc;
        return fail(c, TRM_EINVAL, "k_column: no instance for this launch");
    } else {
        // (Heun: the same signatures)
        const int hsig = (c->opt_bc_signature && H != HYD_GENERIC) ? bc_signature_of(c) : -1;
        if constexpr (F64) {
            if (by_signature<RICH>(hsig, [&](auto SIG) { rc = ColumnSigHeunLaunch<NF, RICH, SIG()>::run(c, grid, block, v, p, a); })) return rc;
        }
        return run_column<NF, RICH, H, LPC, DERIVE_NONE, PROG_HEUN>(c, grid, block, v, p, a);
    }
}

template <class NF, bool RICH, int PROG> int ColumnLaunch<NF, RICH, PROG>::run(trm_ctx* c, const StepPlan& plan, double dt, int finalize, int nsteps) {
    int rc = TRM_OK;
    by_hyd(Policy<NF>::hyd(c), [&](auto H) { by_lanes(c->Nz, [&](auto LPC) { rc = launch_column<NF, RICH, H(), LPC(), PROG>(c, plan, dt, finalize, nsteps); }); });
    return rc;
}

}  // namespace trmh
