// trm_launch_column.inl -- the launch of k_column<NF, RICH, ., ., ., PROG, ...> (trm_column.hpp) for one (precision, flow scheme,
// program): included by the trm_launch_column_*.hip files, each of which instantiates its share of ColumnLaunch<NF, RICH, PROG>.
#include "trm_host.hpp"

namespace trmh {

template <class NF, bool RICH, int H, int LPC, int PROG> static int launch_column(trm_ctx* c, const StepPlan& plan, double dt, int finalize, int nsteps) {
    using P = Policy<NF>;
    const View<NF>& v = state_view<NF>(c);
    const DevParams<NF>& p = launch_args<NF>(c).p;
    ColumnArgs<NF> a = column_args<NF>(c, dt, finalize, nsteps, PROG);
    const dim3 grid = column_grid(c, LPC), block(TRM_STEP_BLOCK);
    const int derive = PROG == PROG_EULER ? plan.derive : P::template derive_now<RICH>(c);     // (ForwardEuler: the plan's instance; for this kernel DERIVE_NONE or DERIVE_T_LIQ)
    if (PROG == PROG_EULER) a.store_closure = plan.store_closure;      // (0: a deriving instance alone)
    if (derive != DERIVE_NONE && derive != DERIVE_T_LIQ) return fail(c, TRM_EINVAL, "k_column: no instance for this derivation mode");
    int pid = 0;    // TRM_INFO_LAST_PROGRAM of the instance that is launched below
    if constexpr (PROG == PROG_MULTI) {
        const bool series = !c->series.empty();
        pid = program_id(TRM_PROGRAM_COLUMN_MULTI, H, LPC, DERIVE_NONE, 0, 1, -1) | (c->params.seb ? 1 << 25 : 0) | (series ? 1 << 26 : 0);
        if (c->params.seb && series) hipLaunchKernelGGL((k_column<NF, RICH, H, LPC, DERIVE_NONE, PROG_MULTI, true, true>), grid, block, 0, c->stream, v, p, a);
        else if (c->params.seb) hipLaunchKernelGGL((k_column<NF, RICH, H, LPC, DERIVE_NONE, PROG_MULTI, true, false>), grid, block, 0, c->stream, v, p, a);
        else if (series) hipLaunchKernelGGL((k_column<NF, RICH, H, LPC, DERIVE_NONE, PROG_MULTI, false, true>), grid, block, 0, c->stream, v, p, a);
        else hipLaunchKernelGGL((k_column<NF, RICH, H, LPC, DERIVE_NONE, PROG_MULTI, false, false>), grid, block, 0, c->stream, v, p, a);
    } else if constexpr (PROG == PROG_EULER) {
        // the context's boundary kinds as a signature; the instantiated ones take the program with the kinds compiled in (fp64; with
        // the derivation of T / liq or without it); every instance below stores pressure_head / water_table as column_closure forms them, or is interior
        const int sig = plan.sig, staged = plan.staged, scalar_in = plan.scalar_in;
        if (plan.psi_form != PSI_STORED) {
            // TRM_OPT_INTERIOR_STEPS: the instance that derives the pressure head at entry stands in for the signature instance this
            // launch would otherwise be, and reports that instance's id
            if constexpr (std::is_same<NF, double>::value && RICH && H != HYD_GENERIC) {
                if (derive != DERIVE_T_LIQ || !column_psi_supported(sig) || staged == scalar_in) return fail(c, TRM_EINVAL, "k_column_psi: no instance for this launch");
                a.check_entry = plan.check_entry;
                switch (sig) {
                    case 0: ColumnPsiLaunch<0>::run(c, v, p, a, grid, block, LPC, plan.psi_form, staged, scalar_in); break;
                    case BCSIG_T_TOP: ColumnPsiLaunch<BCSIG_T_TOP>::run(c, v, p, a, grid, block, LPC, plan.psi_form, staged, scalar_in); break;
                    case BCSIG_T_TOP | BCSIG_FU_BOT: ColumnPsiLaunch<BCSIG_T_TOP | BCSIG_FU_BOT>::run(c, v, p, a, grid, block, LPC, plan.psi_form, staged, scalar_in); break;
                    default: ColumnPsiLaunch<BCSIG_T_TOP | BCSIG_FS_TOP>::run(c, v, p, a, grid, block, LPC, plan.psi_form, staged, scalar_in); break;
                }
                pid = program_id(TRM_PROGRAM_COLUMN_EULER, H, LPC, DERIVE_T_LIQ, staged, scalar_in, sig);
            } else return fail(c, TRM_EINVAL, "k_column_psi: no instance for this launch");
        }
        else if (launch_by_signature<ColumnSigLaunch, NF, RICH>(sig, c, v, p, a, grid, block, LPC, derive, staged, scalar_in)) {
            // (trm_launch_column_sig.inl: without the derivation the signature instances store directly and take the scalar path)
            pid = derive == DERIVE_T_LIQ ? program_id(TRM_PROGRAM_COLUMN_EULER, H, LPC, DERIVE_T_LIQ, staged, scalar_in, sig) : program_id(TRM_PROGRAM_COLUMN_EULER, H, LPC, DERIVE_NONE, 0, 1, sig);
        }
        // with the derivation (every large or HBM-resident fp64 state): how the per-column outputs leave / inputs arrive
        else if (derive == DERIVE_T_LIQ) {
            pid = std::is_same<NF, double>::value ? program_id(TRM_PROGRAM_COLUMN_EULER, H, LPC, DERIVE_T_LIQ, staged, scalar_in, -1) : program_id(TRM_PROGRAM_COLUMN_EULER, H, LPC, DERIVE_T_LIQ, 0, 1, -1);
            if constexpr (!std::is_same<NF, double>::value) {
                // (fp32 off the packed kernel derives only on request: one instance)
                hipLaunchKernelGGL((k_column<NF, RICH, H, LPC, DERIVE_T_LIQ, PROG_EULER, false>), grid, block, 0, c->stream, v, p, a);
            } else {
                if (staged && scalar_in) hipLaunchKernelGGL((k_column<NF, RICH, H, LPC, DERIVE_T_LIQ, PROG_EULER, false, false, true, true>), grid, block, 0, c->stream, v, p, a);
                else if (staged) hipLaunchKernelGGL((k_column<NF, RICH, H, LPC, DERIVE_T_LIQ, PROG_EULER, false, false, true, false>), grid, block, 0, c->stream, v, p, a);
                else hipLaunchKernelGGL((k_column<NF, RICH, H, LPC, DERIVE_T_LIQ, PROG_EULER, false, false, false, true>), grid, block, 0, c->stream, v, p, a);     // (io_paths: never (0, 0))
            }
        }
        else { pid = program_id(TRM_PROGRAM_COLUMN_EULER, H, LPC, DERIVE_NONE, 0, 1, -1); hipLaunchKernelGGL((k_column<NF, RICH, H, LPC, DERIVE_NONE, PROG_EULER, false>), grid, block, 0, c->stream, v, p, a); }
    } else {
        // (Heun: the same signatures)
        const int hsig = (c->opt_bc_signature && H != HYD_GENERIC) ? bc_signature_of(c) : -1;
        const bool launched = launch_by_signature<ColumnSigHeunLaunch, NF, RICH>(hsig, c, v, p, a, grid, block, LPC);
        pid = program_id(TRM_PROGRAM_COLUMN_HEUN, H, LPC, DERIVE_NONE, 0, 1, launched ? hsig : -1);
        if (!launched) hipLaunchKernelGGL((k_column<NF, RICH, H, LPC, DERIVE_NONE, PROG, false>), grid, block, 0, c->stream, v, p, a);
    }
    TRM_HIP(c, hipGetLastError());
    c->last_program = pid;
    return TRM_OK;
}

template <class NF, bool RICH, int PROG> int ColumnLaunch<NF, RICH, PROG>::run(trm_ctx* c, const StepPlan& plan, double dt, int finalize, int nsteps) {
    int rc = TRM_OK;
    const bool deep = c->Nz > 32;
    TRM_BY_HYD(c, rc = deep ? (launch_column<NF, RICH, H, 64, PROG>(c, plan, dt, finalize, nsteps)) : (launch_column<NF, RICH, H, 32, PROG>(c, plan, dt, finalize, nsteps)));
    return rc;
}

}  // namespace trmh
