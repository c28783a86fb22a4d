// trm_launch_column_psi.inl -- k_column_psi<HYD, LPC, STAGED, SCALAR_IN, BCSIG, PSI_LAST | PSI_INTERIOR> (trm_column.hpp) for ONE boundary-condition
// signature: included by the trm_launch_column_psi_f64_*.hip files, each of which instantiates its signature.  Both compiled hydraulics,
// 32 and 64 lanes per column, and the two I/O combinations the deriving signature instances have (trm_launch_column_sig.inl).
#pragma once
#include "trm_host.hpp"

namespace trmh {

template <int SIG>
int ColumnPsiLaunch<SIG>::run(trm_ctx* c, dim3 grid, dim3 block, const View<double>& v, const DevParams<double>& p, const ColumnArgs<double>& a, int form, int staged, int scalar_in) {
    int rc = NO_INSTANCE;
    by_compiled_hyd(Policy<double>::hyd(c), [&](auto H) { by_lanes(c->Nz, [&](auto LPC) {
        by_value<PSI_LAST, PSI_INTERIOR>(form, [&](auto PSI) { by_io(staged, scalar_in, [&](auto ST, auto SC) {
            if constexpr (ST() != SC()) rc = run_column_psi<H(), LPC(), ST(), SC(), SIG, PSI()>(c, grid, block, v, p, a);
        }); });
    }); });
    return launched(c, rc, "k_column_psi: no instance for this launch");
}

}  // namespace trmh
