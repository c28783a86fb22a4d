// trm_launch_column_psi.inl -- k_column_psi<HYD, LPC, STAGED, SCALAR_IN, BCSIG, PSI_LAST | PSI_INTERIOR> (trm_column.hpp) for ONE boundary-condition
// signature: included by the trm_launch_column_psi_f64_*.hip files, each of which instantiates its signature.  Both compiled hydraulics,
// 32 and 64 lanes per column, and the two I/O combinations the deriving signature instances have (trm_launch_column_sig.inl).
#include "trm_host.hpp"

namespace trmh {

template <int SIG, int H, int LPC, int PSI>
static void launch_column_psi(trm_ctx* c, const View<double>& v, const DevParams<double>& p, const ColumnArgs<double>& a, dim3 grid, dim3 block, int staged) {
    if (staged) hipLaunchKernelGGL((k_column_psi<H, LPC, true, false, SIG, PSI>), grid, block, 0, c->stream, v, p, a);
    else hipLaunchKernelGGL((k_column_psi<H, LPC, false, true, SIG, PSI>), grid, block, 0, c->stream, v, p, a);
}

template <int SIG>
void ColumnPsiLaunch<SIG>::run(trm_ctx* c, const View<double>& v, const DevParams<double>& p, const ColumnArgs<double>& a, dim3 grid, dim3 block, int lpc, int form, int staged, int scalar_in) {
    using NF = double;
    (void)scalar_in;      // (the caller has reduced the pair to (0, 1) or (1, 0))
    if (form == PSI_INTERIOR) {
        TRM_BY_COMPILED_HYD(c, (lpc == 64 ? (launch_column_psi<SIG, H, 64, PSI_INTERIOR>(c, v, p, a, grid, block, staged))
                                 : (launch_column_psi<SIG, H, 32, PSI_INTERIOR>(c, v, p, a, grid, block, staged))));
    } else {
        TRM_BY_COMPILED_HYD(c, (lpc == 64 ? (launch_column_psi<SIG, H, 64, PSI_LAST>(c, v, p, a, grid, block, staged))
                                 : (launch_column_psi<SIG, H, 32, PSI_LAST>(c, v, p, a, grid, block, staged))));
    }
}

}  // namespace trmh
