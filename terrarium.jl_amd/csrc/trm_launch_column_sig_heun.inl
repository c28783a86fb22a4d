// trm_launch_column_sig_heun.inl -- k_column<NF, RICH, ., ., DERIVE_NONE, PROG_HEUN, ..., BCSIG>: the one-launch Heun step with the
// boundary-condition signature compiled in (trm_kernels.hpp: BCSIG); included by the trm_launch_column_sig_heun_*.hip files.
#pragma once
#include "trm_host.hpp"

namespace trmh {

template <class NF, bool RICH, int SIG>
int ColumnSigHeunLaunch<NF, RICH, SIG>::run(trm_ctx* c, dim3 grid, dim3 block, const View<NF>& v, const DevParams<NF>& p, const ColumnArgs<NF>& a) {
    int rc = NO_INSTANCE;
    by_compiled_hyd(Policy<NF>::hyd(c), [&](auto H) { by_lanes(c->Nz, [&](auto LPC) {
        rc = run_column<NF, RICH, H(), LPC(), DERIVE_NONE, PROG_HEUN, false, false, false, true, SIG>(c, grid, block, v, p, a);
    }); });
    return launched(c, rc, "k_column: no instance for this launch");
}

}  // namespace trmh
