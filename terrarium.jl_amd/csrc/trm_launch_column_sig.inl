// trm_launch_column_sig.inl -- k_column<NF, RICH, ., ., DERIVE_T_LIQ | DERIVE_NONE, PROG_EULER, ..., STAGED, SCALAR_IN, BCSIG> for ONE boundary-condition
// signature (trm_kernels.hpp: BCSIG): included by the trm_launch_column_sig_*.hip files, each of which instantiates its signatures.
#pragma once
#include "trm_host.hpp"

namespace trmh {

template <class NF, bool RICH, int SIG>
int ColumnSigLaunch<NF, RICH, SIG>::run(trm_ctx* c, dim3 grid, dim3 block, const View<NF>& v, const DevParams<NF>& p, const ColumnArgs<NF>& a, int derive, int staged, int scalar_in) {
    int rc = NO_INSTANCE;
    by_compiled_hyd(Policy<NF>::hyd(c), [&](auto H) { by_lanes(c->Nz, [&](auto LPC) {
        // (T and liq read as stored -- small grids, the vegetation-coupled LandModel, the first step after an upload: direct stores, scalar inputs)
        if (derive != DERIVE_T_LIQ) rc = run_column<NF, RICH, H(), LPC(), DERIVE_NONE, PROG_EULER, false, false, false, true, SIG>(c, grid, block, v, p, a);
        // (1, 1) exists for the LandModel alone (Policy::io_paths)
        else by_io(staged, scalar_in, [&](auto ST, auto SC) {
            if constexpr (SIG == BCSIG_LAND || !(ST() && SC())) rc = run_column<NF, RICH, H(), LPC(), DERIVE_T_LIQ, PROG_EULER, false, false, ST(), SC(), SIG>(c, grid, block, v, p, a);
        });
    }); });
    return launched(c, rc, "k_column: no instance for this launch");
}

}  // namespace trmh
