// trm_launch_land.hip -- the interleaved LandModel launches in fp64 (TRM_OPT_PIPELINE_PARTS = 1): k_land_euler (trm_column.hpp)
// steps the soil columns of one half of the context and evaluates the 0-D surface processes of the other half.
#include "trm_host.hpp"

namespace trmh {

template <int H, int LPC, int DERIVE, bool TOP_ARRAYS> static int run_land(trm_ctx* c, int qcol, int qsurf, double dt, int finalize) {
    using NF = double;
    const LaunchArgs<NF>& la = launch_args<NF>(c);
    const unsigned sblocks = (unsigned)((c->part_n[qsurf] + TRM_STEP_BLOCK - 1) / TRM_STEP_BLOCK);
    const ColumnArgs<NF> a = column_args<NF>(c, dt, finalize, 1, PROG_EULER);
    const long waves = (c->part_n[qcol] + (64 / LPC) - 1) / (64 / LPC);
    const dim3 grid(sblocks + (unsigned)((waves * 64 + TRM_STEP_BLOCK - 1) / TRM_STEP_BLOCK));
    TRM_LAUNCH(c, (k_land_euler<NF, true, H, LPC, DERIVE, TOP_ARRAYS>), grid, dim3(TRM_STEP_BLOCK), la.part[qcol], la.p, a, la.part[qsurf], (int)sblocks);
    c->last_program = program_id(TRM_PROGRAM_LAND_INTERLEAVED, H, LPC, DERIVE, 0, 1, -1);
    return TRM_OK;
}
template <> int LandLaunch<double>::run(trm_ctx* c, int qcol, int qsurf, double dt, int finalize, bool top_arrays) {
    using P = Policy<double>;
    if (top_arrays && !launch_args<double>(c).part[qsurf].top_T) return fail(c, TRM_EINVAL, "LandModel launch: the top-cell arrays were requested on a context that has none");
    const int derive = P::derive_now<true>(c) == DERIVE_T_LIQ ? DERIVE_T_LIQ : DERIVE_NONE;
    int rc = TRM_OK;
    by_hyd(P::hyd(c), [&](auto H) { by_lanes(c->Nz, [&](auto LPC) {
        by_value<DERIVE_NONE, DERIVE_T_LIQ>(derive, [&](auto D) { by_bool(top_arrays, [&](auto TOPS) {
            rc = run_land<H(), LPC(), D(), TOPS()>(c, qcol, qsurf, dt, finalize);
        }); });
    }); });
    return rc;
}

}  // namespace trmh
