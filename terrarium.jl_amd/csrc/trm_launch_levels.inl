// trm_launch_levels.inl -- columns of 65 ... 256 levels, M levels per lane: the launches of k_column_deep (M = 2,
// trm_column_deep.hpp) and k_column_wide (M = 4, trm_column_wide.hpp).  Included by trm_launch_deep_f64.hip / _f32.hip (M = 2) and
// trm_launch_wide_f64.hip / _f32.hip (M = 4).
#include "trm_host.hpp"
#include "trm_column_deep.hpp"
#include "trm_column_wide.hpp"

namespace trmh {

template <class NF, int M, bool RICH, int H, int PROG, bool GENERIC> static int launch_levels(trm_ctx* c, double dt, int finalize, int nsteps) {
    const LaunchArgs<NF>& la = launch_args<NF>(c);
    const ColumnArgs<NF> a = column_args<NF>(c, dt, finalize, nsteps, PROG);
    const dim3 grid((unsigned)((ncols(c) + (TRM_STEP_BLOCK / 64) - 1) / (TRM_STEP_BLOCK / 64))), block(TRM_STEP_BLOCK);
    // T / liq derived in registers: two levels per lane, branch-free kinds (no generic instance of its own)
    const bool derive = M == 2 && !GENERIC && Policy<NF>::template derive_now<RICH>(c) == DERIVE_T_LIQ;
    if constexpr (M == 4) hipLaunchKernelGGL((k_column_wide<NF, RICH, H, 4, PROG, GENERIC>), grid, block, 0, c->stream, state_view<NF>(c), la.p, a, la.stage);
    else if (derive) hipLaunchKernelGGL((k_column_deep<NF, RICH, H, true, PROG, false>), grid, block, 0, c->stream, state_view<NF>(c), la.p, a, la.stage);
    else hipLaunchKernelGGL((k_column_deep<NF, RICH, H, false, PROG, GENERIC>), grid, block, 0, c->stream, state_view<NF>(c), la.p, a, la.stage);
    TRM_HIP(c, hipGetLastError());
    // (lanes per column: 64, M levels each; bits 25-26 the program, 27 the generic boundary kinds)
    c->last_program = program_id(M == 2 ? TRM_PROGRAM_DEEP : TRM_PROGRAM_WIDE, H, 64, derive ? DERIVE_T_LIQ : DERIVE_NONE, 0, 1, -1) | (PROG << 25) | ((GENERIC ? 1 : 0) << 27);
    return TRM_OK;
}
template <class NF, int M, int PROG, bool GENERIC> static int levels_by_flow(trm_ctx* c, double dt, int finalize, int nsteps) {
    int rc = TRM_OK;
    if (Policy<NF>::richards(c)) { TRM_BY_HYD(c, rc = (launch_levels<NF, M, true, H, PROG, GENERIC>(c, dt, finalize, nsteps))); }
    else { TRM_BY_HYD(c, rc = (launch_levels<NF, M, false, H, PROG, GENERIC>(c, dt, finalize, nsteps))); }
    return rc;
}
template <class NF, int M> int LevelsLaunch<NF, M>::run(trm_ctx* c, int prog, bool generic, double dt, int finalize, int nsteps) {
    static_assert(M == 2 || M == 4, "two or four levels per lane");
    if (Policy<NF>::levels_per_lane(c) != M) return fail(c, TRM_EINVAL, M == 2 ? "k_column_deep serves columns of 65 ... 128 levels" : "k_column_wide serves columns of 129 ... 256 levels");
    if (prog == PROG_EULER) return generic ? levels_by_flow<NF, M, PROG_EULER, true>(c, dt, finalize, nsteps) : levels_by_flow<NF, M, PROG_EULER, false>(c, dt, finalize, nsteps);
    if (prog == PROG_HEUN) return generic ? levels_by_flow<NF, M, PROG_HEUN, true>(c, dt, finalize, nsteps) : levels_by_flow<NF, M, PROG_HEUN, false>(c, dt, finalize, nsteps);
    if constexpr (M == 2) {
        if (prog == PROG_MULTI && generic) return fail(c, TRM_EINVAL, "k_column_deep: the generic boundary kinds run one step per launch");
        if (prog == PROG_MULTI) return levels_by_flow<NF, M, PROG_MULTI, false>(c, dt, finalize, nsteps);
        return fail(c, TRM_EINVAL, "k_column_deep: unknown program");
    }
    return fail(c, TRM_EINVAL, "k_column_wide: one step per launch (ForwardEuler or Heun)");
}

}  // namespace trmh
