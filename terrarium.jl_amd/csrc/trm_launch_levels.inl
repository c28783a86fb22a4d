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
    if constexpr (M == 4) TRM_LAUNCH(c, (k_column_wide<NF, RICH, H, 4, PROG, GENERIC>), grid, block, state_view<NF>(c), la.p, a, la.stage);
    else if (derive) TRM_LAUNCH(c, (k_column_deep<NF, RICH, H, true, PROG, false>), grid, block, state_view<NF>(c), la.p, a, la.stage);
    else TRM_LAUNCH(c, (k_column_deep<NF, RICH, H, false, PROG, GENERIC>), grid, block, state_view<NF>(c), la.p, a, la.stage);
    // (lanes per column: 64, M levels each; bits 25-26 the program, 27 the generic boundary kinds)
    c->last_program = program_id(M == 2 ? TRM_PROGRAM_DEEP : TRM_PROGRAM_WIDE, H, 64, derive ? DERIVE_T_LIQ : DERIVE_NONE, 0, 1, -1) | (PROG << 25) | ((GENERIC ? 1 : 0) << 27);
    return TRM_OK;
}
template <class NF, int M> int LevelsLaunch<NF, M>::run(trm_ctx* c, int prog, bool generic, double dt, int finalize, int nsteps) {
    static_assert(M == 2 || M == 4, "two or four levels per lane");
    if (Policy<NF>::levels_per_lane(c) != M) return fail(c, TRM_EINVAL, M == 2 ? "k_column_deep serves columns of 65 ... 128 levels" : "k_column_wide serves columns of 129 ... 256 levels");
    if (M == 2 && prog == PROG_MULTI && generic) return fail(c, TRM_EINVAL, "k_column_deep: the generic boundary kinds run one step per launch");
    int rc = NO_INSTANCE;
    by_value<PROG_EULER, PROG_HEUN, PROG_MULTI>(prog, [&](auto PROG) { by_bool(generic, [&](auto GENERIC) {
        // (the multi-step program: k_column_deep with the branch-free kinds alone)
        if constexpr (PROG() != PROG_MULTI || (M == 2 && !GENERIC()))
            by_bool(Policy<NF>::richards(c), [&](auto RICH) { by_hyd(Policy<NF>::hyd(c), [&](auto H) {
                rc = launch_levels<NF, M, RICH(), H(), PROG(), GENERIC()>(c, dt, finalize, nsteps);
            }); });
    }); });
    return launched(c, rc, M == 2 ? "k_column_deep: unknown program" : "k_column_wide: one step per launch (ForwardEuler or Heun)");
}

}  // namespace trmh
