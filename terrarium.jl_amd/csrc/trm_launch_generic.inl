// trm_launch_generic.inl -- the step kernels that serve every boundary kind (Gradient conditions, Value conditions on liquid
// fraction / saturation / pressure head, a per-cell vwc_forcing field): k_step_wave (ForwardEuler, trm_kernels.hpp) and
// k_heun_generic (Heun in one launch, trm_column.hpp).  Included by trm_launch_generic_f64.hip / _f32.hip.
#include "trm_host.hpp"

namespace trmh {

template <class NF, bool RICH, int H, int LPC> static int launch_wave(trm_ctx* c, double dt, int finalize) {
    const LaunchArgs<NF>& la = launch_args<NF>(c);
    TRM_LAUNCH(c, (k_step_wave<NF, RICH, H, LPC>), column_grid(c, LPC), dim3(TRM_STEP_BLOCK), state_view<NF>(c), la.p, (NF)dt, finalize, write_kf(c, finalize));
    c->last_program = program_id(TRM_PROGRAM_GENERIC_EULER, H, LPC, DERIVE_NONE, 0, 0, -1);
    return TRM_OK;
}
// Heun with the generic boundary kinds: k_heun_generic, one launch per step like k_column<PROG_HEUN>
template <class NF, bool RICH, int H, int LPC> static int launch_heun_generic(trm_ctx* c, double dt, int finalize) {
    const LaunchArgs<NF>& la = launch_args<NF>(c);
    const ColumnArgs<NF> a = column_args<NF>(c, dt, finalize, 1, PROG_HEUN);
    TRM_LAUNCH(c, (k_heun_generic<NF, RICH, H, LPC>), column_grid(c, LPC), dim3(TRM_STEP_BLOCK), la.state, la.p, la.stage, a);
    c->last_program = program_id(TRM_PROGRAM_GENERIC_HEUN, H, LPC, DERIVE_NONE, 0, 0, -1);
    return TRM_OK;
}
template <class NF, bool HEUN> static int generic_launch(trm_ctx* c, double dt, int finalize) {
    int rc = TRM_OK;
    by_bool(Policy<NF>::richards(c), [&](auto RICH) { by_hyd(Policy<NF>::hyd(c), [&](auto H) { by_lanes(c->Nz, [&](auto LPC) {
        if constexpr (HEUN) rc = launch_heun_generic<NF, RICH(), H(), LPC()>(c, dt, finalize);
        else rc = launch_wave<NF, RICH(), H(), LPC()>(c, dt, finalize);
    }); }); });
    return rc;
}
template <class NF> int GenericLaunch<NF>::step(trm_ctx* c, double dt, int finalize) { return generic_launch<NF, false>(c, dt, finalize); }
template <class NF> int GenericLaunch<NF>::heun(trm_ctx* c, double dt, int finalize) { return generic_launch<NF, true>(c, dt, finalize); }

}  // namespace trmh
