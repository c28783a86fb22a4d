// trm_launch_column_tangent_rich.hip -- the launches of k_column_tangent_rich<HYD, LPC> (three hydraulics, both lanes-per-column layouts)
// and k_closure_tangent_rich<HYD> (trm_column_tangent_rich.hpp): forward-mode tangents of the heat + Richards fp64 SoilModel step with
// seeds on the initial internal energy and saturation (TRM_OPT_DERIVATIVE_RICHARDS).
#include "trm_launch_derivative.inl"

namespace trmh {
int TangentRichLaunch::step(trm_ctx* c, double dt, int nsteps) { return tangent_step_rich<>(c, dt, nsteps); }
int TangentRichLaunch::closure(trm_ctx* c) { return tangent_closure_rich<>(c); }
}  // namespace trmh
