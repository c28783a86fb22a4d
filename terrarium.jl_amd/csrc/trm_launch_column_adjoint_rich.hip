// trm_launch_column_adjoint_rich.hip -- the launches of k_column_record_rich<HYD, LPC> and k_column_adjoint_rich<HYD, LPC> (three
// hydraulics, both lanes-per-column layouts; trm_column_adjoint_rich.hpp): reverse-mode gradients of the heat + Richards fp64 SoilModel run
// with respect to the initial internal energy and saturation (TRM_OPT_DERIVATIVE_RICHARDS_ADJOINT).
#include "trm_launch_derivative.inl"

namespace trmh {
int AdjointRichLaunch::record(trm_ctx* c, double dt, int nsteps, int slot) { return adjoint_record_rich<>(c, dt, nsteps, slot); }
template int adjoint_backward_rich<false, false>(trm_ctx*, double, int, int, int);
}  // namespace trmh
