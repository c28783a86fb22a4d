// trm_launch_column_tangent.hip -- the launches of k_column_tangent<HYD, LPC, RIDE_NONE> (both lanes-per-column layouts) and k_closure_tangent<RIDE_NONE>
// (trm_column_tangent.hpp): forward-mode tangents of the heat-only fp64 SoilModel step.
#include "trm_launch_derivative.inl"

namespace trmh {
template int tangent_step<RIDE_NONE, NO_RECORD>(trm_ctx*, double, int);
template int tangent_closure<RIDE_NONE>(trm_ctx*);
}  // namespace trmh
