// trm_launch_column_tangent_bc.hip -- the launches of k_column_tangent<HYD, LPC, RIDE_BC> (both lanes-per-column layouts;
// trm_column_tangent.hpp): the forward-mode tangents with seeds on the boundary values (trm_tangent_bc_upload).
#include "trm_launch_derivative.inl"

namespace trmh {
template int tangent_step<RIDE_BC, NO_RECORD>(trm_ctx*, double, int);
}  // namespace trmh
