// trm_launch_column_tangent_record_bc.hip -- the launches of k_column_tangent_record<HYD, LPC, RIDE_BC> (both lanes-per-column layouts;
// trm_column_tangent_record.hpp): the forward-mode tangents with seeds on the boundary values (trm_tangent_bc_upload) with a tangent record attached
// (trm_tangent_record_attach), T and dT sampled inside the launch.
#include "trm_launch_derivative.inl"

namespace trmh {
template int tangent_step<RIDE_BC, WITH_RECORD>(trm_ctx*, double, int);
}  // namespace trmh
