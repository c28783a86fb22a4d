// trm_launch_column_tangent_param.hip -- the launches of k_column_tangent<HYD, LPC, RIDE_PARAM> (both lanes-per-column
// layouts) and k_closure_tangent<RIDE_PARAM> (trm_column_tangent.hpp): the forward-mode tangents with seeds on the thermal
// parameters (trm_tangent_param_set); the boundary seeds ride along, zero unless trm_tangent_bc_upload has set them.
#include "trm_launch_derivative.inl"

namespace trmh {
template int tangent_step<RIDE_PARAM, NO_RECORD>(trm_ctx*, double, int);
template int tangent_closure<RIDE_PARAM>(trm_ctx*);
}  // namespace trmh
