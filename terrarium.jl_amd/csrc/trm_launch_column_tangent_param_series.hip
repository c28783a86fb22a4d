// trm_launch_column_tangent_param_series.hip -- the launches of k_column_tangent<HYD, LPC, RIDE_PARAM_SERIES> (both
// lanes-per-column layouts; trm_column_tangent.hpp, trm_series_derivative.hpp): the forward-mode tangents with seeds on the thermal
// parameters (trm_tangent_param_set) of a run driven by boundary time series, whose node seeds ride along
// (TRM_OPT_DERIVATIVE_SERIES_PARAMS, trm_tangent_bc_series_upload).
#include "trm_launch_derivative.inl"

namespace trmh {
template int tangent_step<RIDE_PARAM_SERIES, NO_RECORD>(trm_ctx*, double, int);
}  // namespace trmh
