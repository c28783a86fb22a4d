// trm_launch_column_tangent_record_param_series.hip -- the launches of k_column_tangent_record<HYD, LPC, RIDE_PARAM_SERIES> (both lanes-per-column layouts;
// trm_column_tangent_record.hpp): the forward-mode tangents with seeds on the thermal parameters of a run driven by boundary time series (TRM_OPT_DERIVATIVE_SERIES_PARAMS) with a tangent record attached
// (trm_tangent_record_attach), T and dT sampled inside the launch.
#include "trm_launch_derivative.inl"

namespace trmh {
template int tangent_step<RIDE_PARAM_SERIES, WITH_RECORD>(trm_ctx*, double, int);
}  // namespace trmh
