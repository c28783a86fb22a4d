// trm_launch_column_tangent_series.hip -- the launches of k_column_tangent<HYD, LPC, RIDE_SERIES> (both
// lanes-per-column layouts; trm_column_tangent.hpp, trm_series_derivative.hpp): the forward-mode tangents with boundary time series
// evaluated in the launch and seeds shaped like the series (TRM_OPT_DERIVATIVE_SERIES, trm_tangent_bc_series_upload).
#include "trm_launch_derivative.inl"

namespace trmh {
template int tangent_step<RIDE_SERIES, NO_RECORD>(trm_ctx*, double, int);
}  // namespace trmh
