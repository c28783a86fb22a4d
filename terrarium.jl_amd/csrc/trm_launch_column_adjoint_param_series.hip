// trm_launch_column_adjoint_param_series.hip -- the launches of k_column_adjoint<HYD, LPC, RIDE_PARAM_SERIES> (both
// lanes-per-column layouts; trm_column_adjoint.hpp, trm_series_derivative.hpp): the backward sweep of the per-step tape of a run driven by
// boundary time series, with the node gradients and the thermal parameter gradients riding along (TRM_OPT_DERIVATIVE_SERIES_PARAMS,
// trm_adjoint_param_open).  The record is the series one (trm_launch_column_adjoint_series.hip), k_param_reduce ends the sweep
// (trm_launch_column_adjoint_param.hip).
#include "trm_launch_derivative.inl"

namespace trmh {
template int adjoint_backward<false, RIDE_PARAM_SERIES, NO_RECORD>(trm_ctx*, double, int, int, int, int);
}  // namespace trmh
