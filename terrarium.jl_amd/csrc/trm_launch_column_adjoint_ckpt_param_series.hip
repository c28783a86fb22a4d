// trm_launch_column_adjoint_ckpt_param_series.hip -- the launches of k_column_adjoint_ckpt<HYD, LPC, RIDE_PARAM_SERIES>
// (both lanes-per-column layouts; trm_column_adjoint_ckpt.hpp, trm_series_derivative.hpp): the backward sweep of the checkpointed
// tape of a run driven by boundary time series, with the node gradients and the thermal parameter gradients riding along.
#include "trm_launch_derivative.inl"

namespace trmh {
template int adjoint_backward<true, RIDE_PARAM_SERIES, NO_RECORD>(trm_ctx*, double, int, int, int, int);
}  // namespace trmh
