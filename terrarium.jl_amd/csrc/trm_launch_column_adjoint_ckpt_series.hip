// trm_launch_column_adjoint_ckpt_series.hip -- the launches of k_column_adjoint_ckpt<HYD, LPC, RIDE_SERIES>
// (both lanes-per-column layouts; trm_column_adjoint_ckpt.hpp, trm_series_derivative.hpp): the backward sweep of the checkpointed tape
// with boundary time series evaluated in the launch and the gradients delivered per node of the series.
#include "trm_launch_derivative.inl"

namespace trmh {
template int adjoint_backward<true, RIDE_SERIES, NO_RECORD>(trm_ctx*, double, int, int, int, int);
}  // namespace trmh
