// trm_launch_column_adjoint_ckpt_record_series.hip -- the launches of k_column_adjoint_ckpt_record<HYD, LPC, RIDE_SERIES> (both lanes-per-column layouts; trm_column_adjoint_ckpt.hpp): the
// backward sweep of the checkpointed tape that reads an attached temperature record inside the launch (trm_adjoint_observe_record), with
// boundary time series evaluated in the launch and the gradients delivered per node of the series.
#include "trm_launch_derivative.inl"

namespace trmh {
template int adjoint_backward<true, RIDE_SERIES, WITH_RECORD>(trm_ctx*, double, int, int, int, int);
}  // namespace trmh
