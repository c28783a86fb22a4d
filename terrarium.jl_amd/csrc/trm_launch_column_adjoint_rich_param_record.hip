// trm_launch_column_adjoint_rich_param_record.hip -- the launches of k_column_adjoint_rich_params_record<HYD, LPC> (three hydraulics,
// both lanes-per-column layouts; trm_column_adjoint_rich.hpp): the record-reading backward sweep of the heat + Richards per-step
// tape with the hydraulic-parameter gradients beside it (TRM_OPT_DERIVATIVE_RICHARDS_RECORD and TRM_OPT_DERIVATIVE_RICHARDS_PARAMS).  The
// reduction that ends the sweep is trm_launch_column_adjoint_rich_param.hip's.
#include "trm_launch_derivative.inl"

namespace trmh {
template int adjoint_backward_rich<true, true>(trm_ctx*, double, int, int, int);
}  // namespace trmh
