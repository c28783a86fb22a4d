// trm_launch_column_adjoint_rich_param.hip -- the launches of k_column_adjoint_rich_params<HYD, LPC> (three hydraulics, both
// lanes-per-column layouts) and k_hyd_param_reduce (trm_column_adjoint_rich.hpp): the backward sweep of the heat + Richards per-step tape
// with the gradients with respect to the seven hydraulic parameters beside it (TRM_OPT_DERIVATIVE_RICHARDS_PARAMS, trm_adjoint_param_open
// on a Richards context).  The record is trm_launch_column_adjoint_rich.hip's.
#include "trm_launch_derivative.inl"

namespace trmh {
template int adjoint_backward_rich<true, false>(trm_ctx*, double, int, int, int);
int AdjointRichLaunch::param_reduce(trm_ctx* c) { return adjoint_rich_param_reduce<>(c); }
}  // namespace trmh
