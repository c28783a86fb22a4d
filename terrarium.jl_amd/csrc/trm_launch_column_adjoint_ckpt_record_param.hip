// trm_launch_column_adjoint_ckpt_record_param.hip -- the launches of k_column_adjoint_ckpt_record<HYD, LPC, RIDE_PARAM> (both lanes-per-column layouts; trm_column_adjoint_ckpt.hpp): the
// backward sweep of the checkpointed tape that reads an attached temperature record inside the launch (trm_adjoint_observe_record), with
// the boundary and the thermal-parameter gradients riding along (trm_adjoint_param_open).
#include "trm_launch_derivative.inl"

namespace trmh {
template int adjoint_backward<true, RIDE_PARAM, WITH_RECORD>(trm_ctx*, double, int, int, int, int);
}  // namespace trmh
