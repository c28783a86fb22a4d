// trm_launch_column_adjoint_ckpt_param.hip -- the launches of k_column_adjoint_ckpt<HYD, LPC, RIDE_PARAM> (both
// lanes-per-column layouts; trm_column_adjoint_ckpt.hpp): the backward sweep of the checkpointed tape with the boundary and the thermal
// parameter gradients riding along.
#include "trm_launch_derivative.inl"

namespace trmh {
template int adjoint_backward<true, RIDE_PARAM, NO_RECORD>(trm_ctx*, double, int, int, int, int);
}  // namespace trmh
