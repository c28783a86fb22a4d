// trm_launch_column_adjoint_ckpt.hip -- the launches of the strided k_column_record<HYD, LPC, true, false> and k_column_adjoint_ckpt<HYD, LPC, RIDE_NONE>
// (both lanes-per-column layouts; trm_column_adjoint_ckpt.hpp): the checkpointed tape of the reverse-mode gradients.
#include "trm_launch_derivative.inl"

namespace trmh {
template int adjoint_record<true, false>(trm_ctx*, double, int, int, int, int);
template int adjoint_backward<true, RIDE_NONE, NO_RECORD>(trm_ctx*, double, int, int, int, int);
}  // namespace trmh
