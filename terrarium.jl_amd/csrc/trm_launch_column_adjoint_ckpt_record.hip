// trm_launch_column_adjoint_ckpt_record.hip -- the launches of k_column_adjoint_ckpt_record<HYD, LPC, RIDE_NONE> (both lanes-per-column layouts; trm_column_adjoint_ckpt.hpp): the
// backward sweep of the checkpointed tape that reads an attached temperature record inside the launch (trm_adjoint_observe_record), with
// nothing else riding along.
#include "trm_launch_derivative.inl"

namespace trmh {
template int adjoint_backward<true, RIDE_NONE, WITH_RECORD>(trm_ctx*, double, int, int, int, int);
}  // namespace trmh
