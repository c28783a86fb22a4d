// trm_launch_column_adjoint_record.hip -- the launches of k_column_adjoint_record<HYD, LPC, RIDE_NONE> (both lanes-per-column layouts; trm_column_adjoint.hpp): the
// backward sweep of the per-step tape that reads an attached temperature record inside the launch (trm_adjoint_observe_record), with
// nothing else riding along.
#include "trm_launch_derivative.inl"

namespace trmh {
template int adjoint_backward<false, RIDE_NONE, WITH_RECORD>(trm_ctx*, double, int, int, int, int);
}  // namespace trmh
