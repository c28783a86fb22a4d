// trm_launch_column_adjoint_rich_record.hip -- the launches of k_column_adjoint_rich_record<HYD, LPC> (three hydraulics, both
// lanes-per-column layouts; trm_column_adjoint_rich.hpp): the backward sweep of the heat + Richards per-step tape that reads an
// attached soil-moisture record inside the launch (TRM_OPT_DERIVATIVE_RICHARDS_RECORD, trm_adjoint_observe_record on a Richards
// context).  The sweep without a record is trm_launch_column_adjoint_rich.hip's.
#include "trm_launch_derivative.inl"

namespace trmh {
template int adjoint_backward_rich<false, true>(trm_ctx*, double, int, int, int);
}  // namespace trmh
