// trm_launch_column_adjoint_rich_record.hip -- the launches of k_column_adjoint_rich_record<HYD, LPC> (three hydraulics, both
// lanes-per-column layouts; trm_column_adjoint_rich_record.hpp): the backward sweep of the heat + Richards per-step tape that reads an
// attached soil-moisture record inside the launch (TRM_OPT_DERIVATIVE_RICHARDS_RECORD, trm_adjoint_observe_record on a Richards
// context).  The sweep without a record is trm_launch_column_adjoint_rich.hip's.
#include "trm_launch_derivative.inl"

namespace trmh {
int AdjointRichLaunch::backward_record(trm_ctx* c, double dt, int nsteps, int slot, int fold) { return adjoint_backward_rich_record<>(c, dt, nsteps, slot, fold); }
}  // namespace trmh
