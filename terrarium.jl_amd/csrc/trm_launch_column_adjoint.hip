// trm_launch_column_adjoint.hip -- the launches of k_column_record<HYD, LPC, false, false> and k_column_adjoint<HYD, LPC, RIDE_NONE> (both lanes-per-column
// layouts; trm_column_adjoint.hpp): reverse-mode gradients of the heat-only fp64 SoilModel run.
#include "trm_launch_derivative.inl"

namespace trmh {
template int adjoint_record<false, false>(trm_ctx*, double, int, int, int, int);
template int adjoint_backward<false, RIDE_NONE, NO_RECORD>(trm_ctx*, double, int, int, int, int);
}  // namespace trmh
