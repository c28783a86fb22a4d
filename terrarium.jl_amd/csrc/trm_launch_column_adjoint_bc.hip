// trm_launch_column_adjoint_bc.hip -- the launches of k_column_adjoint<HYD, LPC, RIDE_BC> (both lanes-per-column layouts;
// trm_column_adjoint.hpp): the backward sweep of the per-step tape with the boundary gradients riding along (trm_adjoint_bc_open).
#include "trm_launch_derivative.inl"

namespace trmh {
template int adjoint_backward<false, RIDE_BC, NO_RECORD>(trm_ctx*, double, int, int, int, int);
}  // namespace trmh
