// trm_launch_column_adjoint_series.hip -- the launches of k_column_record<HYD, LPC, STRIDED, true> (both tapes) and
// k_column_adjoint<HYD, LPC, RIDE_SERIES> (both lanes-per-column layouts; trm_column_adjoint.hpp,
// trm_series_derivative.hpp): the record and the backward sweep of the per-step tape with boundary time series evaluated in the launch
// and the gradients delivered per node of the series (TRM_OPT_DERIVATIVE_SERIES, trm_adjoint_bc_series_download).
#include "trm_launch_derivative.inl"

namespace trmh {
template int adjoint_record<false, true>(trm_ctx*, double, int, int, int, int);
template int adjoint_record<true, true>(trm_ctx*, double, int, int, int, int);
template int adjoint_backward<false, RIDE_SERIES, NO_RECORD>(trm_ctx*, double, int, int, int, int);
}  // namespace trmh
