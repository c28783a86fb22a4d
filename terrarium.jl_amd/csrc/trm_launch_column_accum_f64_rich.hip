// trm_launch_column_accum_f64_rich.hip -- k_column_accum instantiations: double, Richards (see trm_launch_column_accum.inl)
#include "trm_launch_column_accum.inl"
namespace trmh {
template struct ColumnAccumLaunch<double, true>;
}  // namespace trmh
