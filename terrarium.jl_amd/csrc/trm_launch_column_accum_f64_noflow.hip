// trm_launch_column_accum_f64_noflow.hip -- k_column_accum instantiations: double, NoFlow (see trm_launch_column_accum.inl)
#include "trm_launch_column_accum.inl"
namespace trmh {
template struct ColumnAccumLaunch<double, false>;
}  // namespace trmh
