// trm_launch_column_accum_f32.hip -- k_column_accum instantiations: float (see trm_launch_column_accum.inl)
#include "trm_launch_column_accum.inl"
namespace trmh {
template struct ColumnAccumLaunch<float, true>;
template struct ColumnAccumLaunch<float, false>;
}  // namespace trmh
