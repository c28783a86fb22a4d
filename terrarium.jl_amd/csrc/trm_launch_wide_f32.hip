// trm_launch_wide_f32.hip -- k_column_wide instantiations, float (see trm_launch_levels.inl)
#include "trm_launch_levels.inl"
namespace trmh {
template struct LevelsLaunch<float, 4>;
}  // namespace trmh
