// trm_launch_deep_f32.hip -- k_column_deep instantiations, float (see trm_launch_levels.inl)
#include "trm_launch_levels.inl"
namespace trmh {
template struct LevelsLaunch<float, 2>;
}  // namespace trmh
