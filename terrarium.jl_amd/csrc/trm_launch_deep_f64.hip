// trm_launch_deep_f64.hip -- k_column_deep instantiations, double (see trm_launch_levels.inl)
#include "trm_launch_levels.inl"
namespace trmh {
template struct LevelsLaunch<double, 2>;
}  // namespace trmh
