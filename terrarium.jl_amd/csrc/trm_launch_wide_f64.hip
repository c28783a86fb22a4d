// trm_launch_wide_f64.hip -- k_column_wide instantiations, double (see trm_launch_levels.inl)
#include "trm_launch_levels.inl"
namespace trmh {
template struct LevelsLaunch<double, 4>;
}  // namespace trmh
