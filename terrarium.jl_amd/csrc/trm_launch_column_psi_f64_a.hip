// the fp64 Richards ForwardEuler program with the pressure head derived at entry (TRM_OPT_INTERIOR_STEPS), signature: no boundary condition set
#include "trm_launch_column_psi.inl"
namespace trmh {
template struct ColumnPsiLaunch<0>;
}  // namespace trmh
