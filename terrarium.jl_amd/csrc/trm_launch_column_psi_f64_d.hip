// the fp64 Richards ForwardEuler program with the pressure head derived at entry (TRM_OPT_INTERIOR_STEPS), signature: prescribed surface temperature + infiltration flux
#include "trm_launch_column_psi.inl"
namespace trmh {
template struct ColumnPsiLaunch<BCSIG_T_TOP | BCSIG_FS_TOP>;
}  // namespace trmh
