// trm_launch_column_land_bc.hip -- k_column_land with the reference-default hydraulics (see trm_launch_column_land.inl)
#include "trm_launch_column_land.inl"
namespace trmh {
extern template int FrontLaunch::run_hyd<HYD_VG_N2>(trm_ctx*, const StepPlan&, double, int, bool);     // (trm_launch_column_land_vg.hip)
template int FrontLaunch::run_hyd<HYD_BC_LINEAR>(trm_ctx*, const StepPlan&, double, int, bool);
int FrontLaunch::run(trm_ctx* c, const StepPlan& plan, double dt, int finalize, bool heun) {
    int rc = NO_INSTANCE;
    by_compiled_hyd(Policy<double>::hyd(c), [&](auto H) { rc = run_hyd<H()>(c, plan, dt, finalize, heun); });
    return launched(c, rc, "k_column_land: no instance for the generic hydraulics");
}
}  // namespace trmh
