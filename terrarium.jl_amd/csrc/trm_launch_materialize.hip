// trm_launch_materialize.hip -- k_materialize_closure (trm_column.hpp): temperature and liquid_water_fraction of the whole state from
// its stored (internal_energy, saturation), after per-step launches that did not store them (TRM_OPT_DEFER_CLOSURE_STORES).
#include "trm_host.hpp"

namespace trmh {

// the grid of the step launches (column_grid), every column of the context whatever part the launch helpers address
template <class NF> int MaterializeLaunch<NF>::run(trm_ctx* c) {
    if (c->Nz > 64) return fail(c, TRM_EINVAL, "k_materialize_closure: one level per lane (<= 64 levels)");
    const LaunchArgs<NF>& la = launch_args<NF>(c);
    const int part = c->part;
    c->part = -1;
    const dim3 grid = column_grid(c, lanes_per_column(c->Nz)), block(TRM_STEP_BLOCK);
    c->part = part;
    by_lanes(c->Nz, [&](auto LPC) { hipLaunchKernelGGL((k_materialize_closure<NF, LPC()>), grid, block, 0, c->stream, la.state, la.p); });
    TRM_HIP(c, hipGetLastError());
    return TRM_OK;
}

template struct MaterializeLaunch<double>;
template struct MaterializeLaunch<float>;

}  // namespace trmh
