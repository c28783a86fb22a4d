// trm_launch_column_adjoint_param.hip -- the launches of k_column_adjoint<HYD, LPC, RIDE_PARAM> (both lanes-per-column
// layouts) and k_param_reduce (trm_column_adjoint.hpp): the backward sweep of the per-step tape with the boundary and the thermal
// parameter gradients riding along (trm_adjoint_param_open), and the reduction that ends a sweep on either tape.
#include "trm_launch_derivative.inl"

namespace trmh {
template int adjoint_backward<false, RIDE_PARAM, NO_RECORD>(trm_ctx*, double, int, int, int, int);

int AdjointLaunch::param_reduce(trm_ctx* c) {
    if (!c->d_adj_param_out) return fail(c, TRM_EINVAL, "k_param_reduce: no accumulators");
    if (int rc = arrays_ok(c, c->d_adj_param, "k_param_reduce", "accumulators")) return rc;
    ParamChain ch;
    thermal_param_chain(c->params, launch_args<double>(c).p, ch.w);
    hipLaunchKernelGGL((k_param_reduce<ParamGradPtrs>), dim3((unsigned)((c->Nh + 255) / 256)), dim3(256), 0, c->stream, param_grad_ptrs(c), ch, c->d_adj_param_out,
                       (long long)c->Nh, c->Nz, c->Nzp);
    TRM_HIP(c, hipGetLastError());
    return TRM_OK;
}
}  // namespace trmh
