// trm_launch_record.hip -- attached temperature records (trm_adjoint_observe_record; DESIGN 4.8 "Attached records"): the launch of
// k_record_misfit (trm_column_adjoint.hpp), which sums the residuals a sweep wrote into the misfit per column.  The record-reading backward
// launches are adjoint_backward<CKPT, R, WITH_RECORD> (trm_launch_derivative.inl; trm_launch_column_adjoint{,_ckpt}_record*.hip).
#include "trm_host.hpp"
#include "trm_column_adjoint.hpp"

namespace trmh {

int RecordLaunch::misfit(trm_ctx* c) {
    if (c->rec.npos < 1 || !c->d_rec_out) return fail(c, TRM_EINVAL, "k_record_misfit: no record is attached");
    const size_t cells = (size_t)c->rec.npos * (size_t)c->rec.nlevels * (size_t)c->Nh;
    hipLaunchKernelGGL((k_record_misfit<double>), dim3((unsigned)((c->Nh + 255) / 256)), dim3(256), 0, c->stream, (const double*)c->d_rec_out, c->d_rec_weight, c->d_rec_out + cells,
                       (long long)c->Nh, c->rec.npos, c->rec.nlevels);
    TRM_HIP(c, hipGetLastError());
    return TRM_OK;
}

}  // namespace trmh
