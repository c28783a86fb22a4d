// trm_launch_record.hip -- attached temperature records (trm_adjoint_observe_record; DESIGN 4.8 "Attached records"): the dispatch from a
// ride to its record-reading backward launch (adjoint_backward_record, trm_launch_record.inl; the instances live in the
// trm_launch_column_adjoint{,_ckpt}_record*.hip files) and the launch of k_record_misfit (trm_column_adjoint.hpp), which sums the residuals a
// sweep wrote into the misfit per column.
#include "trm_host.hpp"
#include "trm_column_adjoint.hpp"

namespace trmh {

int RecordLaunch::backward(trm_ctx* c, bool ckpt, double dt, int nsteps, int slot, int fold, Ride ride, int first) {
    int rc = NO_INSTANCE;
    by_ride(ride, [&](auto r) {
        constexpr Ride R = decltype(r)::value;
        rc = ckpt ? adjoint_backward_record<true, R>(c, dt, nsteps, slot, fold, first) : adjoint_backward_record<false, R>(c, dt, nsteps, slot, fold, first);
    });
    return launched(c, rc, "k_column_adjoint_record: a ride without an instance");
}

int RecordLaunch::misfit(trm_ctx* c) {
    if (c->rec_npos < 1 || !c->d_rec_out) return fail(c, TRM_EINVAL, "k_record_misfit: no record is attached");
    const size_t cells = (size_t)c->rec_npos * (size_t)c->rec_nlevels * (size_t)c->Nh;
    hipLaunchKernelGGL((k_record_misfit<double>), dim3((unsigned)((c->Nh + 255) / 256)), dim3(256), 0, c->stream, (const double*)c->d_rec_out, c->d_rec_weight, c->d_rec_out + cells,
                       (long long)c->Nh, c->rec_npos, c->rec_nlevels);
    TRM_HIP(c, hipGetLastError());
    return TRM_OK;
}

}  // namespace trmh
