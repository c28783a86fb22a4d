// trm_launch_column_adjoint_ckpt.hip -- the launches of the strided k_column_record<HYD, LPC, true, CheckpointArgs> and k_column_adjoint_ckpt<HYD, LPC> (both
// lanes-per-column layouts; trm_column_adjoint_ckpt.hpp): the checkpointed tape of the reverse-mode gradients.
#include "trm_host.hpp"
#include "trm_column_adjoint_ckpt.hpp"

namespace trmh {

namespace {
CheckpointArgs checkpoint_args(const trm_ctx* c, int slot, int fold, int first, int every) {
    CheckpointArgs ca;
    ca.lU = c->d_adj[TRM_ADJOINT_INTERNAL_ENERGY];
    ca.lT = c->d_adj[TRM_ADJOINT_TEMPERATURE];
    ca.lliq = c->d_adj[TRM_ADJOINT_LIQUID_WATER_FRACTION];
    ca.slot_elems = (long long)c->Nh * (long long)c->Nzp;
    ca.tape = c->d_tape + (size_t)slot * (size_t)ca.slot_elems;
    ca.generic = Policy<double>::generic_bcs(c) ? 1 : 0;
    ca.fold = fold;
    ca.first = first;
    ca.every = every;
    return ca;
}

template <int H, int LPC, bool BACKWARD> int launch_checkpoint(trm_ctx* c, double dt, int nsteps, int slot, int fold, int first, int every) {
    const LaunchArgs<double>& la = launch_args<double>(c);
    const ColumnArgs<double> a = column_args<double>(c, dt, 1, nsteps, PROG_EULER);
    const CheckpointArgs ca = checkpoint_args(c, slot, fold, first, every);
    // the backward launch holds the segment's states in dynamic LDS: 2 KiB per step and workgroup, sized by the segment
    const size_t lds = BACKWARD ? (size_t)nsteps * TRM_STEP_BLOCK * sizeof(double) : 0;
    if (BACKWARD) hipLaunchKernelGGL((k_column_adjoint_ckpt<H, LPC>), column_grid(c, LPC), dim3(TRM_STEP_BLOCK), lds, c->stream, la.state, la.p, a, ca);
    else hipLaunchKernelGGL((k_column_record<H, LPC, true, CheckpointArgs>), column_grid(c, LPC), dim3(TRM_STEP_BLOCK), 0, c->stream, la.state, la.p, a, ca);
    TRM_HIP(c, hipGetLastError());
    c->last_program = program_id(TRM_PROGRAM_COLUMN_ADJOINT, H, LPC, DERIVE_NONE, 0, 0, -1) | (ca.generic ? 1 << 25 : 0) | (BACKWARD ? 1 << 26 : 0) | 1 << 27;
    return TRM_OK;
}
}  // namespace

int CheckpointLaunch::record(trm_ctx* c, double dt, int nsteps, int slot, int first, int every) {
    if (slot < 0 || nsteps < 0 || first < 0 || every < 1) return fail(c, TRM_EINVAL, "k_column_record (strided): bad launch");
    const int stores = first < nsteps ? (nsteps - first + every - 1) / every : 0;
    if (slot + stores > c->tape_cap) return fail(c, TRM_EINVAL, "k_column_record (strided): the launch leaves the tape");
    if (stores == 0) slot = 0;     // (no store: any address inside the tape)
    int rc = TRM_OK;
    using NF = double;
    const bool deep = c->Nz > 32;
    TRM_BY_HYD(c, rc = deep ? (launch_checkpoint<H, 64, false>(c, dt, nsteps, slot, 0, first, every))
                            : (launch_checkpoint<H, 32, false>(c, dt, nsteps, slot, 0, first, every)));
    return rc;
}

int CheckpointLaunch::backward(trm_ctx* c, double dt, int nsteps, int slot, int fold) {
    if (slot < 0 || nsteps < 0 || nsteps > TRM_ADJOINT_MAX_INTERVAL || slot >= c->tape_cap)
        return fail(c, TRM_EINVAL, "k_column_adjoint_ckpt: the launch leaves the tape");
    int rc = TRM_OK;
    using NF = double;
    const bool deep = c->Nz > 32;
    TRM_BY_HYD(c, rc = deep ? (launch_checkpoint<H, 64, true>(c, dt, nsteps, slot, fold, 0, 1)) : (launch_checkpoint<H, 32, true>(c, dt, nsteps, slot, fold, 0, 1)));
    return rc;
}

}  // namespace trmh
