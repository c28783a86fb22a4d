// trm_launch_record.inl -- the launches of the record-reading backward sweeps, k_column_adjoint_record (trm_column_adjoint.hpp) and
// k_column_adjoint_ckpt_record (trm_column_adjoint_ckpt.hpp): the sweeps of trm_launch_derivative.inl with a temperature record attached
// to the open adjoint (trm_adjoint_observe_record; DESIGN 4.8 "Attached records").  Included by the
// trm_launch_column_adjoint{,_ckpt}_record*.hip files, each of which instantiates the launcher of one tape and ride.
#include "trm_launch_derivative.inl"

namespace trmh {

// the record as a launch whose first step is taped position `first` sees it
inline RecordArgs record_args(const trm_ctx* c, int first) {
    RecordArgs r;
    const int32_t* tables = (const int32_t*)c->d_rec_tables;
    r.row_of_level = tables;
    r.row_of_position = tables + c->Nz + first;
    r.observed = c->d_rec_observed;
    r.weight = c->d_rec_weight;
    r.residual = c->d_rec_out;
    r.nlevels = c->rec_nlevels;
    return r;
}
// the tables are those of this tape, and the launch's positions first ... first + nsteps are inside them
inline int record_launch_ok(trm_ctx* c, int nsteps, int first, const std::string& who) {
    if (c->rec_npos < 1 || !c->d_rec_tables || !c->d_rec_observed || !c->d_rec_out || c->rec_table_n < 0)
        return fail(c, TRM_EINVAL, who + ": no record is attached, or its tables are not built");
    if (first < 0 || nsteps < 0 || first + nsteps > c->rec_table_n) return fail(c, TRM_EINVAL, who + ": the launch leaves the record's position table");
    return TRM_OK;
}

// adjoint_backward<CKPT, R> (trm_launch_derivative.inl) with the record as the fifth kernel argument: the same preconditions, the same
// arguments, the same TRM_INFO_LAST_PROGRAM
template <bool CKPT, Ride R> int adjoint_backward_record(trm_ctx* c, double dt, int nsteps, int slot, int fold, int first) {
    const std::string who = ride_name(CKPT ? "k_column_adjoint_ckpt_record" : "k_column_adjoint_record", R, false);
    if (int rc = CKPT ? segment_range_ok(c, nsteps, slot, who) : tape_range_ok(c, nsteps, slot, who)) return rc;
    if (int rc = gradients_ok<R>(c, nsteps, who)) return rc;
    if (int rc = record_launch_ok(c, nsteps, first, who)) return rc;
    const LaunchArgs<double>& la = launch_args<double>(c);
    const ColumnArgs<double> a = column_args<double>(c, dt, 1, nsteps, PROG_EULER);
    SweepArgs<CKPT, R> aa;
    fill_cotangent(c, aa, slot, fold, ride_has_series(R));
    fill_gradients(c, aa);
    if constexpr (CKPT) {
        aa.first = 0;
        aa.every = 1;
    }
    const RecordArgs r = record_args(c, first);
    const int bits = PROGRAM_BACKWARD | (CKPT ? PROGRAM_CHECKPOINTED : 0) | (ride_has_bc(R) ? PROGRAM_BC_GRADIENT : 0) | (ride_has_params(R) ? (int)TRM_PROGRAM_PARAMETERS : 0);
    return by_instance(c, [&](auto h, auto lpc) {
        constexpr int H = decltype(h)::value, LPC = decltype(lpc)::value;
        if constexpr (CKPT)
            hipLaunchKernelGGL((k_column_adjoint_ckpt_record<H, LPC, R>), column_grid(c, LPC), dim3(TRM_STEP_BLOCK), (size_t)nsteps * TRM_STEP_BLOCK * sizeof(double),
                               c->stream, la.state, la.p, a, aa, r);
        else hipLaunchKernelGGL((k_column_adjoint_record<H, LPC, R>), column_grid(c, LPC), dim3(TRM_STEP_BLOCK), 0, c->stream, la.state, la.p, a, aa, r);
        TRM_HIP(c, hipGetLastError());
        c->last_program = derivative_program_id(TRM_PROGRAM_COLUMN_ADJOINT, H, LPC, aa.generic, bits);
        return (int)TRM_OK;
    });
}

}  // namespace trmh
