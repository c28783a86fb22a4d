// trm_launch_tangent_record.inl -- the launches of k_column_tangent_record (trm_column_tangent_record.hpp): tangent_step<R> of
// trm_launch_derivative.inl with a tangent record attached to the open tangent (trm_tangent_record_attach; DESIGN 4.7 "Tangent records").
// Included by the trm_launch_column_tangent_record*.hip files, each of which instantiates the launcher of one ride.
#include "trm_launch_derivative.inl"
#include "trm_column_tangent_record.hpp"

namespace trmh {

// the record as a launch whose first state is position `start` of the record's count sees it
inline TangentRecordArgs tangent_record_args(const trm_ctx* c, long long start) {
    TangentRecordArgs r;
    const int32_t* tables = (const int32_t*)c->d_trec_tables;
    r.row_of_level = tables;
    r.row_of_position = tables + c->Nz + start;
    r.T = c->d_trec[TRM_TANGENT_RECORD_TEMPERATURE];
    r.dT = c->d_trec[TRM_TANGENT_RECORD_TANGENT];
    r.nlevels = c->trec_nlevels;
    r.sample_entry = start == 0 ? 1 : 0;
    return r;
}
// the tables and the sample arrays are those of the attached record, and the launch's positions start ... start + nsteps are inside the
// position table (the caller clips a launch to it: tangent_record_steps)
inline int tangent_record_launch_ok(trm_ctx* c, int nsteps, const std::string& who) {
    if (c->trec_npos < 1 || c->trec_nlevels < 1 || c->trec_positions.empty() || !c->d_trec_tables || !c->d_trec[0] || !c->d_trec[1])
        return fail(c, TRM_EINVAL, who + ": no record is attached, or its tables are not built");
    if ((int)c->trec_positions.size() != c->trec_npos || (int)c->trec_levels.size() != c->trec_nlevels || c->trec_nlevels > c->Nz)
        return fail(c, TRM_EINVAL, who + ": the sample arrays do not have the attached shape");
    if (c->trec_position < 0 || nsteps < 0 || c->trec_position + nsteps > (long long)tangent_record_limit(c->trec_positions))
        return fail(c, TRM_EINVAL, who + ": the launch leaves the record's position table");
    return TRM_OK;
}

// tangent_step<R> with the record as the fifth kernel argument: the same preconditions, the same arguments, the same TRM_INFO_LAST_PROGRAM
template <Ride R> int tangent_record_step(trm_ctx* c, double dt, int nsteps) {
    const std::string who = ride_name("k_column_tangent_record", R, true);
    if (int rc = tangent_seeds_ok<R>(c, nsteps, who)) return rc;
    if (int rc = tangent_record_launch_ok(c, nsteps, who)) return rc;
    const LaunchArgs<double>& la = launch_args<double>(c);
    const ColumnArgs<double> a = column_args<double>(c, dt, 1, nsteps, PROG_EULER);
    TangentArgs<R> ta;
    fill_tangent(c, ta, ride_has_series(R));
    fill_tangent_seeds(c, ta);
    const TangentRecordArgs r = tangent_record_args(c, c->trec_position);
    return by_instance(c, [&](auto h, auto lpc) {
        constexpr int H = decltype(h)::value, LPC = decltype(lpc)::value;
        hipLaunchKernelGGL((k_column_tangent_record<H, LPC, R>), column_grid(c, LPC), dim3(TRM_STEP_BLOCK), 0, c->stream, la.state, la.p, a, ta, r);
        TRM_HIP(c, hipGetLastError());
        c->last_program = derivative_program_id(TRM_PROGRAM_COLUMN_TANGENT, H, LPC, ta.generic,
                                                (ride_has_bc(R) ? PROGRAM_BC_SEEDS : 0) | (ride_has_params(R) ? (int)TRM_PROGRAM_PARAMETERS : 0));
        return (int)TRM_OK;
    });
}

}  // namespace trmh
