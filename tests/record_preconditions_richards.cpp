// Exercises the host-side preconditions of the heat + Richards sweeps that read an attached soil-moisture record
// (adjoint_backward_rich<false, true> and <true, true>, trm_launch_derivative.inl; TRM_OPT_DERIVATIVE_RICHARDS_RECORD) on
// contexts built by hand: no GPU call.  What the sweeps without a record need, then the record's: no record, missing tables, a position
// behind the tape, a launch that leaves the position table; the addresses the argument filler hands to the kernel; and the option gate
// of richards_tape_only (trm_host.hpp): the seven record calls pass under both options alone, every other call stays refused.  Built with
// the host sanitizers and run by `make -C terrarium.jl_amd/csrc check-preconditions`.
#include "trm_launch_derivative.inl"
#include <cassert>

namespace trmh {
static std::string last;
int fail(trm_ctx*, int code, const std::string& msg) { last = msg; return code; }
template <class NF> const LaunchArgs<NF>& launch_args(trm_ctx*) { static LaunchArgs<NF> a{}; return a; }
}  // namespace trmh
using namespace trmh;

int main() {
    const auto sweep = adjoint_backward_rich<false, true>, sweep_hyd = adjoint_backward_rich<true, true>;      // RECORD, and PARAMS with it
    static_assert(TRM_OPT_DERIVATIVE_RICHARDS_RECORD == 19 && TRM_OPT_DERIVATIVE_RICHARDS_PARAMS == 18 && TRM_OPT_DERIVATIVE_RICHARDS_ADJOINT == 17, "the public values");
    static_assert(TRM_PROGRAM_COLUMN_ADJOINT_RICHARDS == 17 && TRM_ABI_VERSION == 20, "the family and the ABI version as they were");
    static_assert(std::is_trivially_copyable<RecordArgs>::value, "a kernel argument");

    // ---- the option gate
    const char* kText = "trm_adjoint_record_detach: on a Richards context: final-state cotangents on a per-step tape only";
    for (int flow : {TRM_FLOW_NOFLOW, TRM_FLOW_RICHARDS})
        for (int adjoint = 0; adjoint < 2; ++adjoint)
            for (int record = 0; record < 2; ++record)
                for (int params = 0; params < 2; ++params) {
                    trm_ctx g;
                    g.params.flow = flow;
                    g.opt_derivative_richards_adjoint = adjoint;
                    g.opt_derivative_richards_record = record;
                    g.opt_derivative_richards_params = params;
                    const bool refused = flow == TRM_FLOW_RICHARDS && adjoint;
                    assert(richards_record_enabled(&g) == (refused && record));
                    // a call the Richards adjoint does not cover: whatever the new option says
                    last.clear();
                    assert(richards_tape_only(&g, "trm_adjoint_record_detach") == (refused ? TRM_EUNSUPPORTED : TRM_OK));
                    assert(!refused || last == kText);
                    // one of the seven record calls: let through under both options alone, the text today's otherwise
                    last.clear();
                    assert(richards_tape_only(&g, "trm_adjoint_record_detach", true) == (refused && !record ? TRM_EUNSUPPORTED : TRM_OK));
                    assert(!(refused && !record) || last == kText);
                }

    // ---- the launchers' preconditions: Nz = 4, Nh = 3, a tape of six steps
    trm_ctx c;
    c.Nh = 3; c.Nz = 4; c.Nzp = 4;
    c.params.flow = TRM_FLOW_RICHARDS;
    double x[5][12] = {};
    static double acc[HP_COUNT][12] = {};
    static double out[HP_COUNT * 3] = {};
    constexpr int CAP = 6;
    static double tape[CAP * 2 * 12] = {};
    for (int f = 0; f < 5; ++f) c.d_adj[f] = x[f];
    for (int q = 0; q < HP_COUNT; ++q) c.d_adj_hyd[q] = acc[q];
    c.d_adj_hyd_out = out;
    c.d_tape = tape;
    c.tape_cap = CAP;
    const std::string plain = "k_column_adjoint_rich_record", hyd = "k_column_adjoint_rich_record (parameter gradients)";
    const std::string none = ": no record is attached, or its tables are not built";
    auto both_refuse = [&](int nsteps, int slot, int fold, const std::string& why) {
        assert(sweep(&c, 60.0, nsteps, slot, fold) == TRM_EINVAL && last == plain + why);
        assert(sweep_hyd(&c, 60.0, nsteps, slot, fold) == TRM_EINVAL && last == hyd + why);
    };
    // no record
    assert(adjoint_rich_ok(&c, 4, 2, plain) == TRM_OK && hyd_params_ok(&c, hyd) == TRM_OK);
    both_refuse(4, 2, 1, none);
    // attached, nothing built yet: the lists alone
    const int32_t positions[4] = {0, 3, 5, 6}, levels[2] = {0, 3};
    static double observed[4 * 2 * 3] = {}, residual[4 * 2 * 3 + 3] = {};
    record_table_attach(c.rec, 4, positions, 2, levels);
    both_refuse(4, 2, 1, none);
    c.d_rec_observed = observed;
    c.d_rec_out = residual;
    both_refuse(4, 2, 1, none);                              // (missing tables)
    // the tables of a tape of six steps; the device copy is stood in for by a host copy, so every read below is one the sanitizer sees
    assert(record_fits_tape(&c, 6, "trm_adjoint_backward") == TRM_OK);
    record_table_build(c.rec, c.Nz, 6);
    std::vector<int32_t> device = c.rec.host;
    device.resize((device.size() + 1) / 2 * 2);
    c.rec.d_tables = (double*)device.data();
    assert(record_launch_ok(&c, 4, 2, plain) == TRM_OK && record_launch_ok(&c, 2, 0, plain) == TRM_OK && record_launch_ok(&c, 0, 6, plain) == TRM_OK);
    // what the kernel gets for the launch of the steps 2 ... 5: its step s is position 2 + s, the fold's position its entry 4
    const RecordArgs r = record_args(&c, 2);
    assert(r.row_of_level[0] == 0 && r.row_of_level[1] == -1 && r.row_of_level[3] == 1 && r.nlevels == 2);
    assert(r.row_of_position[0] == -1 && r.row_of_position[1] == 1 && r.row_of_position[2] == -1 && r.row_of_position[3] == 2 && r.row_of_position[4] == 3);
    assert(record_args(&c, 0).row_of_position[0] == 0 && r.observed == observed && r.weight == nullptr && r.residual == residual);
    // a launch that leaves the position table, either way
    both_refuse(5, 2, 1, ": the launch leaves the tape");   // (the sweep's own conditions come first)
    both_refuse(1, 6, 1, ": the launch leaves the tape");
    c.tape_cap = 8;
    both_refuse(5, 2, 1, ": the launch leaves the record's position table");
    both_refuse(1, 6, 1, ": the launch leaves the record's position table");
    c.tape_cap = CAP;
    // a position behind the tape: refused by the sweep before anything is launched, and tables of a shorter tape do not cover the launch
    assert(record_fits_tape(&c, 5, "trm_adjoint_backward") == TRM_EINVAL && last == "trm_adjoint_backward: the attached record is longer than the tape: position 6 of 5 taped steps");
    c.rec.d_tables = nullptr;
    record_table_build(c.rec, c.Nz, 5);
    std::vector<int32_t> shorter = c.rec.host;
    shorter.resize((shorter.size() + 1) / 2 * 2);
    c.rec.d_tables = (double*)shorter.data();
    both_refuse(2, 4, 1, ": the launch leaves the record's position table");
    assert(record_launch_ok(&c, 1, 4, plain) == TRM_OK);
    // the sweep's own conditions come first, then the accumulators, then the record
    c.ckpt_interval = 4;
    both_refuse(1, 0, 0, ": no per-step tape");
    c.ckpt_interval = 0;
    c.d_adj[TRM_ADJOINT_SATURATION] = nullptr;
    both_refuse(1, 0, 0, ": no cotangent fields");
    c.d_adj[TRM_ADJOINT_SATURATION] = x[TRM_ADJOINT_SATURATION];
    c.params.flow = TRM_FLOW_NOFLOW;
    both_refuse(1, 0, 0, ": a Richards context only");
    c.params.flow = TRM_FLOW_RICHARDS;
    c.d_adj_hyd_out = nullptr;
    assert(sweep_hyd(&c, 60.0, 1, 0, 0) == TRM_EINVAL && last == hyd + ": no accumulators");
    c.d_adj_hyd_out = out;
    c.d_rec_out = nullptr;
    both_refuse(1, 0, 0, none);
    c.d_rec_out = residual;
    assert(adjoint_rich_ok(&c, 1, 0, plain) == TRM_OK && hyd_params_ok(&c, hyd) == TRM_OK && record_launch_ok(&c, 1, 0, plain) == TRM_OK);
    c.rec.d_tables = nullptr;
    std::puts("record preconditions (heat + Richards soil-moisture records) ok");
    return 0;
}
