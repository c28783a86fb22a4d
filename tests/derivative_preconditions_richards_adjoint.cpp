// Exercises the host-side preconditions of the heat + Richards adjoint launches (adjoint_record_rich / adjoint_backward_rich,
// trm_launch_derivative.inl; TRM_OPT_DERIVATIVE_RICHARDS_ADJOINT) on contexts built by hand: no GPU call.  A Richards context only, the
// branch-free boundary kinds only, the five cotangent fields and a per-step tape present, the launch's slots inside the tape -- one
// missing condition at a time -- and the addresses the two argument fillers hand to the kernels.  Built with the host sanitizers and run
// by `make -C terrarium.jl_amd/csrc check-preconditions`.
#include "trm_launch_derivative.inl"
#include <cassert>

namespace trmh {
static std::string last;
int fail(trm_ctx*, int code, const std::string& msg) { last = msg; return code; }
template <class NF> const LaunchArgs<NF>& launch_args(trm_ctx*) { static LaunchArgs<NF> a{}; return a; }
}  // namespace trmh
using namespace trmh;

int main() {
    static_assert(std::is_trivially_copyable<RichTapeArgs>::value && sizeof(RichTapeArgs) == 16, "a kernel argument: the slot and its stride");
    static_assert(std::is_trivially_copyable<RichSweepArgs>::value && sizeof(RichSweepArgs) == 64, "a kernel argument: five fields, the tape, the stride, the fold flag");
    static_assert(TRM_ADJOINT_SATURATION == 3 && TRM_ADJOINT_PRESSURE_HEAD == 4 && TRM_OPT_DERIVATIVE_RICHARDS_ADJOINT == 17, "the public values");
    static_assert(TRM_ADJOINT_SATURATION == TRM_TANGENT_SATURATION && TRM_ADJOINT_PRESSURE_HEAD == TRM_TANGENT_PRESSURE_HEAD, "the tangent's ids");
    static_assert(TRM_PROGRAM_COLUMN_ADJOINT_RICHARDS == 17 && TRM_ABI_VERSION == 20, "a new family in the low byte, the ABI version as it was");
    trm_ctx c;
    c.Nh = 3; c.Nz = 4; c.Nzp = 4;
    c.params.flow = TRM_FLOW_RICHARDS;
    double x[5][12] = {};
    constexpr int CAP = 6;
    static double tape[CAP * 2 * 12] = {};
    for (int f = 0; f < 5; ++f) c.d_adj[f] = x[f];
    c.d_tape = tape;
    c.tape_cap = CAP;
    // a context that is complete for the launch: every block inside the tape, the empty launch of an empty tape included
    assert(adjoint_rich_ok(&c, 4, 0, "k") == TRM_OK && adjoint_rich_ok(&c, 2, 4, "k") == TRM_OK && adjoint_rich_ok(&c, 0, 0, "k") == TRM_OK);
    assert(adjoint_rich_ok(&c, CAP, 0, "k") == TRM_OK && adjoint_rich_ok(&c, 0, CAP, "k") == TRM_OK);
    // a launch that leaves the tape, either way
    assert(adjoint_rich_ok(&c, CAP + 1, 0, "k") == TRM_EINVAL && last == "k: the launch leaves the tape");
    assert(adjoint_rich_ok(&c, 3, 4, "k") == TRM_EINVAL && last == "k: the launch leaves the tape");
    assert(adjoint_rich_ok(&c, 1, -1, "k") == TRM_EINVAL && adjoint_rich_ok(&c, -1, 0, "k") == TRM_EINVAL);
    // a slot is two fields: the record's first store and the sweep's newest slot are inside the allocation
    assert(rich_slot_elems(&c) == 12);
    const RichTapeArgs ra = rich_tape_args(&c, 4);
    assert(ra.tape == tape + 4 * 24 && ra.slot_elems == 12 && ra.tape + 2 * 2 * ra.slot_elems == tape + CAP * 24);
    // the arguments name the five fields in the kernel's order: lU, lsat, lT, lliq, lpsi
    const RichSweepArgs sa = rich_sweep_args(&c, 2, 1);
    assert(sa.lU == x[TRM_ADJOINT_INTERNAL_ENERGY] && sa.lsat == x[TRM_ADJOINT_SATURATION] && sa.lT == x[TRM_ADJOINT_TEMPERATURE] &&
           sa.lliq == x[TRM_ADJOINT_LIQUID_WATER_FRACTION] && sa.lpsi == x[TRM_ADJOINT_PRESSURE_HEAD]);
    assert(sa.tape == tape + 2 * 24 && sa.slot_elems == 12 && sa.fold == 1);
    // each of the five fields missing in turn (an adjoint opened on a NoFlow context has three)
    for (auto& q : c.d_adj) {
        double* const kept = q;
        q = nullptr;
        assert(adjoint_rich_ok(&c, 1, 0, "k") == TRM_EINVAL && last == "k: no cotangent fields");
        q = kept;
    }
    // no tape, or the checkpointed one
    c.d_tape = nullptr;
    assert(adjoint_rich_ok(&c, 1, 0, "k") == TRM_EINVAL && last == "k: no per-step tape");
    c.d_tape = tape;
    c.ckpt_interval = 4;
    assert(adjoint_rich_ok(&c, 1, 0, "k") == TRM_EINVAL && last == "k: no per-step tape");
    c.ckpt_interval = 0;
    // a NoFlow context
    c.params.flow = TRM_FLOW_NOFLOW;
    assert(adjoint_rich_ok(&c, 1, 0, "k") == TRM_EINVAL && last == "k: a Richards context only");
    c.params.flow = TRM_FLOW_RICHARDS;
    // the generic boundary kinds
    for (int var : {TRM_BCV_SATURATION_WATER_ICE, TRM_BCV_LIQUID_WATER_FRACTION, TRM_BCV_PRESSURE_HEAD})
        for (int side : {TRM_BOTTOM, TRM_TOP})
            for (int kind : {TRM_BC_VALUE, TRM_BC_GRADIENT}) {
                c.bc_kind[var][side] = kind;
                assert(Policy<double>::generic_bcs(&c) && adjoint_rich_ok(&c, 1, 0, "k") == TRM_EINVAL && last == "k: the generic boundary kinds");
                c.bc_kind[var][side] = TRM_BC_NOFLUX;
            }
    c.bc_kind[TRM_BCV_TEMPERATURE][TRM_TOP] = TRM_BC_GRADIENT;
    assert(adjoint_rich_ok(&c, 1, 0, "k") == TRM_EINVAL && last == "k: the generic boundary kinds");
    c.bc_kind[TRM_BCV_TEMPERATURE][TRM_TOP] = TRM_BC_VALUE;
    c.opt_vwc_field = 1;
    assert(adjoint_rich_ok(&c, 1, 0, "k") == TRM_EINVAL && last == "k: the generic boundary kinds");
    c.opt_vwc_field = 0;
    // the branch-free kinds: Value on temperature, Flux on the prognostics
    c.bc_kind[TRM_BCV_INTERNAL_ENERGY][TRM_BOTTOM] = TRM_BC_FLUX;
    c.bc_kind[TRM_BCV_SATURATION_WATER_ICE][TRM_TOP] = TRM_BC_FLUX;
    assert(!Policy<double>::generic_bcs(&c) && adjoint_rich_ok(&c, 4, 0, "k") == TRM_OK);
    std::puts("derivative preconditions (heat + Richards adjoint) ok");
    return 0;
}
