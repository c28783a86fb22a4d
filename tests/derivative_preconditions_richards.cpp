// Exercises the host-side preconditions of the heat + Richards tangent launches (tangent_step_rich / tangent_closure_rich,
// trm_launch_derivative.inl; TRM_OPT_DERIVATIVE_RICHARDS) on contexts built by hand: no GPU call.  A Richards context only, the branch-free
// boundary kinds only, the five tangent fields present -- one missing condition at a time.  Built with the host sanitizers and run by
// `make -C terrarium.jl_amd/csrc check-preconditions`.
#include "trm_launch_derivative.inl"
#include <cassert>

namespace trmh {
static std::string last;
int fail(trm_ctx*, int code, const std::string& msg) { last = msg; return code; }
template <class NF> const LaunchArgs<NF>& launch_args(trm_ctx*) { static LaunchArgs<NF> a{}; return a; }
}  // namespace trmh
using namespace trmh;

int main() {
    static_assert(std::is_trivially_copyable<RichTangentArgs>::value && sizeof(RichTangentArgs) == 40, "a kernel argument: five pointers");
    static_assert(TRM_TANGENT_SATURATION == 3 && TRM_TANGENT_PRESSURE_HEAD == 4 && TRM_OPT_DERIVATIVE_RICHARDS == 16, "the public values");
    static_assert(TRM_PROGRAM_COLUMN_TANGENT_RICHARDS == 16 && TRM_ABI_VERSION == 20, "a new family in the low byte, the ABI version as it was");
    trm_ctx c;
    c.Nh = 3; c.Nz = 4; c.Nzp = 4;
    c.params.flow = TRM_FLOW_RICHARDS;
    double x[5][4] = {};
    for (int f = 0; f < 5; ++f) c.d_tan[f] = x[f];
    // a context that is complete for the launch
    assert(tangent_rich_ok(&c, "k") == TRM_OK);
    // the arguments name the five fields in the kernel's order: dU, dsat, dT, dliq, dpsi
    const RichTangentArgs ta = rich_tangent_args(&c);
    assert(ta.dU == x[TRM_TANGENT_INTERNAL_ENERGY] && ta.dsat == x[TRM_TANGENT_SATURATION] && ta.dT == x[TRM_TANGENT_TEMPERATURE] &&
           ta.dliq == x[TRM_TANGENT_LIQUID_WATER_FRACTION] && ta.dpsi == x[TRM_TANGENT_PRESSURE_HEAD]);
    // each of the five fields missing in turn (a tangent opened on a NoFlow context has three)
    for (auto& q : c.d_tan) {
        double* const kept = q;
        q = nullptr;
        assert(tangent_rich_ok(&c, "k") == TRM_EINVAL && last == "k: no tangent fields");
        q = kept;
    }
    // a NoFlow context
    c.params.flow = TRM_FLOW_NOFLOW;
    assert(tangent_rich_ok(&c, "k") == TRM_EINVAL && last == "k: a Richards context only");
    c.params.flow = TRM_FLOW_RICHARDS;
    // the generic boundary kinds: a Value or a Gradient on saturation, liquid fraction or pressure head, a Gradient on temperature, the
    // per-cell vwc_forcing field
    for (int var : {TRM_BCV_SATURATION_WATER_ICE, TRM_BCV_LIQUID_WATER_FRACTION, TRM_BCV_PRESSURE_HEAD})
        for (int side : {TRM_BOTTOM, TRM_TOP})
            for (int kind : {TRM_BC_VALUE, TRM_BC_GRADIENT}) {
                c.bc_kind[var][side] = kind;
                assert(Policy<double>::generic_bcs(&c) && tangent_rich_ok(&c, "k") == TRM_EINVAL && last == "k: the generic boundary kinds");
                c.bc_kind[var][side] = TRM_BC_NOFLUX;
            }
    c.bc_kind[TRM_BCV_TEMPERATURE][TRM_TOP] = TRM_BC_GRADIENT;
    assert(tangent_rich_ok(&c, "k") == TRM_EINVAL && last == "k: the generic boundary kinds");
    c.bc_kind[TRM_BCV_TEMPERATURE][TRM_TOP] = TRM_BC_VALUE;
    c.opt_vwc_field = 1;
    assert(tangent_rich_ok(&c, "k") == TRM_EINVAL && last == "k: the generic boundary kinds");
    c.opt_vwc_field = 0;
    // the branch-free kinds: Value on temperature, Flux on the prognostics
    c.bc_kind[TRM_BCV_INTERNAL_ENERGY][TRM_BOTTOM] = TRM_BC_FLUX;
    c.bc_kind[TRM_BCV_SATURATION_WATER_ICE][TRM_TOP] = TRM_BC_FLUX;
    assert(!Policy<double>::generic_bcs(&c) && tangent_rich_ok(&c, "k") == TRM_OK);
    std::puts("derivative preconditions (heat + Richards tangent) ok");
    return 0;
}
