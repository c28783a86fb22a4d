// Exercises the host-side preconditions of the heat + Richards sweep that carries the hydraulic-parameter gradients
// (adjoint_backward_rich<true, false> / adjoint_rich_param_reduce, trm_launch_derivative.inl; TRM_OPT_DERIVATIVE_RICHARDS_PARAMS) on contexts
// built by hand: no GPU call.  What the sweep without them needs, then the seven per-cell accumulators and the per-column result -- one
// missing at a time -- the addresses the argument filler hands to the kernel, and the id rule of trm_adjoint_param_download /
// _device_ptr: exactly the seven TRM_HYDRAULIC_PARAM_* ids name a row.  Built with the host sanitizers and run by
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
    const auto sweep = adjoint_backward_rich<true, false>;      // PARAMS, no record
    static_assert(std::is_trivially_copyable<HydParamPtrs>::value && sizeof(HydParamPtrs) == 7 * sizeof(double*), "a kernel argument: seven accumulators");
    static_assert(TRM_OPT_DERIVATIVE_RICHARDS_PARAMS == 18 && TRM_HYDRAULIC_PARAM_COUNT == 7 && HP_COUNT == 7, "the public values");
    static_assert(TRM_HYDRAULIC_PARAM_K_SAT == TRM_THERMAL_PARAM_COUNT && TRM_HYDRAULIC_PARAM_IMPEDANCE == 16, "one id space with the thermal ids");
    static_assert(TRM_HYDRAULIC_PARAM_K_SAT + HP_THETA_RES == TRM_HYDRAULIC_PARAM_THETA_RES && TRM_HYDRAULIC_PARAM_K_SAT + HP_BC_PSI_S == TRM_HYDRAULIC_PARAM_BC_PSI_S &&
                      TRM_HYDRAULIC_PARAM_K_SAT + HP_BC_LAMBDA == TRM_HYDRAULIC_PARAM_BC_LAMBDA && TRM_HYDRAULIC_PARAM_K_SAT + HP_VG_ALPHA == TRM_HYDRAULIC_PARAM_VG_ALPHA &&
                      TRM_HYDRAULIC_PARAM_K_SAT + HP_VG_N == TRM_HYDRAULIC_PARAM_VG_N && TRM_HYDRAULIC_PARAM_K_SAT + HP_IMPEDANCE == TRM_HYDRAULIC_PARAM_IMPEDANCE,
                  "the kernel's order is the header's");
    static_assert(TRM_PROGRAM_COLUMN_ADJOINT_RICHARDS == 17 && TRM_ABI_VERSION == 20, "the family and the ABI version as they were");
    // the parameters an instance's hydraulics read
    static_assert(hyd_param_mask<HYD_BC_LINEAR>() == 0x0fu && hyd_param_mask<HYD_VG_N2>() == 0x73u && hyd_param_mask<HYD_GENERIC>() == 0x7fu, "a bit per HP_*");

    // ---- the id rule: the seven hydraulic ids name the rows 0 ... 6, every other number none
    for (int which = -3; which < 40; ++which) {
        const bool hydraulic = which >= TRM_HYDRAULIC_PARAM_K_SAT && which <= TRM_HYDRAULIC_PARAM_IMPEDANCE;
        assert(hyd_param_row(which) == (hydraulic ? which - TRM_HYDRAULIC_PARAM_K_SAT : -1));
    }
    for (int which = 0; which < TRM_THERMAL_PARAM_COUNT; ++which) assert(hyd_param_row(which) == -1);
    assert(hyd_param_row(TRM_HYDRAULIC_PARAM_K_SAT) == HP_K_SAT && hyd_param_row(TRM_HYDRAULIC_PARAM_VG_N) == HP_VG_N);
    assert(hyd_param_row(2147483647) == -1 && hyd_param_row(-2147483647 - 1 + TRM_HYDRAULIC_PARAM_K_SAT) == -1);

    // ---- the launcher's preconditions
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
    const std::string who = "k";
    // a context that is complete: the sweep's conditions and the accumulators'
    assert(adjoint_rich_ok(&c, 4, 0, who) == TRM_OK && hyd_params_ok(&c, who) == TRM_OK);
    // the arguments name the accumulators in the order of TRM_HYDRAULIC_PARAM_*
    const HydParamPtrs hp = hyd_param_ptrs(&c);
    for (int q = 0; q < HP_COUNT; ++q) assert(hp.g[q] == acc[q]);
    // each accumulator missing in turn, then the result
    for (auto& q : c.d_adj_hyd) {
        double* const kept = q;
        q = nullptr;
        assert(hyd_params_ok(&c, who) == TRM_EINVAL && last == "k: no accumulators");
        assert(adjoint_rich_param_reduce<>(&c) == TRM_EINVAL && last == "k_hyd_param_reduce: no accumulators");
        assert(sweep(&c, 60.0, 1, 0, 1) == TRM_EINVAL && last == "k_column_adjoint_rich (parameter gradients): no accumulators");
        q = kept;
    }
    c.d_adj_hyd_out = nullptr;
    assert(hyd_params_ok(&c, who) == TRM_EINVAL && last == "k: no accumulators");
    assert(adjoint_rich_param_reduce<>(&c) == TRM_EINVAL && last == "k_hyd_param_reduce: no accumulators");
    assert(sweep(&c, 60.0, 1, 0, 1) == TRM_EINVAL && last == "k_column_adjoint_rich (parameter gradients): no accumulators");
    c.d_adj_hyd_out = out;
    // the sweep's own conditions come first: the tape, the fields, the kind of context, the boundary kinds
    assert(sweep(&c, 60.0, CAP + 1, 0, 0) == TRM_EINVAL && last == "k_column_adjoint_rich (parameter gradients): the launch leaves the tape");
    assert(sweep(&c, 60.0, 3, 4, 0) == TRM_EINVAL && last == "k_column_adjoint_rich (parameter gradients): the launch leaves the tape");
    c.ckpt_interval = 4;
    assert(sweep(&c, 60.0, 1, 0, 1) == TRM_EINVAL && last == "k_column_adjoint_rich (parameter gradients): no per-step tape");
    c.ckpt_interval = 0;
    c.d_adj[TRM_ADJOINT_PRESSURE_HEAD] = nullptr;
    assert(sweep(&c, 60.0, 1, 0, 1) == TRM_EINVAL && last == "k_column_adjoint_rich (parameter gradients): no cotangent fields");
    c.d_adj[TRM_ADJOINT_PRESSURE_HEAD] = x[TRM_ADJOINT_PRESSURE_HEAD];
    c.params.flow = TRM_FLOW_NOFLOW;
    assert(sweep(&c, 60.0, 1, 0, 1) == TRM_EINVAL && last == "k_column_adjoint_rich (parameter gradients): a Richards context only");
    assert(adjoint_rich_param_reduce<>(&c) == TRM_EINVAL && last == "k_hyd_param_reduce: a Richards context only");
    c.params.flow = TRM_FLOW_RICHARDS;
    c.bc_kind[TRM_BCV_PRESSURE_HEAD][TRM_BOTTOM] = TRM_BC_VALUE;
    assert(sweep(&c, 60.0, 1, 0, 1) == TRM_EINVAL && last == "k_column_adjoint_rich (parameter gradients): the generic boundary kinds");
    c.bc_kind[TRM_BCV_PRESSURE_HEAD][TRM_BOTTOM] = TRM_BC_NOFLUX;
    assert(adjoint_rich_ok(&c, CAP, 0, who) == TRM_OK && hyd_params_ok(&c, who) == TRM_OK);
    std::puts("derivative preconditions (heat + Richards hydraulic-parameter gradients) ok");
    return 0;
}
