// Exercises the host-side preconditions of the derivative launches that carry a boundary series and the thermal parameters together
// (RIDE_PARAM_SERIES, trm_launch_derivative.inl) on contexts built by hand: no GPU call.  The union of the two rides' conditions, one
// kind of missing array at a time.  Built with the host sanitizers and run by `make -C terrarium.jl_amd/csrc check-preconditions`.
#include "trm_launch_derivative.inl"
#include <cassert>

namespace trmh {
static std::string last;
int fail(trm_ctx*, int code, const std::string& msg) { last = msg; return code; }
template <class NF> const LaunchArgs<NF>& launch_args(trm_ctx*) { static LaunchArgs<NF> a{}; return a; }
}  // namespace trmh
using namespace trmh;

int main() {
    static_assert(ride_has_params(RIDE_PARAM_SERIES) && ride_has_series(RIDE_PARAM_SERIES), "the union of both rides");
    static_assert(ride_has_params(RIDE_PARAM) && !ride_has_series(RIDE_PARAM) && !ride_has_params(RIDE_SERIES) && ride_has_series(RIDE_SERIES), "the rides as they were");
    static_assert(std::is_same<RideArgs<RIDE_PARAM_SERIES, int, int, int, int, AdjointParamSeriesArgs>, AdjointParamSeriesArgs>::value, "RideArgs selects the fifth");
    static_assert(std::is_same<RideArgs<RIDE_SERIES, int, int, int, AdjointSeriesArgs, char>, AdjointSeriesArgs>::value, "... and the fourth as before");
    trm_ctx c;
    c.Nh = 3; c.Nz = 4; c.Nzp = 4;
    c.tape_cap = 8;
    double x[4] = {};
    constexpr Ride R = RIDE_PARAM_SERIES;
    // a context that is complete for the ride: series table and rows, the branch-free kinds, one series on the top temperature with a
    // node accumulator and node seeds of its shape, the four boundary arrays of either family, the eight parameter accumulators
    c.d_series_table = x;
    c.d_series_rows = x;
    c.bc_kind[TRM_BCV_TEMPERATURE][TRM_TOP] = TRM_BC_VALUE;
    trm_ctx::Series sr;
    sr.is_bc = true; sr.var = TRM_BCV_TEMPERATURE; sr.side = TRM_TOP; sr.cap = 5;
    c.series.push_back(sr);
    c.d_adj_bcs[SLOT_T_TOP] = x; c.adj_bcs_nt[SLOT_T_TOP] = 5;
    c.d_tan_bcs[SLOT_T_TOP] = x; c.tan_bcs_nt[SLOT_T_TOP] = 5;
    for (auto& q : c.d_adj_bc) q = x;
    for (auto& q : c.d_tan_bc) q = x;
    for (auto& q : c.d_adj_param) q = x;
    assert(gradients_ok<R>(&c, 1, "g") == TRM_OK && tangent_seeds_ok<R>(&c, 1, "t") == TRM_OK);
    assert(gradients_ok<RIDE_SERIES>(&c, 1, "g") == TRM_OK && gradients_ok<RIDE_PARAM>(&c, 1, "g") == TRM_OK);

    // parameter accumulators missing while the series arrays are present: each of the eight in turn
    for (auto& q : c.d_adj_param) {
        q = nullptr;
        assert(gradients_ok<R>(&c, 1, "g") == TRM_EINVAL && last == "g: no accumulators");
        assert(gradients_ok<RIDE_SERIES>(&c, 1, "g") == TRM_OK);          // (the series ride does not ask for them)
        q = x;
    }
    // a boundary accumulator / seed array missing: named as the parameter rides name it
    c.d_adj_bc[2] = nullptr;
    assert(gradients_ok<R>(&c, 1, "g") == TRM_EINVAL && last == "g: no boundary accumulators");
    c.d_adj_bc[2] = x;
    c.d_tan_bc[1] = nullptr;
    assert(tangent_seeds_ok<R>(&c, 1, "t") == TRM_EINVAL && last == "t: no boundary seed arrays");
    assert(tangent_seeds_ok<RIDE_SERIES>(&c, 1, "t") == TRM_EINVAL && last == "t: no seed arrays");
    c.d_tan_bc[1] = x;
    // node accumulator / node seeds of the wrong shape, or missing, while the parameter arrays are present
    c.adj_bcs_nt[SLOT_T_TOP] = 4;
    assert(gradients_ok<R>(&c, 1, "g") == TRM_EINVAL && last == "g: a series without an accumulator of its shape");
    assert(gradients_ok<RIDE_PARAM>(&c, 1, "g") == TRM_OK);               // (the parameter ride does not ask for it)
    c.adj_bcs_nt[SLOT_T_TOP] = 5;
    c.d_adj_bcs[SLOT_T_TOP] = nullptr;
    assert(gradients_ok<R>(&c, 1, "g") == TRM_EINVAL && last == "g: a series without an accumulator of its shape");
    c.d_adj_bcs[SLOT_T_TOP] = x;
    c.tan_bcs_nt[SLOT_T_TOP] = 6;
    assert(tangent_seeds_ok<R>(&c, 1, "t") == TRM_EINVAL && last == "t: a series without seeds of its shape");
    c.tan_bcs_nt[SLOT_T_TOP] = 5;
    c.d_tan_bcs[SLOT_T_TOP] = nullptr;
    assert(tangent_seeds_ok<R>(&c, 1, "t") == TRM_EINVAL && last == "t: a series without seeds of its shape");
    c.d_tan_bcs[SLOT_T_TOP] = x;
    // series rows missing (a launch without steps reads none), the table missing
    c.d_series_rows = nullptr;
    assert(gradients_ok<R>(&c, 1, "g") == TRM_EINVAL && last == "g: no series rows, or the generic boundary kinds");
    assert(tangent_seeds_ok<R>(&c, 1, "t") == TRM_EINVAL && last == "t: no series rows, or the generic boundary kinds");
    assert(gradients_ok<R>(&c, 0, "g") == TRM_OK && tangent_seeds_ok<R>(&c, 0, "t") == TRM_OK);
    c.d_series_rows = x;
    c.d_series_table = nullptr;
    assert(gradients_ok<R>(&c, 0, "g") == TRM_EINVAL && tangent_seeds_ok<R>(&c, 0, "t") == TRM_EINVAL);
    c.d_series_table = x;
    // the generic boundary kinds (a Gradient on temperature off the branch-free kinds)
    c.bc_kind[TRM_BCV_TEMPERATURE][TRM_TOP] = TRM_BC_GRADIENT;
    assert(Policy<double>::generic_bcs(&c) && gradients_ok<R>(&c, 1, "g") == TRM_EINVAL && tangent_seeds_ok<R>(&c, 1, "t") == TRM_EINVAL);
    c.bc_kind[TRM_BCV_TEMPERATURE][TRM_TOP] = TRM_BC_VALUE;
    assert(gradients_ok<R>(&c, 1, "g") == TRM_OK && tangent_seeds_ok<R>(&c, 1, "t") == TRM_OK);
    // what the launch is called in a refusal
    assert(ride_name("k", R, true) == "k (series, parameter seeds)" && ride_name("k", R, false) == "k (series, parameter gradients)");
    assert(ride_name("k", RIDE_SERIES, true) == "k (series)" && ride_name("k", RIDE_PARAM, false) == "k (parameter gradients)");
    std::puts("derivative preconditions (parameters with a series) ok");
    return 0;
}
