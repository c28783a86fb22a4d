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

// The kernel arguments of the derivative families are composed from parts by the ride (TangentArgs<R>, TapeArgs<STRIDED>, SweepArgs<CKPT, R>:
// trm_column_tangent.hpp, trm_column_adjoint.hpp).  A ride's struct holds exactly its parts ...
#define HAS_MEMBER(m)                                                     \
    template <class T, class = void> struct has_##m : std::false_type {}; \
    template <class T> struct has_##m<T, std::void_t<decltype(std::declval<T&>().m)>> : std::true_type {}
HAS_MEMBER(g); HAS_MEMBER(sg); HAS_MEMBER(pg); HAS_MEMBER(sTb); HAS_MEMBER(sn); HAS_MEMBER(s);
template <class T> constexpr int parts_of_sweep() { return has_g<T>::value | has_sg<T>::value << 1 | has_pg<T>::value << 2; }
template <class T> constexpr int parts_of_tangent() { return has_sTb<T>::value | has_sn<T>::value << 1 | has_s<T>::value << 2; }
// ... and every instance lies byte for byte as the hand-written struct it replaces lay: the sizes and offsets below were printed from
// the fifteen structs TangentArgs ... CheckpointParamSeriesArgs of the commit before the composition (a kernel reads its arguments by
// offset: fields, then bc, then series, then params)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winvalid-offsetof"
template <Ride R, size_t SIZE, size_t BC, size_t SERIES, size_t PARAMS> void check_tangent_layout() {
    using T = TangentArgs<R>;
    static_assert(offsetof(T, dU) == 0 && offsetof(T, dT) == 8 && offsetof(T, dliq) == 16 && offsetof(T, generic) == 24, "the fields");
    static_assert(parts_of_tangent<T>() == (ride_has_bc(R) | ride_has_series(R) << 1 | ride_has_params(R) << 2), "exactly the ride's parts");
    static_assert(std::is_trivially_copyable<T>::value, "a kernel argument");
    static_assert(sizeof(T) == SIZE, "the size the hand-written struct had");
    if constexpr (ride_has_bc(R)) static_assert(offsetof(T, sTb) == BC && offsetof(T, sTt) == BC + 8 && offsetof(T, sUb) == BC + 16 && offsetof(T, sUt) == BC + 24, "bc");
    if constexpr (ride_has_series(R)) static_assert(offsetof(T, sn) == SERIES, "series");
    if constexpr (ride_has_params(R)) static_assert(offsetof(T, s) == PARAMS, "params");
}
template <bool CKPT, Ride R, size_t SIZE, size_t BC, size_t SERIES, size_t PARAMS> void check_sweep_layout() {
    using T = SweepArgs<CKPT, R>;
    static_assert(offsetof(T, lU) == 0 && offsetof(T, lT) == 8 && offsetof(T, lliq) == 16 && offsetof(T, tape) == 24 && offsetof(T, slot_elems) == 32 &&
                      offsetof(T, generic) == 40 && offsetof(T, fold) == 44, "the tape");
    if constexpr (CKPT) static_assert(offsetof(T, first) == 48 && offsetof(T, every) == 52, "the strided tape");
    static_assert(parts_of_sweep<T>() == (ride_has_bc(R) | ride_has_series(R) << 1 | ride_has_params(R) << 2), "exactly the ride's parts");
    static_assert(std::is_trivially_copyable<T>::value, "a kernel argument");
    static_assert(sizeof(T) == SIZE, "the size the hand-written struct had");
    if constexpr (ride_has_bc(R)) static_assert(offsetof(T, g) == BC, "bc");
    if constexpr (ride_has_series(R)) static_assert(offsetof(T, sg) == SERIES, "series");
    if constexpr (ride_has_params(R)) static_assert(offsetof(T, pg) == PARAMS, "params");
}
static void check_argument_layouts() {
    // what was pinned on RideArgs: the fifth ride has all three parts, the fourth has two and is smaller by the parameter part
    static_assert(parts_of_sweep<SweepArgs<false, RIDE_PARAM_SERIES>>() == 7 && parts_of_sweep<SweepArgs<false, RIDE_SERIES>>() == 3, "g, sg, pg / g, sg");
    static_assert(sizeof(SweepArgs<false, RIDE_PARAM_SERIES>) - sizeof(SweepArgs<false, RIDE_SERIES>) == sizeof(ParamGradPtrs), "");
    static_assert(parts_of_tangent<TangentArgs<RIDE_PARAM_SERIES>>() == 7 && parts_of_tangent<TangentArgs<RIDE_SERIES>>() == 3, "sTb.., sn, s / sTb.., sn");
    static_assert(sizeof(TangentArgs<RIDE_PARAM_SERIES>) - sizeof(TangentArgs<RIDE_SERIES>) == sizeof(ParamSeeds), "");
    static_assert(sizeof(ParamSeeds) == 64 && sizeof(BcGradPtrs) == 32 && sizeof(SeriesGradPtrs) == 32 && sizeof(ParamGradPtrs) == 64, "the parts");
    // (size, offset of the bc part, of the series part, of the parameter part; 0: the ride has none)
    check_tangent_layout<RIDE_NONE, 32, 0, 0, 0>();
    check_tangent_layout<RIDE_BC, 64, 32, 0, 0>();
    check_tangent_layout<RIDE_PARAM, 128, 32, 0, 64>();
    check_tangent_layout<RIDE_SERIES, 96, 32, 64, 0>();
    check_tangent_layout<RIDE_PARAM_SERIES, 160, 32, 64, 96>();
    static_assert(sizeof(TapeArgs<false>) == 48 && sizeof(TapeArgs<true>) == 56 && offsetof(TapeArgs<true>, first) == 48 && offsetof(TapeArgs<true>, every) == 52, "the records'");
    static_assert(offsetof(TapeArgs<false>, fold) == 44 && offsetof(TapeArgs<true>, fold) == 44, "");
    check_sweep_layout<false, RIDE_NONE, 48, 0, 0, 0>();
    check_sweep_layout<false, RIDE_BC, 80, 48, 0, 0>();
    check_sweep_layout<false, RIDE_PARAM, 144, 48, 0, 80>();
    check_sweep_layout<false, RIDE_SERIES, 112, 48, 80, 0>();
    check_sweep_layout<false, RIDE_PARAM_SERIES, 176, 48, 80, 112>();
    check_sweep_layout<true, RIDE_NONE, 56, 0, 0, 0>();
    check_sweep_layout<true, RIDE_BC, 88, 56, 0, 0>();
    check_sweep_layout<true, RIDE_PARAM, 152, 56, 0, 88>();
    check_sweep_layout<true, RIDE_SERIES, 120, 56, 88, 0>();
    check_sweep_layout<true, RIDE_PARAM_SERIES, 184, 56, 88, 120>();
}
#pragma clang diagnostic pop

int main() {
    static_assert(ride_has_params(RIDE_PARAM_SERIES) && ride_has_series(RIDE_PARAM_SERIES), "the union of both rides");
    static_assert(ride_has_params(RIDE_PARAM) && !ride_has_series(RIDE_PARAM) && !ride_has_params(RIDE_SERIES) && ride_has_series(RIDE_SERIES), "the rides as they were");
    check_argument_layouts();
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
