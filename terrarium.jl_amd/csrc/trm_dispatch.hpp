// trm_dispatch.hpp -- from the run-time values of a decided launch to the template arguments of its kernel instance.  Every list of
// values that have instances is written here once; the launch files (trm_launch_*) nest these helpers around a generic lambda and
// prune the combinations without an instance with `if constexpr` inside it.  A value outside a list reaches NO instance: the helper
// returns false and the launcher refuses.  Plain C++17, no HIP call (tests/launch_dispatch.cpp).
#pragma once
#include "../../include/terrarium_hip.h"
#include "trm_kernels.hpp"

#include <cstddef>
#include <type_traits>
#include <utility>

namespace trmh {
using namespace trm;

// calls f(std::integral_constant<int, V>{}) for the V of the (distinct) Vs that equals v; returns whether one did.  f returns nothing: a
// launcher's callbacks assign its return code, which starts as NO_INSTANCE (trm_host.hpp)
template <int... Vs, class F> bool by_value(int v, F&& f) {
    return ((v == Vs && (f(std::integral_constant<int, Vs>{}), true)) || ...);
}
// the hydraulics (Policy::hyd): the two compiled ones and the one with run-time exponents; or the compiled ones alone
template <class F> bool by_hyd(int hyd, F&& f) { return by_value<HYD_BC_LINEAR, HYD_VG_N2, HYD_GENERIC>(hyd, f); }
template <class F> bool by_compiled_hyd(int hyd, F&& f) { return by_value<HYD_BC_LINEAR, HYD_VG_N2>(hyd, f); }
// lanes per column of the lane = level kernels: 32 up to 32 levels, else 64
constexpr int lanes_per_column(int nz) { return nz > 32 ? 64 : 32; }
template <class F> bool by_lanes(int nz, F&& f) { return by_value<32, 64>(lanes_per_column(nz), f); }
// a flag (the flow scheme, seb, series, generic, top_arrays, heun): f(std::true_type{}) or f(std::false_type{})
template <class F> bool by_bool(bool b, F&& f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
    return true;
}
// the number format of a context (trm_ctx::precision): f(NumberFormat<double>{}) or f(NumberFormat<float>{}); returns what f returns.
// The one place the host code asks for the precision of a context; f runs after the test, so its arguments are evaluated as a ternary's
template <class T> struct NumberFormat { using type = T; };
template <class F> auto by_precision(int precision, F&& f) { return precision == TRM_F64 ? f(NumberFormat<double>{}) : f(NumberFormat<float>{}); }
// what rides along with a derivative launch (Ride, trm_kernels.hpp): f(std::integral_constant<Ride, R>{}) for the ride that equals r
template <Ride... Rs, class F> bool by_ride_value(int r, F&& f) {
    return ((r == Rs && (f(std::integral_constant<Ride, Rs>{}), true)) || ...);
}
template <class F> bool by_ride(int r, F&& f) { return by_ride_value<RIDE_NONE, RIDE_BC, RIDE_PARAM, RIDE_SERIES, RIDE_PARAM_SERIES>(r, f); }
// (STAGED, SCALAR_IN) as Policy::io_paths leaves them: f(ST, SC) for (0, 1), (1, 0), (1, 1).  (0, 0) -- direct 2-lane stores AND vector
// loads of one address -- has no instance anywhere
template <class F> bool by_io(int staged, int scalar_in, F&& f) {
    if (staged && scalar_in) f(std::true_type{}, std::true_type{});
    else if (staged) f(std::true_type{}, std::false_type{});
    else if (scalar_in) f(std::false_type{}, std::true_type{});
    return staged || scalar_in;
}

// The boundary signatures (BCSIG, trm_kernels.hpp) with fp64 instances of k_column -- ForwardEuler (trm_launch_column_sig_*.hip) and
// Heun (trm_launch_column_sig_heun_*.hip) -- whether only under Richards, and whether k_column_psi has them too
// (trm_launch_column_psi_f64_*.hip)
struct SignatureEntry { int sig; bool richards_only, column_psi; };
constexpr SignatureEntry kSignatures[] = {
    {0, false, true},
    {BCSIG_T_TOP, false, true},
    {BCSIG_T_TOP | BCSIG_FU_BOT, false, true},
    {BCSIG_LAND, true, false},
    {BCSIG_T_TOP | BCSIG_FS_TOP, true, true},      // prescribed surface temperature + InfiltrationFlux (soil_model_bcs.jl:28)
};
constexpr std::size_t kSignatureCount = sizeof kSignatures / sizeof kSignatures[0];
constexpr bool signature_listed(int sig, bool rich, bool psi) {
    for (const SignatureEntry& e : kSignatures)
        if (e.sig == sig && (rich || !e.richards_only) && (!psi || e.column_psi)) return true;
    return false;
}
constexpr bool signature_has_instance(int sig, bool rich) { return signature_listed(sig, rich, false); }
constexpr bool column_psi_supported(int sig) { return signature_listed(sig, true, true); }
template <bool RICH, bool PSI, std::size_t... I, class F> bool by_signature_entries(int sig, F& f, std::index_sequence<I...>) {
    auto entry = [&](auto i) {
        constexpr SignatureEntry e = kSignatures[decltype(i)::value];
        if constexpr (signature_listed(e.sig, RICH, PSI))
            if (sig == e.sig) return f(std::integral_constant<int, e.sig>{}), true;
        return false;
    };
    return (entry(std::integral_constant<std::size_t, I>{}) || ...);
}
// f(std::integral_constant<int, SIG>{}) for the listed signature that equals sig and has an instance under the flow scheme
template <bool RICH, class F> bool by_signature(int sig, F&& f) { return by_signature_entries<RICH, false>(sig, f, std::make_index_sequence<kSignatureCount>{}); }
// ... and has a k_column_psi instance (fp64 Richards)
template <class F> bool by_psi_signature(int sig, F&& f) { return by_signature_entries<true, true>(sig, f, std::make_index_sequence<kSignatureCount>{}); }
// the signatures the packed fp32 step has instances of (Richards, DERIVE_LIQ: trm_launch_packed.hip)
template <class F> bool by_packed_signature(int sig, F&& f) { return by_value<BCSIG_LAND, BCSIG_T_TOP>(sig, f); }

}  // namespace trmh
