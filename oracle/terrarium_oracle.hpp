// oracle/terrarium_oracle.hpp
//
// TEST INFRASTRUCTURE -- NOT PRODUCT CODE.
//
// CPU restatement of the Terrarium.jl SoilModel / LandModel(vegetation = nothing)
// explicit time-step path, written from the reference's Julia sources (read as
// text; Julia is not installed in the build image so the reference cannot be
// run).  It exists only so that tests/, __graft_entry__.smoke() and the
// cpu_baseline leg of bench.py can check and time-compare the HIP library.
// Nothing under terrarium.jl_amd/ may include, link or call this file.
//
// PARITY PINNING: the reference's own known-answer tests K1..K18 (SURVEY.md
// section 8c) are re-run against this restatement in tests/test_oracle_*.py.
// Three pieces of third-party arithmetic are NOT on disk and are restated from
// their published algorithms (see DESIGN.md "parity unpinned" list):
//   * Oceananigans.jl 0.100-0.106: z operators, halo filling, compute_z_bcs!
//   * FreezeCurves.jl 0.9: BrooksCorey / VanGenuchten SWRC and inverses
//   * Julia Base: min/max, x^n (compensated power by squaring), false*x
//
// THREE INSTANCES: Oracle<double> and Oracle<float> are the Float64 and Float32 models in their own arithmetic (what the
// device is compared with); Oracle<long double, double> and Oracle<long double, float> are the same two models evaluated
// in long double -- the measure of how much either loses to rounding (tests/accuracy.py).  See model_literal below.
//
// Layout mirrors the reference Field storage: one plane per z level, x fastest,
// one halo level below (k = 0) and above (k = Nz+1); k = 1 is the BOTTOM cell
// and k = Nz the surface cell (src/grids/column_grid.jl:31).  The driver runs
// one pass per reference kernel in the reference's order
// (src/timesteppers/forward_euler.jl:19-31, src/state_variables.jl:72-80).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>
#include <algorithm>

#ifdef _OPENMP
#define TRM_OMP_FOR _Pragma("omp parallel for schedule(static)")
#define TRM_OMP_FOR2 _Pragma("omp parallel for collapse(2) schedule(static)")
#else
#define TRM_OMP_FOR
#define TRM_OMP_FOR2
#endif

namespace trm_oracle {

// Field storage of the timing leg (bench.py cpu_baseline).  std::vector writes every element from the constructing thread, so
// on a multi-socket host all pages of all fields would sit on ONE NUMA node and the OpenMP passes would stream remotely.
// FieldVec sizes without writing; Oracle's constructor then first-touches every array inside an `omp parallel for
// schedule(static)` over the columns -- the decomposition of every compute pass -- so a thread's columns live on its node.
template <class T> struct NoInitAlloc : std::allocator<T> {
    template <class U> struct rebind { using other = NoInitAlloc<U>; };
    template <class U, class... A> void construct(U* q, A&&... a) {
        if constexpr (sizeof...(A) == 0) ::new ((void*)q) U;      // default-init: no write
        else ::new ((void*)q) U(std::forward<A>(a)...);
    }
};
template <class NF> using FieldVec = std::vector<NF, NoInitAlloc<NF>>;

// ---------------------------------------------------------------------------
// Julia Base semantics used by the reference
// ---------------------------------------------------------------------------

// Base.min / Base.max for floats (NaN-propagating, signed-zero aware).
template <class NF> inline NF jl_min(NF x, NF y) {
    NF diff = x - y;
    NF arg = std::signbit(diff) ? x : y;
    return (std::isnan(x) || std::isnan(y)) ? diff : arg;
}
template <class NF> inline NF jl_max(NF x, NF y) {
    NF diff = x - y;
    NF arg = std::signbit(diff) ? y : x;
    return (std::isnan(x) || std::isnan(y)) ? diff : arg;
}
// Bool * Float: `false` is a strong zero that keeps the sign of x.
template <class NF> inline NF jl_boolmul(bool b, NF x) { return b ? x : std::copysign(NF(0), x); }

template <class NF> inline void two_mul(NF a, NF b, NF& hi, NF& lo) {
    hi = a * b;
    lo = std::fma(a, b, -hi);
}
// Base.Math.pow_body(x::Float64, n::Integer): compensated power by squaring.
template <class NF> inline NF jl_pow_int(NF x, long n) {
    if (n == 0) return NF(1);
    NF y = NF(1), xnlo = NF(0), ynlo = NF(0);
    if (n == 3) return x * x * x;
    if (n < 0) {
        NF rx = NF(1) / x;
        if (n == -2) return rx * rx;
        if (std::isfinite(x)) xnlo = -std::fma(x, rx, NF(-1)) * rx;
        x = rx;
        n = -n;
    }
    while (n > 1) {
        if (n & 1) {
            NF err = std::fma(y, xnlo, x * ynlo);
            NF hi, lo;
            two_mul(x, y, hi, lo);
            y = hi;
            ynlo = lo + err;
        }
        NF err = x * NF(2) * xnlo;
        NF hi, lo;
        two_mul(x, x, hi, lo);
        x = hi;
        xnlo = lo + err;
        n >>= 1;
    }
    NF err = std::fma(y, xnlo, x * ynlo);
    return (std::isfinite(x) && std::isfinite(err)) ? std::fma(x, y, err) : x * y;
}
// Base.:^(x::Float64, y::Float64): integer-valued exponents take the
// power-by-squaring path, everything else the generic pow.  (Float32 in Julia
// widens to Float64 for the generic path; std::pow on float is within the
// fp32 tolerance the tests use.)
template <class NF> inline NF jl_pow(NF x, NF y) {
    if (x == NF(1)) return NF(1);
    if (std::fabs(y) < NF(4.0e18)) {
        long long yi = (long long)y;
        if ((NF)yi == y) {
            if (yi == 0) return NF(1);
            if (yi >= -4096 && yi <= 24576) return jl_pow_int(x, (long)yi);
        }
    }
    return std::pow(x, y);
}

// ARITHMETIC TYPE AND MODEL PRECISION.  `NF` is the type every operation is carried out in; `MF` is the number format of
// the model being restated (Float32 or Float64 in the reference) and defaults to `NF`.  Whatever the reference takes from
// its number format rather than computes -- eps(NF) in safediv, the literals it converts to NF, the parameters, the grid
// coordinates and the inputs -- is part of the model and keeps MF's value when NF is wider: Oracle<long double, float> is
// the Float32 model evaluated without Float32's rounding, the yardstick of tests/accuracy.py.  With MF = NF every
// expression below is the one it was before MF existed (NF(NF(x)) == NF(x)).
template <class NF, class MF> inline NF model_literal(double x) { return NF(MF(x)); }

// src/utils/utils.jl:25 (eps(NF) is the model's)
template <class NF, class MF = NF> inline NF safediv(NF x, NF y) {
    return (y == NF(0)) ? std::numeric_limits<NF>::infinity() : x / (y + NF(std::numeric_limits<MF>::epsilon()));
}

// ---------------------------------------------------------------------------
// Parameters (defaults in Appendix A-0)
// ---------------------------------------------------------------------------
enum Flow { FLOW_NOFLOW = 0, FLOW_RICHARDS = 1 };
enum Swrc { SWRC_BROOKS_COREY = 0, SWRC_VAN_GENUCHTEN = 1 };
enum UnsatK { UNSATK_LINEAR = 0, UNSATK_VAN_GENUCHTEN = 1 };
enum HaloPolicy { HALO_REFERENCE_ZERO = 0, HALO_MIRROR = 1 };
enum BcKind { BC_NOFLUX = 0, BC_VALUE = 1, BC_FLUX = 2, BC_GRADIENT = 3 };
enum BcVar { BCV_INTERNAL_ENERGY = 0, BCV_SATURATION = 1, BCV_TEMPERATURE = 2, BCV_LIQUID_FRACTION = 3, BCV_PRESSURE_HEAD = 4, BCV_COUNT = 5 };

struct ParamsD {  // plain doubles + ints across the C API
    // physical_constants.jl:9-51
    double rho_w, rho_i, rho_a, c_a, Lsl, Llg, Lsg, g, Tref, sigma, kappa_vk, eps_mw, R_a;
    // soil_thermal_properties.jl:14-46
    double k_water, k_ice, k_air, k_mineral, k_organic;
    double c_water, c_ice, c_air, c_mineral, c_organic;
    // soil_porosity.jl:7-13, constant_soil_carbon.jl:10-16
    double por_mineral, por_organic, rho_soc, rho_org;
    // soil_hydraulic_properties.jl / FreezeCurves
    double K_sat, theta_res, bc_psi_s, bc_lambda, vg_alpha, vg_n, impedance, vwc_forcing;
    // surface energy balance
    double albedo, emissivity, kappa_s, C_h, min_windspeed, tau_r, beta_evap, field_capacity;
    int32_t flow, swrc, unsat_k, seb, halo_policy, prescribed_albedo, evap_resistance, reserved;
};

// the parameters as the model's number format holds them (convert(MF, x)); the identity for MF = double
template <class MF> inline ParamsD model_params(ParamsD d) {
    double* q = &d.rho_w;
    for (size_t n = 0; n < offsetof(ParamsD, flow) / sizeof(double); ++n) q[n] = (double)MF(q[n]);
    return d;
}

template <class NF> struct Params {
    NF rho_w, rho_i, rho_a, c_a, Lsl, Llg, Lsg, g, Tref, sigma, kappa_vk, eps_mw, R_a;
    NF k_water, k_ice, k_air, k_mineral, k_organic;
    NF c_water, c_ice, c_air, c_mineral, c_organic;
    NF por_mineral, por_organic, rho_soc, rho_org;
    NF K_sat, theta_res, bc_psi_s, bc_lambda, vg_alpha, vg_n, impedance, vwc_forcing;
    NF albedo, emissivity, kappa_s, C_h, min_windspeed, tau_r, beta_evap, field_capacity;
    int flow, swrc, unsat_k, seb, halo_policy, prescribed_albedo, evap_resistance;
    explicit Params(const ParamsD& d)
        : rho_w(NF(d.rho_w)), rho_i(NF(d.rho_i)), rho_a(NF(d.rho_a)), c_a(NF(d.c_a)), Lsl(NF(d.Lsl)), Llg(NF(d.Llg)),
          Lsg(NF(d.Lsg)), g(NF(d.g)), Tref(NF(d.Tref)), sigma(NF(d.sigma)), kappa_vk(NF(d.kappa_vk)),
          eps_mw(NF(d.eps_mw)), R_a(NF(d.R_a)), k_water(NF(d.k_water)), k_ice(NF(d.k_ice)), k_air(NF(d.k_air)),
          k_mineral(NF(d.k_mineral)), k_organic(NF(d.k_organic)), c_water(NF(d.c_water)), c_ice(NF(d.c_ice)),
          c_air(NF(d.c_air)), c_mineral(NF(d.c_mineral)), c_organic(NF(d.c_organic)), por_mineral(NF(d.por_mineral)),
          por_organic(NF(d.por_organic)), rho_soc(NF(d.rho_soc)), rho_org(NF(d.rho_org)), K_sat(NF(d.K_sat)),
          theta_res(NF(d.theta_res)), bc_psi_s(NF(d.bc_psi_s)), bc_lambda(NF(d.bc_lambda)), vg_alpha(NF(d.vg_alpha)),
          vg_n(NF(d.vg_n)), impedance(NF(d.impedance)), vwc_forcing(NF(d.vwc_forcing)), albedo(NF(d.albedo)),
          emissivity(NF(d.emissivity)), kappa_s(NF(d.kappa_s)), C_h(NF(d.C_h)), min_windspeed(NF(d.min_windspeed)),
          tau_r(NF(d.tau_r)), beta_evap(NF(d.beta_evap)), field_capacity(NF(d.field_capacity)), flow(d.flow), swrc(d.swrc), unsat_k(d.unsat_k), seb(d.seb),
          halo_policy(d.halo_policy), prescribed_albedo(d.prescribed_albedo), evap_resistance(d.evap_resistance) {}
};

// ---------------------------------------------------------------------------
// Scalar physics (Appendix A-1 .. A-5, A-9)
// ---------------------------------------------------------------------------

// homogeneous_strat.jl:34-44 organic_fraction
template <class NF> inline NF organic_fraction(const Params<NF>& p) {
    return p.rho_soc / ((NF(1) - p.por_organic) * p.rho_org);
}
// homogeneous_strat.jl:51-61 porosity
template <class NF> inline NF porosity(const Params<NF>& p) {
    NF org = organic_fraction(p);
    return (NF(1) - org) * p.por_mineral + org * p.por_organic;
}

template <class NF> struct Fractions { NF water, ice, air, organic, mineral; };

// soil_volume.jl:52-67, 103-107 volumetric_fractions; the constructor's
// @assert bounds (soil_volume.jl:26-28, 85) are reported through `viol`.
template <class NF>
inline Fractions<NF> volumetric_fractions(NF por, NF sat, NF liq, NF org, uint32_t* viol = nullptr) {
    if (viol) {
        bool ok = (NF(0) <= por && por <= NF(1)) && (NF(0) <= sat && sat <= NF(1)) && (NF(0) <= liq && liq <= NF(1)) &&
                  (NF(0) <= org && org <= NF(1));
        if (!ok) __atomic_fetch_or(viol, 2u, __ATOMIC_RELAXED);
    }
    Fractions<NF> f;
    NF water_ice = sat * por;
    f.water = water_ice * liq;
    f.ice = water_ice * (NF(1) - liq);
    f.air = (NF(1) - sat) * por;
    NF solid_frac = NF(1) - por;
    f.organic = solid_frac * org;
    f.mineral = solid_frac * (NF(1) - org);
    return f;
}

// soil_thermal_properties.jl:90-95,119-123 InverseQuadratic, constituent order
// of SoilThermalConductivities: water, ice, air, mineral, organic; left fold.
template <class NF> inline NF thermal_conductivity(const Params<NF>& p, const Fractions<NF>& f) {
    NF s = std::sqrt(p.k_water) * f.water;
    s = s + std::sqrt(p.k_ice) * f.ice;
    s = s + std::sqrt(p.k_air) * f.air;
    s = s + std::sqrt(p.k_mineral) * f.mineral;
    s = s + std::sqrt(p.k_organic) * f.organic;
    return s * s;
}
// soil_thermal_properties.jl:102-107 heat_capacity
template <class NF> inline NF heat_capacity(const Params<NF>& p, const Fractions<NF>& f) {
    NF s = p.c_water * f.water;
    s = s + p.c_ice * f.ice;
    s = s + p.c_air * f.air;
    s = s + p.c_mineral * f.mineral;
    s = s + p.c_organic * f.organic;
    return s;
}

// soil_energy_closures.jl:131-141 liquid_water_fraction(::FreeWater, U, Lθ, sat)
template <class NF, class MF = NF> inline NF liquid_water_fraction(NF U, NF Ltheta) {
    if (U >= NF(0)) return NF(1);
    return jl_boolmul(U >= -Ltheta, NF(1) - safediv<NF, MF>(U, -Ltheta));
}
// soil_energy_closures.jl:147-159 energy_to_temperature(::FreeWater, U, Lθ, C)
template <class NF> inline NF energy_to_temperature(NF U, NF Ltheta, NF C) {
    if (U < -Ltheta) return (U + Ltheta) / C;
    if (U >= NF(0)) return U / C;
    return NF(0);
}

// FreezeCurves.jl 0.9 (not on disk): theta(psi)
template <class NF> inline NF swrc_theta(const Params<NF>& p, NF psi, NF theta_sat) {
    NF theta_res = p.theta_res;
    if (p.swrc == SWRC_VAN_GENUCHTEN) {
        NF n = p.vg_n, m = NF(1) - NF(1) / n;
        if (psi <= NF(0)) return theta_res + (theta_sat - theta_res) * jl_pow(NF(1) + jl_pow(-p.vg_alpha * psi, n), -m);
        return theta_sat;
    }
    if (psi < -p.bc_psi_s) return theta_res + (theta_sat - theta_res) * jl_pow(-p.bc_psi_s / psi, p.bc_lambda);
    return theta_sat;
}
// inverse: psi(theta)
template <class NF> inline NF swrc_psi(const Params<NF>& p, NF theta, NF theta_sat) {
    NF theta_res = p.theta_res;
    if (p.swrc == SWRC_VAN_GENUCHTEN) {
        NF n = p.vg_n, m = NF(1) - NF(1) / n;
        if (theta < theta_sat) {
            NF r = (theta - theta_res) / (theta_sat - theta_res);
            return NF(-1) / p.vg_alpha * jl_pow(jl_pow(r, NF(-1) / m) - NF(1), NF(1) / n);
        }
        return NF(0);
    }
    if (theta < theta_sat) {
        NF r = (theta - theta_res) / (theta_sat - theta_res);
        return -p.bc_psi_s * jl_pow(r, NF(-1) / p.bc_lambda);
    }
    return -p.bc_psi_s;
}

// soil_hydraulic_properties.jl:170-181 (linear) and :203-221 (van Genuchten
// with ice impedance; evaluated in complex arithmetic by the reference so that
// illegal states give a finite magnitude -- inside 0<=x<=1 the complex
// evaluation is the real one, outside we return the complex magnitude).
template <class NF> inline NF hydraulic_conductivity_cell(const Params<NF>& p, NF por, NF liq, const Fractions<NF>& f) {
    if (p.unsat_k == UNSATK_LINEAR) {
        NF theta_sat = f.water + f.ice + f.air;
        return p.K_sat * f.water / theta_sat;
    }
    NF n = p.vg_n;
    NF x = f.water / por;
    NF I_ice = jl_pow(NF(10), -p.impedance * (NF(1) - liq));
    NF e1 = n / (n + NF(1)), e2 = (n - NF(1)) / n;
    if (x >= NF(0) && x <= NF(1)) {
        NF inner = NF(1) - jl_pow(x, e1);
        NF t = NF(1) - jl_pow(inner, e2);
        return std::fabs(p.K_sat * I_ice * std::sqrt(x) * (t * t));
    }
    // complex branch (illegal states only)
    typedef std::pair<double, double> cx;
    auto cpow = [](cx z, double e) {
        double r = std::hypot(z.first, z.second), th = std::atan2(z.second, z.first);
        double rp = std::pow(r, e);
        return cx(rp * std::cos(e * th), rp * std::sin(e * th));
    };
    auto cmul = [](cx a, cx b) { return cx(a.first * b.first - a.second * b.second, a.first * b.second + a.second * b.first); };
    cx zx((double)x, 0.0);
    cx a = cpow(zx, (double)e1);
    cx inner(1.0 - a.first, -a.second);
    cx b = cpow(inner, (double)e2);
    cx t(1.0 - b.first, -b.second);
    cx t2 = cmul(t, t);
    cx sq = cpow(zx, 0.5);
    cx r = cmul(cx((double)(p.K_sat * I_ice) * sq.first, (double)(p.K_sat * I_ice) * sq.second), t2);
    return (NF)std::hypot(r.first, r.second);
}

// physics_utils.jl:54,67-73 saturation_vapor_pressure (August-Roche-Magnus)
template <class NF, class MF = NF> inline NF saturation_vapor_pressure(NF T) {
    auto c = [](double x) { return model_literal<NF, MF>(x); };
    if (T <= NF(0)) return c(611.0) * std::exp(c(22.46) * T / (T + c(272.62)));
    return c(611.0) * std::exp(c(17.62) * T / (T + c(243.12)));
}
// physical_constants.jl:83-97 compute_vpd
template <class NF, class MF = NF> inline NF compute_vpd(const Params<NF>& p, NF pres, NF q_air, NF T) {
    NF e_sat = saturation_vapor_pressure<NF, MF>(T);
    NF e_air = q_air * pres / (p.eps_mw + (NF(1) - p.eps_mw) * q_air);
    return jl_max(e_sat - e_air, model_literal<NF, MF>(0.1));
}
// physical_constants.jl:68 stefan_boltzmann: ϵ * σ * T^4 (T^4 = pow_body(T, 4))
template <class NF> inline NF stefan_boltzmann(const Params<NF>& p, NF T, NF emis) {
    return emis * p.sigma * jl_pow_int(T, 4);
}

// direct_surface_runoff.jl:27-33 compute_surface_drainage
template <class NF> inline NF compute_surface_drainage(const Params<NF>& p, NF surface_excess_water) {
    NF S = jl_max(surface_excess_water, NF(0));
    return S / p.tau_r;
}
// direct_surface_runoff.jl:41-47 compute_infiltration: min(influx, max_infil) * is_unsaturated
template <class NF> inline NF compute_infiltration(NF influx, NF sat_top, NF max_infil) {
    bool is_unsaturated = sat_top < NF(1);
    return jl_boolmul(is_unsaturated, jl_min(influx, max_infil));
}
// direct_surface_runoff.jl:54-62 compute_surface_runoff: P + dS/dt - I
template <class NF> inline NF compute_surface_runoff(NF rain, NF surface_drainage, NF infil) {
    return rain + surface_drainage - infil;
}
// turbulent_fluxes.jl:36-50 compute_sensible_heat_flux(tur, Q_T, rho_a, c_a), compute_latent_heat_flux(tur, Q_h, rho_a, L)
template <class NF> inline NF sensible_heat_flux(const Params<NF>& p, NF Q_T) { return p.c_a * p.rho_a * Q_T; }
template <class NF> inline NF latent_heat_flux(const Params<NF>& p, NF Q_h) { return p.Llg * p.rho_a * Q_h; }
// skin_temperature.jl:62-68 compute_skin_temperature(skinT, Tg, G, dz)
template <class NF> inline NF compute_skin_temperature(const Params<NF>& p, NF Tg, NF G, NF dz) {
    return Tg - G * dz / (NF(2) * p.kappa_s);
}

// ---------------------------------------------------------------------------
// Column grid (column_grid.jl:20-34 + Oceananigans generate_coordinate)
// ---------------------------------------------------------------------------
template <class NF> struct Grid {
    long Nh = 0;
    int Nz = 0;
    NF dx = NF(1);
    std::vector<NF> zF;   // faces   0..Nz+2 (face k is the lower face of cell k; 0 and Nz+2 are halo faces)
    std::vector<NF> zC;   // centres 0..Nz+1
    std::vector<NF> dzc;  // Δzᵃᵃᶜ   0..Nz+1
    std::vector<NF> dzf;  // Δzᵃᵃᶠ   1..Nz+1 (index 0 unused)
    std::vector<NF> rdzc, rdzf;

    // `thickness` is get_spacing(vert) (vertical_discretization.jl:20): index 0
    // is the SURFACE layer.  dx <= 0 selects the ColumnGrid default x = (0, 1).
    // MF: the number format the coordinates are converted to (column_grid.jl:31 `convert.(NF, ...)`), NF by default
    template <class MF = NF> void build(long nh, int nz, const double* thickness, double dx_in) {
        Nh = nh;
        Nz = nz;
        // z_coords = convert.(NF, vcat(-reverse(cumsum(z_thick)), 0))   (column_grid.jl:31)
        std::vector<double> cs(nz);
        double s = thickness[0];
        cs[0] = s;
        for (int i = 1; i < nz; ++i) { s = s + thickness[i]; cs[i] = s; }
        zF.assign(nz + 3, NF(0));
        for (int k = 1; k <= nz; ++k) zF[k] = NF(MF(-cs[nz - k]));
        zF[nz + 1] = NF(0);
        // Bounded halo faces continue with the boundary cell's spacing
        NF dlo = zF[2] - zF[1], dhi = zF[nz + 1] - zF[nz];
        zF[0] = zF[1] - dlo;
        zF[nz + 2] = zF[nz + 1] + dhi;
        zC.assign(nz + 2, NF(0));
        for (int k = 0; k <= nz + 1; ++k) zC[k] = (zF[k + 1] + zF[k]) / NF(2);
        dzc.assign(nz + 2, NF(0));
        for (int k = 0; k <= nz + 1; ++k) dzc[k] = zF[k + 1] - zF[k];
        dzf.assign(nz + 2, NF(0));
        for (int k = 1; k <= nz + 1; ++k) dzf[k] = zC[k] - zC[k - 1];
        rdzc.assign(nz + 2, NF(0));
        rdzf.assign(nz + 2, NF(0));
        for (int k = 0; k <= nz + 1; ++k) rdzc[k] = NF(1) / dzc[k];
        for (int k = 1; k <= nz + 1; ++k) rdzf[k] = NF(1) / dzf[k];
        dx = dx_in > 0 ? NF(MF(dx_in)) : NF(MF(1.0 / (double)nh));
    }
};

// ---------------------------------------------------------------------------
// Field ids shared with the Python harness
// ---------------------------------------------------------------------------
enum FieldId {
    F_INTERNAL_ENERGY = 0, F_SATURATION = 1, F_TEMPERATURE = 2, F_LIQUID_FRACTION = 3, F_PRESSURE_HEAD = 4,
    F_HYDRAULIC_CONDUCTIVITY = 5,  // Face field: Nz+1 rows
    F_TEND_INTERNAL_ENERGY = 6, F_TEND_SATURATION = 7,
    // 2-D
    F_SURFACE_EXCESS_WATER = 8, F_TEND_SURFACE_EXCESS_WATER = 9, F_WATER_TABLE = 10, F_SKIN_TEMPERATURE = 11,
    F_GROUND_HEAT_FLUX = 12, F_SW_UP = 13, F_LW_UP = 14, F_NET_RADIATION = 15, F_SENSIBLE_HEAT_FLUX = 16,
    F_LATENT_HEAT_FLUX = 17, F_EVAPORATION_GROUND = 18, F_INFILTRATION = 19, F_SURFACE_RUNOFF = 20,
    // inputs (PrescribedAtmosphere)
    F_AIR_TEMPERATURE = 21, F_AIR_PRESSURE = 22, F_WINDSPEED = 23, F_SPECIFIC_HUMIDITY = 24, F_RAINFALL = 25,
    F_SW_DOWN = 26, F_LW_DOWN = 27,
    F_CARBON_VEGETATION = 31, F_TEND_VEGETATION_AREA_FRACTION = 34, F_NET_PRIMARY_PRODUCTION = 44, F_CO2 = 45,
    F_SOIL_MOISTURE_LIMITING_FACTOR = 46, F_DAILY_LEAF_RESPIRATION = 47, F_PLANT_AVAILABLE_WATER = 49, F_ROOT_FRACTION = 50,
    F_CANOPY_WATER = 51, F_TEND_CANOPY_WATER = 52, F_CANOPY_WATER_INTERCEPTION = 53, F_CANOPY_WATER_REMOVAL = 54,
    F_SATURATION_CANOPY_WATER = 55, F_RAINFALL_GROUND = 56, F_EVAPORATION_CANOPY = 57, F_TRANSPIRATION = 58, F_STEM_AREA_INDEX = 59,
    F_VWC_FORCING = 28, F_ALBEDO = 29, F_EMISSIVITY = 30,  // user vwc_forcing evaluated per cell (soil_hydrology.jl:37-38, forcings.jl:13-15)
    F_COUNT = 29
};

template <class NF> struct Bc {
    int kind = BC_NOFLUX;
    FieldVec<NF> value;  // per column
};

}  // namespace trm_oracle
#include "vegetation_oracle.hpp"   // the 0-D vegetation / canopy processes the coupled LandModel below steps
namespace trm_oracle {

template <class NF, class MF = NF> class Oracle {
  public:
    static NF lit(double x) { return model_literal<NF, MF>(x); }   // a literal the reference converts to its number format
    Grid<NF> g;
    ParamsD pd;
    Params<NF> p;
    long Nh;
    int Nz;
    double time = 0.0;
    long long iteration = 0;
    uint32_t status = 0;  // bit0 NaN seen (unused here), bit1 composition out of [0,1]
    // Column range the passes below work on: the whole grid by default; the cache-blocked driver (steps_blocked)
    // narrows it per thread to one block of columns at a time.
    static long& range_lo() { static thread_local long v = 0; return v; }
    static long& range_hi() { static thread_local long v = -1; return v; }
    long col_lo() const { return range_lo(); }
    long col_hi() const { long h = range_hi(); return h < 0 ? Nh : h; }

    // 3-D centre fields with z halos: (Nz+2) x Nh
    FieldVec<NF> U, sat, T, liq, psi, G_U, G_sat;
    FieldVec<NF> Fvwc;        // per-cell vwc_forcing (halo layout); used instead of p.vwc_forcing once set
    bool use_Fvwc = false;
    // face field with halos: (Nz+3) x Nh (faces 0..Nz+2)
    FieldVec<NF> Kf;
    // 2-D
    FieldVec<NF> S, G_S, wt, Ts, ghf, swu, lwu, rnet, Hs, Hl, evap, infil, runoff;
    FieldVec<NF> Tair, pres, wind, qair, rain, swd, lwd;
    FieldVec<NF> albedo_in, emissivity_in;   // PrescribedAlbedo inputs (albedo.jl:8-14)
    Bc<NF> bc[BCV_COUNT][2];  // [var][0 = bottom, 1 = top]
    bool land_model = false;  // LandModel wiring of ground_heat_flux / infiltration flux BCs

    // LandModel(vegetation = VegetationCarbon) (land_model.jl:24-25,79-97): the vegetation state, the canopy water store and
    // the canopy evapotranspiration fluxes; plant available water per cell (halo layout) and the static root fractions per level
    bool veg_on = false;
    VegetationOracle<NF, MF> veg;
    FieldVec<NF> w_can, G_w_can, I_can, R_can, f_can, rain_ground, E_can, transp, SAI, paw;
    std::vector<NF> root_frac;

    Oracle(long nh, int nz, const double* thickness, double dx, const ParamsD& pd_in) : pd(pd_in), p(model_params<MF>(pd_in)), Nh(nh), Nz(nz) {
        g.template build<MF>(nh, nz, thickness, dx);
        size_t n3 = (size_t)(nz + 2) * nh, nf = (size_t)(nz + 3) * nh, n2 = (size_t)nh;
        (void)n3; (void)nf; (void)n2;
        for (auto* v : {&U, &sat, &T, &liq, &psi, &G_U, &G_sat, &Fvwc}) first_touch(*v, nz + 2, NF(0));
        first_touch(Kf, nz + 3, NF(0));
        for (auto* v : {&S, &G_S, &wt, &Ts, &ghf, &swu, &lwu, &rnet, &Hs, &Hl, &evap, &infil, &runoff}) first_touch(*v, 1, NF(0));
        // input defaults (prescribed_atmosphere.jl:90-92,148,221-223)
        first_touch(Tair, 1, NF(10));
        first_touch(pres, 1, NF(101325));
        first_touch(wind, 1, lit(0.1));
        first_touch(qair, 1, lit(1.0e-3));
        first_touch(rain, 1, NF(0));
        first_touch(swd, 1, NF(300));
        first_touch(lwd, 1, NF(50));
        first_touch(albedo_in, 1, NF(0));
        first_touch(emissivity_in, 1, NF(0));
        land_model = p.seb != 0;
    }

    // sizes `v` to rows x Nh and writes `x` from the thread that owns each column in the compute passes (static schedule over i)
    void first_touch(FieldVec<NF>& v, int rows, NF x) {
        v.resize((size_t)rows * Nh);
        NF* q = v.data();
        const long nh = Nh;
        TRM_OMP_FOR
        for (long i = 0; i < nh; ++i)
            for (int k = 0; k < rows; ++k) q[(size_t)k * nh + i] = x;
    }
    inline size_t C(int k, long i) const { return (size_t)k * Nh + i; }

    bool richards() const { return p.flow == FLOW_RICHARDS; }

    // ---- field access for the harness (interior only, k = 0 bottom) ---------
    FieldVec<NF>* field3(int id) {
        switch (id) {
            case F_INTERNAL_ENERGY: return &U;
            case F_SATURATION: return &sat;
            case F_TEMPERATURE: return &T;
            case F_LIQUID_FRACTION: return &liq;
            case F_PRESSURE_HEAD: return &psi;
            case F_TEND_INTERNAL_ENERGY: return &G_U;
            case F_TEND_SATURATION: return &G_sat;
            case F_VWC_FORCING: return &Fvwc;
            case F_PLANT_AVAILABLE_WATER: return veg_on ? &paw : nullptr;
            default: return nullptr;
        }
    }
    FieldVec<NF>* field2(int id) {
        switch (id) {
            case F_SURFACE_EXCESS_WATER: return &S;
            case F_TEND_SURFACE_EXCESS_WATER: return &G_S;
            case F_WATER_TABLE: return &wt;
            case F_SKIN_TEMPERATURE: return &Ts;
            case F_GROUND_HEAT_FLUX: return &ghf;
            case F_SW_UP: return &swu;
            case F_LW_UP: return &lwu;
            case F_NET_RADIATION: return &rnet;
            case F_SENSIBLE_HEAT_FLUX: return &Hs;
            case F_LATENT_HEAT_FLUX: return &Hl;
            case F_EVAPORATION_GROUND: return &evap;
            case F_INFILTRATION: return &infil;
            case F_SURFACE_RUNOFF: return &runoff;
            case F_AIR_TEMPERATURE: return &Tair;
            case F_AIR_PRESSURE: return &pres;
            case F_WINDSPEED: return &wind;
            case F_SPECIFIC_HUMIDITY: return &qair;
            case F_RAINFALL: return &rain;
            case F_SW_DOWN: return &swd;
            case F_LW_DOWN: return &lwd;
            case F_ALBEDO: return &albedo_in;
            case F_EMISSIVITY: return &emissivity_in;
            default: break;
        }
        if (!veg_on) return nullptr;
        if (id >= F_CARBON_VEGETATION && id <= F_NET_PRIMARY_PRODUCTION) return veg.field(id - F_CARBON_VEGETATION);
        switch (id) {
            case F_CO2: return &veg.CO2;
            case F_SOIL_MOISTURE_LIMITING_FACTOR: return &veg.smlf;
            case F_DAILY_LEAF_RESPIRATION: return &veg.daily_Rd;
            case F_CANOPY_WATER: return &w_can;
            case F_TEND_CANOPY_WATER: return &G_w_can;
            case F_CANOPY_WATER_INTERCEPTION: return &I_can;
            case F_CANOPY_WATER_REMOVAL: return &R_can;
            case F_SATURATION_CANOPY_WATER: return &f_can;
            case F_RAINFALL_GROUND: return &rain_ground;
            case F_EVAPORATION_CANOPY: return &E_can;
            case F_TRANSPIRATION: return &transp;
            case F_STEM_AREA_INDEX: return &SAI;
            default: return nullptr;
        }
    }
    // LandModel(grid; soil, vegetation): switch the vegetation and canopy processes on
    void enable_vegetation(const VegParamsD& vp) {
        veg = VegetationOracle<NF, MF>(Nh, vp, pd);
        veg_on = true;
        for (auto* v : {&w_can, &G_w_can, &I_can, &R_can, &f_can, &rain_ground, &E_can, &transp, &SAI}) first_touch(*v, 1, NF(0));
        first_touch(paw, Nz + 2, NF(0));
        // root_fraction (root_distribution.jl:51-63): density at the cell centres times the thickness, normalised over the column
        root_frac.assign((size_t)Nz + 2, NF(0));
        NF total = NF(0);
        for (int k = 1; k <= Nz; ++k) { root_frac[k] = veg_root_density(veg.p, g.zC[k]) * g.dzc[k]; }
        for (int k = 1; k <= Nz; ++k) total = total + root_frac[k];
        for (int k = 1; k <= Nz; ++k) root_frac[k] = root_frac[k] / total;
    }
    long field_rows(int id) const {
        if (id == F_HYDRAULIC_CONDUCTIVITY) return Nz + 1;
        if (id <= F_TEND_SATURATION || id == F_VWC_FORCING || id == F_PLANT_AVAILABLE_WATER || id == F_ROOT_FRACTION) return Nz;
        return 1;
    }
    int set_field(int id, const NF* src) {  // set!(field, array): interior only
        if (id == F_HYDRAULIC_CONDUCTIVITY) {
            for (int k = 1; k <= Nz + 1; ++k) std::memcpy(&Kf[C(k, 0)], src + (size_t)(k - 1) * Nh, sizeof(NF) * Nh);
            return 0;
        }
        if (auto* v = field3(id)) {
            for (int k = 1; k <= Nz; ++k) std::memcpy(&(*v)[C(k, 0)], src + (size_t)(k - 1) * Nh, sizeof(NF) * Nh);
            if (id == F_VWC_FORCING) use_Fvwc = true;
            return 0;
        }
        if (auto* v = field2(id)) { std::memcpy(v->data(), src, sizeof(NF) * Nh); return 0; }
        return 1;
    }
    int get_field(int id, NF* dst) {
        if (id == F_ROOT_FRACTION && veg_on) {
            for (int k = 1; k <= Nz; ++k) std::fill(dst + (size_t)(k - 1) * Nh, dst + (size_t)k * Nh, root_frac[k]);
            return 0;
        }
        if (id == F_HYDRAULIC_CONDUCTIVITY) {
            for (int k = 1; k <= Nz + 1; ++k) std::memcpy(dst + (size_t)(k - 1) * Nh, &Kf[C(k, 0)], sizeof(NF) * Nh);
            return 0;
        }
        if (auto* v = field3(id)) {
            for (int k = 1; k <= Nz; ++k) std::memcpy(dst + (size_t)(k - 1) * Nh, &(*v)[C(k, 0)], sizeof(NF) * Nh);
            return 0;
        }
        if (auto* v = field2(id)) { std::memcpy(dst, v->data(), sizeof(NF) * Nh); return 0; }
        return 1;
    }
    // read one halo value (test hook for K14)
    NF get_halo(int id, int top, long i) {
        auto* v = field3(id);
        return v ? (*v)[C(top ? Nz + 1 : 0, i)] : NF(0);
    }
    int set_bc(int var, int top, int kind, const NF* values /*Nh or null*/, NF scalar) {
        if (var < 0 || var >= BCV_COUNT) return 1;
        Bc<NF>& b = bc[var][top ? 1 : 0];
        b.kind = kind;
        if (kind == BC_NOFLUX) { b.value.clear(); return 0; }
        b.value.assign(Nh, scalar);
        if (values) std::memcpy(b.value.data(), values, sizeof(NF) * Nh);
        return 0;
    }

    // ---- FieldTimeSeriesInputSource / update_inputs! (input_sources.jl:142-171) -------------
    // `set!(field, fts[Time(clock.time)])`.  The time interpolation is Oceananigans' FieldTimeSeries indexing
    // (OutputReaders, not part of the reference tree: restated from its published behaviour, PARITY UNPINNED):
    //   find_time_index: binary search for the bracketing nodes n1 < n2 (an interior node hit gives n1 == n2;
    //   outside the range the first / last interval is used => Linear extrapolates), fraction
    //   f = (n2 - n1) / (t[n2] - t[n1]) * (t - t[n1]);  Clamp: end values outside the range;  Cyclical: time taken
    //   modulo the period (last node -> first node closes the cycle with the last interval's length);
    //   getindex(fts, Time(t)) = v[n2] * f + v[n1] * (1 - f)  (Float64 scalar times NF field, stored as NF).
    struct Series {
        bool is_bc = false;
        int field = 0, var = 0, top = 0, indexing = 0;
        std::vector<double> times;
        std::vector<NF> values;  // [nt][Nh]
    };
    std::vector<Series> series;
    enum { TIME_LINEAR = 0, TIME_CLAMP = 1, TIME_CYCLICAL = 2, TIME_RASTER = 3 };

    static void find_time_index(const std::vector<double>& times, double t, double& f, long& n1, long& n2) {
        long Nt = (long)times.size();
        long low = 0, high = Nt - 1;   // index_binary_search, 0-based
        while (low + 1 < high) {
            long mid = (low + high) / 2;
            if (times[mid] == t) { n1 = n2 = mid; f = 0.0; return; }
            if (times[mid] < t) low = mid; else high = mid;
        }
        n1 = low; n2 = high;
        double dt = times[n2] - times[n1];
        f = (double)(n2 - n1) / dt * (t - times[n1]);
    }
    static void interpolating_time_indices(const std::vector<double>& times, int indexing, double t, double& f, long& n1, long& n2) {
        long Nt = (long)times.size();
        if (Nt == 1) { f = 0.0; n1 = n2 = 0; return; }
        if (indexing == TIME_CYCLICAL) {
            double t1 = times[0], tN = times[Nt - 1];
            double T = (tN - t1) + (tN - times[Nt - 2]);
            double tau = t - t1;
            double mod_tau = std::fmod(tau, T);
            if (mod_tau < 0) mod_tau += T;
            double mod_t = mod_tau + t1;
            if (mod_t > tN) {  // cycling: between tN and t1 + T
                double dT = T - (tN - t1);
                f = 1.0 / dT * (mod_t - tN);
                n1 = Nt - 1; n2 = 0;
                return;
            }
            find_time_index(times, mod_t, f, n1, n2);
            return;
        }
        find_time_index(times, t, f, n1, n2);
        if (indexing == TIME_CLAMP) {
            if (t >= times[Nt - 1]) { f = 0.0; n1 = n2 = Nt - 1; }
            else if (t <= times[0]) { f = 0.0; n1 = n2 = 0; }
        }
    }
    int set_series(bool is_bc, int field, int var, int top, int kind, long nt, const double* times, const NF* values, int indexing) {
        if (nt < 1) return 1;
        Series sr;
        sr.is_bc = is_bc; sr.field = field; sr.var = var; sr.top = top ? 1 : 0; sr.indexing = indexing;
        sr.times.assign(times, times + nt);
        sr.values.assign(values, values + (size_t)nt * Nh);
        for (size_t n = 0; n < series.size(); ++n) {
            const Series& o = series[n];
            if (o.is_bc == is_bc && (is_bc ? (o.var == var && o.top == sr.top) : o.field == field)) { series.erase(series.begin() + (long)n); break; }
        }
        if (is_bc) {
            Bc<NF>& b = bc[var][sr.top];
            b.kind = kind;
            b.value.assign(Nh, NF(0));
        }
        series.push_back(std::move(sr));
        return 0;
    }
    // (the interpolation weights are Float64 in the reference; the products below are formed in double for every NF, so a
    // wide instance gains nothing on a time series -- the accuracy suite uses constant inputs)
    void update_inputs() {
        for (const Series& sr : series) {
            double f; long n1, n2;
            interpolating_time_indices(sr.times, sr.indexing, time, f, n1, n2);
            FieldVec<NF>* dst = sr.is_bc ? &bc[sr.var][sr.top].value : field2(sr.field);
            const NF* v1 = &sr.values[(size_t)n1 * Nh];
            const NF* v2 = &sr.values[(size_t)n2 * Nh];
            if (sr.indexing == TIME_RASTER) {
                // update_from_raster! (ext/TerrariumRastersExt/TerrariumRastersExt.jl:96-121), numeric time axis
                const std::vector<double>& tt = sr.times;
                const long nt = (long)tt.size();
                const long right = (long)(std::lower_bound(tt.begin(), tt.end(), time) - tt.begin());   // first(searchsorted) - 1
                const long left = (long)(std::upper_bound(tt.begin(), tt.end(), time) - tt.begin()) - 1; // last(searchsorted) - 1
                if (left >= 0 && right <= nt - 1) {
                    const NF* x1 = &sr.values[(size_t)left * Nh];
                    const NF* x2 = &sr.values[(size_t)right * Nh];
                    const double dT = tt[right] - tt[left], eps = time - tt[left];
                    for (long i = col_lo(); i < col_hi(); ++i)
                        (*dst)[i] = dT > 0 ? (NF)((double)x1[i] + eps * (double)(NF)(x2[i] - x1[i]) / dT) : x2[i];
                } else {
                    const NF* x = &sr.values[(size_t)std::min(right, nt - 1) * Nh];
                    for (long i = col_lo(); i < col_hi(); ++i) (*dst)[i] = x[i];
                }
                continue;
            }
            for (long i = col_lo(); i < col_hi(); ++i)
                (*dst)[i] = (n1 == n2) ? v1[i] : (NF)((double)v2[i] * f + (double)v1[i] * (1.0 - f));
        }
    }

    // ---- fill_halo_regions!(state) (state_variables.jl:85-100) --------------
    // Oceananigans z-halo rules: Value -> linear
    // extrapolation through the boundary value with the boundary-face spacing;
    // Gradient -> edge +/- g*Δ; Flux / NoFlux / default -> copy of the edge.
    void fill_halo(FieldVec<NF>& c, int var) {
        const Bc<NF>& bt = bc[var][1];
        const Bc<NF>& bb = bc[var][0];
        NF dtop = g.dzf[Nz + 1], dbot = g.dzf[1];
        TRM_OMP_FOR
        for (long i = col_lo(); i < col_hi(); ++i) {
            NF cN = c[C(Nz, i)], c1 = c[C(1, i)];
            if (bt.kind == BC_VALUE) {
                NF grad = (bt.value[i] - cN) / (dtop / NF(2));
                c[C(Nz + 1, i)] = cN + grad * dtop;
            } else if (bt.kind == BC_GRADIENT) {
                c[C(Nz + 1, i)] = cN + bt.value[i] * dtop;
            } else {
                c[C(Nz + 1, i)] = cN;
            }
            if (bb.kind == BC_VALUE) {
                NF grad = (c1 - bb.value[i]) / (dbot / NF(2));
                c[C(0, i)] = c1 + grad * (-dbot);
            } else if (bb.kind == BC_GRADIENT) {
                c[C(0, i)] = c1 + bb.value[i] * (-dbot);
            } else {
                c[C(0, i)] = c1;
            }
        }
    }
    void fill_halo_regions() {
        // prognostic variables first, then closure variables
        fill_halo(U, BCV_INTERNAL_ENERGY);
        if (richards()) fill_halo(sat, BCV_SATURATION);
        // closure variables: hydrology's (pressure_head) are declared before
        // energy's in the merged variable list, order is irrelevant here
        if (richards()) fill_halo(psi, BCV_PRESSURE_HEAD);
        fill_halo(T, BCV_TEMPERATURE);
        fill_halo(liq, BCV_LIQUID_FRACTION);
        if (!richards() && p.halo_policy == HALO_MIRROR) {
            // policy switch for SURVEY Appendix C-1: under NoFlow the reference
            // never fills the halos of the auxiliary saturation field.
            for (long i = col_lo(); i < col_hi(); ++i) { sat[C(0, i)] = sat[C(1, i)]; sat[C(Nz + 1, i)] = sat[C(Nz, i)]; }
        }
    }

    // ---- soil composition at (k, i) incl. halo cells ------------------------
    inline Fractions<NF> fractions_at(int k, long i, NF por, NF org) {
        return volumetric_fractions(por, sat[C(k, i)], liq[C(k, i)], org, &status);
    }

    // ---- compute_hydraulics! (soil_hydrology.jl:145-163) --------------------
    void compute_hydraulics() {
        NF por = porosity(p), org = organic_fraction(p);
        TRM_OMP_FOR
        for (long i = col_lo(); i < col_hi(); ++i) {
            auto Kc = [&](int k) { return hydraulic_conductivity_cell(p, por, liq[C(k, i)], fractions_at(k, i, por, org)); };
            for (int k = 1; k <= Nz; ++k) {
                if (k <= 1) {
                    Kf[C(k, i)] = Kc(1);
                } else if (k >= Nz) {
                    Kf[C(k, i)] = Kc(Nz);
                    Kf[C(k + 1, i)] = Kf[C(k, i)];
                } else {
                    Kf[C(k, i)] = jl_min(Kc(k), Kc(k - 1));
                }
            }
        }
    }

    // ---- surface processes (Appendix A-9) -----------------------------------
    inline NF aerodynamic_resistance(long i) const {  // prescribed_atmosphere.jl:110-116,137
        NF V = jl_max(wind[i], p.min_windspeed);
        NF Va = jl_max(V, lit(1.0e-6));
        return NF(1) / (p.C_h * Va);
    }
    inline NF humidity_vpd(long i, NF Tsurf) const {  // prescribed_atmosphere.jl:163-182, physics_utils.jl:38
        NF de = compute_vpd<NF, MF>(p, pres[i], qair[i], Tsurf);
        return p.eps_mw * de / pres[i];
    }
    // ground_evaporation_resistance_factor (ground_resistance_factor.jl:12,36-56)
    inline NF ground_resistance_factor(long i) const {
        NF beta = p.beta_evap;
        if (p.evap_resistance == 1) {
            NF por = porosity(p);
            Fractions<NF> fr = volumetric_fractions(por, sat[C(Nz, i)], liq[C(Nz, i)], organic_fraction(p));
            NF fc = p.field_capacity;
            if (fr.water < fc) {
                NF t = NF(1) - std::cos(lit(3.141592653589793) * fr.water / fc);
                beta = (t * t) / NF(4);
            } else {
                beta = NF(1);
            }
        }
        return beta;
    }
    void compute_evaporation() {  // bare_ground_evaporation.jl:49-62
        TRM_OMP_FOR
        for (long i = col_lo(); i < col_hi(); ++i) {
            NF ra = aerodynamic_resistance(i);
            NF dq = humidity_vpd(i, Ts[i]);
            NF beta = ground_resistance_factor(i);
            evap[i] = beta * dq / ra;
        }
    }
    // compute_auxiliary!(state, grid, veg::VegetationCarbon, constants, atmos, soil) (vegetation_carbon.jl:66-104) with the
    // soil present: plant available water from the soil's liquid water content (plant_available_water.jl:48-94), its
    // root-weighted integral as the soil moisture limiting factor (:33-38, Integral sums (W r / dz) dz from the bottom
    // cell up) and ground_temperature = the top soil cell (soil_energy.jl:48-57), then the 0-D processes.
    void compute_vegetation() {
        NF por = porosity(p), org = organic_fraction(p);
        for (long i = col_lo(); i < col_hi(); ++i) {
            NF acc = NF(0);
            for (int k = 1; k <= Nz; ++k) {
                Fractions<NF> fr = volumetric_fractions(por, sat[C(k, i)], liq[C(k, i)], org);
                NF w = veg_plant_available_water(veg.p, fr.water);
                paw[C(k, i)] = w;
                acc = acc + (w * root_frac[k] / g.dzc[k]) * g.dzc[k];
            }
            veg.smlf[i] = acc;
            veg.Tground[i] = T[C(Nz, i)];
            veg.Tair[i] = Tair[i]; veg.pres[i] = pres[i]; veg.qair[i] = qair[i]; veg.swd[i] = swd[i];
        }
        veg.compute_auxiliary(col_lo(), col_hi());
    }
    // compute_auxiliary!(state, grid, ::PALADYNCanopyInterception, atmos) (canopy_interception.jl:170-199)
    void compute_canopy_interception() {
        for (long i = col_lo(); i < col_hi(); ++i) {
            NF LAI = veg.LAI[i], sai = SAI[i], w = w_can[i];
            f_can[i] = canopy_saturation_fraction(veg.p, w, LAI, sai);
            I_can[i] = canopy_interception(veg.p, rain[i], LAI, sai);
            R_can[i] = canopy_water_removal(veg.p, w);
            rain_ground[i] = canopy_precip_ground(rain[i], I_can[i], R_can[i]);
        }
    }
    // compute_evapotranspiration! of PALADYNCanopyEvapotranspiration (canopy_evapotranspiration.jl:127-158)
    void compute_canopy_evapotranspiration() {
        for (long i = col_lo(); i < col_hi(); ++i) {
            NF Tg = T[C(Nz, i)];
            NF dqs = humidity_vpd(i, Ts[i]);
            NF dqg = humidity_vpd(i, Tg);
            NF ra = aerodynamic_resistance(i);
            NF re = canopy_ground_resistance(veg.p, veg.LAI[i], SAI[i], jl_max(wind[i], p.min_windspeed));
            NF beta = ground_resistance_factor(i);
            transp[i] = canopy_transpiration<NF, MF>(dqs, ra, veg.gw_can[i]);
            evap[i] = canopy_evaporation_ground(dqg, beta, ra, re);
            E_can[i] = canopy_evaporation_canopy(dqs, f_can[i], ra);
        }
    }
    void compute_runoff() {  // direct_surface_runoff.jl:87-117
        TRM_OMP_FOR
        for (long i = col_lo(); i < col_hi(); ++i) {
            NF rainfall = veg_on ? rain_ground[i] : rain[i];   // rainfall_ground(i, j, grid, fields, canopy_interception)
            NF excess = richards() ? S[i] : NF(0);
            NF k_unsat = Kf[C(Nz, i)];
            NF sat_top = sat[C(Nz, i)];
            NF drainage, inf;
            if (excess > NF(0)) {
                drainage = compute_surface_drainage(p, excess);
                inf = compute_infiltration(drainage, sat_top, k_unsat);
            } else {
                drainage = NF(0);
                inf = compute_infiltration(rainfall, sat_top, k_unsat);
            }
            infil[i] = inf;
            runoff[i] = compute_surface_runoff(rainfall, drainage, inf);
        }
    }
    // LandModel couples the latent heat flux to the ET scheme (turbulent_fluxes.jl:130-143); the standalone
    // SurfaceEnergyModel of the reference's unit tests has no ET scheme and diagnoses it from the humidity deficit at
    // the skin temperature (turbulent_fluxes.jl:110-126, surface_energy_balance.jl:133-139).
    bool et_coupled = true;
    void seb_fluxes(long i) {  // surface_energy_balance.jl:119-144
        NF Tsurf = Ts[i];
        // albedo(i, j, ...) / emissivity(i, j, ...): ConstantAlbedo's parameters or PrescribedAlbedo's inputs
        // (albedo.jl:37-44, abstract_types.jl:120-131)
        const NF alb = p.prescribed_albedo ? albedo_in[i] : p.albedo;
        const NF emis = p.prescribed_albedo ? emissivity_in[i] : p.emissivity;
        swu[i] = alb * swd[i];
        NF Tk = Tsurf + p.Tref;
        lwu[i] = stefan_boltzmann(p, Tk, emis) + (NF(1) - emis) * lwd[i];
        rnet[i] = swu[i] - swd[i] + lwu[i] - lwd[i];
        NF ra = aerodynamic_resistance(i);
        NF Q_T = (Tsurf - Tair[i]) / ra;
        Hs[i] = sensible_heat_flux(p, Q_T);
        // surface_humidity_flux of the ET scheme: ground evaporation, plus canopy evaporation and transpiration under a
        // canopy (bare_ground_evaporation.jl:29, canopy_evapotranspiration.jl:97-102)
        NF Q_h = !et_coupled ? humidity_vpd(i, Tsurf) / ra : (veg_on ? evap[i] + E_can[i] + transp[i] : evap[i]);
        Hl[i] = latent_heat_flux(p, Q_h);
        ghf[i] = rnet[i] - Hs[i] - Hl[i];
    }
    void compute_surface_energy_fluxes() {  // surface_energy_balance.jl:95-110
        NF dz1 = g.dzc[Nz];
        TRM_OMP_FOR
        for (long i = col_lo(); i < col_hi(); ++i) {
            seb_fluxes(i);
            NF Tg = T[C(Nz, i)];  // ground_temperature = view of the top soil layer (soil_energy.jl:52-57)
            Ts[i] = compute_skin_temperature(p, Tg, ghf[i], dz1);
            seb_fluxes(i);
        }
    }
    void update_skin_temperature() {  // skin_temperature.jl:104-109
        NF dz1 = g.dzc[Nz];
        for (long i = col_lo(); i < col_hi(); ++i) Ts[i] = compute_skin_temperature(p, T[C(Nz, i)], ghf[i], dz1);
    }

    // ---- compute_auxiliary!(state, model) -----------------------------------
    void compute_auxiliary() {
        compute_hydraulics();  // soil_coupled.jl:62-72 (energy/bgc are no-ops)
        if (p.seb) {           // land_model.jl:79-88
            if (veg_on) {      // vegetation, then surface hydrology = canopy interception, evapotranspiration, runoff
                compute_vegetation();
                compute_canopy_interception();
                compute_canopy_evapotranspiration();
            } else {
                compute_evaporation();
            }
            compute_runoff();
            compute_surface_energy_fluxes();
            compute_surface_energy_fluxes();
        }
    }

    // ---- compute_tendencies!(state, model) ----------------------------------
    void compute_tendencies() {
        NF por = porosity(p), org = organic_fraction(p);
        if (veg_on)   // compute_tendencies!(surface_hydrology): canopy water (canopy_interception.jl:201-215)
            for (long i = col_lo(); i < col_hi(); ++i) G_w_can[i] = canopy_w_can_tendency(I_can[i], E_can[i], R_can[i]);
        // hydrology first (soil_coupled.jl:80-90)
        if (richards()) {
            TRM_OMP_FOR
            for (long i = col_lo(); i < col_hi(); ++i) {
                auto darcy = [&](int k) {  // soil_hydrology_rre.jl:115-131
                    NF grad = (psi[C(k, i)] - psi[C(k - 1, i)]) * g.rdzf[k];
                    NF Kk = jl_boolmul(grad < NF(0), jl_min(Kf[C(k - 1, i)], Kf[C(k, i)])) +
                            jl_boolmul(grad >= NF(0), jl_min(Kf[C(k, i)], Kf[C(k + 1, i)]));
                    return -Kk * grad;
                };
                for (int k = 1; k <= Nz; ++k) {
                    NF div = (darcy(k + 1) - darcy(k)) * g.rdzc[k];
                    NF F_user = use_Fvwc ? Fvwc[C(k, i)] : p.vwc_forcing;   // forcing(i, j, k, grid, clock, fields, vwc_forcing, ...)
                    NF dtheta = -div + NF(0) /*ET forcing: evtr is never passed (soil_coupled.jl:86)*/ + F_user;
                    G_sat[C(k, i)] += dtheta / por;
                }
                // surface excess water: evaluated once per column (SURVEY C-3)
                NF s = S[i];
                G_S[i] += jl_min(NF(0), s);
            }
        }
        // energy (soil_energy.jl:112-149)
        TRM_OMP_FOR
        for (long i = col_lo(); i < col_hi(); ++i) {
            auto kappa = [&](int k) { return thermal_conductivity(p, fractions_at(k, i, por, org)); };
            auto q = [&](int k) {
                NF kf = NF(0.5) * (kappa(k) + kappa(k - 1));
                return -kf * ((T[C(k, i)] - T[C(k - 1, i)]) * g.rdzf[k]);
            };
            for (int k = 1; k <= Nz; ++k) {
                NF dUdt = -((q(k + 1) - q(k)) * g.rdzc[k]);
                G_U[C(k, i)] += dUdt;
            }
        }
        if (veg_on) veg.compute_tendencies(col_lo(), col_hi());   // land_model.jl:94
    }

    // ---- update_state! (state_variables.jl:72-80) ---------------------------
    void reset_tendencies() {
        const long i0_ = col_lo(), i1_ = col_hi();
        for (int k = 1; k <= Nz; ++k)
            TRM_OMP_FOR
            for (long i = i0_; i < i1_; ++i) { G_U[C(k, i)] = NF(0); G_sat[C(k, i)] = NF(0); }
        std::fill(G_S.begin() + i0_, G_S.begin() + i1_, NF(0));
        if (veg_on) {
            std::fill(G_w_can.begin() + i0_, G_w_can.begin() + i1_, NF(0));
            std::fill(veg.G_C_veg.begin() + i0_, veg.G_C_veg.begin() + i1_, NF(0));
            std::fill(veg.G_nu.begin() + i0_, veg.G_nu.begin() + i1_, NF(0));
        }
    }
    void update_state(bool tendencies = true, bool inputs = true) {
        reset_tendencies();
        if (inputs) update_inputs();  // constant inputs are set by the harness before the call; series are evaluated at `time`
        fill_halo_regions();
        compute_auxiliary();
        if (tendencies) compute_tendencies();
    }

    // ---- explicit_step! (abstract_timestepper.jl:65-141) --------------------
    void apply_z_flux_bcs(FieldVec<NF>& G, int var, const FieldVec<NF>* top_field, bool negate_top) {
        // Oceananigans compute_z_bcs!: Flux BCs only; G[1] += F*Az/V, G[Nz] -= F*Az/V
        NF Az = g.dx;  // Flat y => Δy = 1
        NF Vtop = Az * g.dzc[Nz], Vbot = Az * g.dzc[1];
        const Bc<NF>& bt = bc[var][1];
        const Bc<NF>& bb = bc[var][0];
        TRM_OMP_FOR
        for (long i = col_lo(); i < col_hi(); ++i) {
            if (bb.kind == BC_FLUX) G[C(1, i)] += bb.value[i] * Az / Vbot;
            if (top_field) {
                NF F = negate_top ? -(*top_field)[i] : (*top_field)[i];
                G[C(Nz, i)] -= F * Az / Vtop;
            } else if (bt.kind == BC_FLUX) {
                G[C(Nz, i)] -= bt.value[i] * Az / Vtop;
            }
        }
    }
    void explicit_step(NF dt) {
        // prognostic order: soil (energy, hydrology) then SEB's skin_temperature
        // (zero tendency); each prognostic is independent of the others here.
        apply_z_flux_bcs(G_U, BCV_INTERNAL_ENERGY, land_model ? &ghf : nullptr, false);  // land_model.jl:56-58
        const long i0_ = col_lo(), i1_ = col_hi();
        for (int k = 1; k <= Nz; ++k)
            TRM_OMP_FOR
            for (long i = i0_; i < i1_; ++i) U[C(k, i)] = U[C(k, i)] + G_U[C(k, i)] * dt;
        if (richards()) {
            apply_z_flux_bcs(G_sat, BCV_SATURATION, land_model ? &infil : nullptr, true);  // land_model.jl:57-61
            for (int k = 1; k <= Nz; ++k)
                TRM_OMP_FOR
                for (long i = i0_; i < i1_; ++i) sat[C(k, i)] = sat[C(k, i)] + G_sat[C(k, i)] * dt;
            for (long i = col_lo(); i < col_hi(); ++i) S[i] = S[i] + G_S[i] * dt;
        }
        if (p.seb)
            for (long i = col_lo(); i < col_hi(); ++i) Ts[i] = Ts[i] + NF(0) * dt;  // skin_temperature: prognostic, zero tendency
        if (veg_on) {
            for (long i = col_lo(); i < col_hi(); ++i) w_can[i] = w_can[i] + G_w_can[i] * dt;
            veg.explicit_step(dt, col_lo(), col_hi());
        }
    }

    // ---- hydrology closure (soil_hydraulic_closures.jl:23-44) ---------------
    void adjust_saturation_profile() {  // soil_hydrology.jl:185-219
        TRM_OMP_FOR
        for (long i = col_lo(); i < col_hi(); ++i) {
            for (int k = 1; k <= Nz - 1; ++k) {
                NF excess = jl_max(sat[C(k, i)] - NF(1), NF(0));
                sat[C(k, i)] -= excess;
                sat[C(k + 1, i)] += excess * g.dzc[k] / g.dzc[k + 1];
            }
            for (int k = Nz; k >= 2; --k) {
                NF deficit = jl_max(-sat[C(k, i)], NF(0));
                sat[C(k, i)] += deficit;
                sat[C(k - 1, i)] -= deficit * g.dzc[k] / g.dzc[k - 1];
            }
            NF excess = jl_max(sat[C(Nz, i)] - NF(1), NF(0));
            sat[C(Nz, i)] -= excess;
            S[i] += excess * g.dzc[Nz];
            sat[C(1, i)] = jl_max(sat[C(1, i)], NF(0));
        }
    }
    void compute_water_table() {  // soil_hydrology.jl:170-175, kernel_utils.jl:7-16
        int n = Nz + 1;           // znodes(Center, Center, Face): Nz+1 faces; index Nz+1 reads the top halo cell
        TRM_OMP_FOR
        for (long i = col_lo(); i < col_hi(); ++i) {
            int idx = -1;
            for (int k = 1; k <= n; ++k)
                if (idx < 0 && sat[C(k, i)] < NF(1)) idx = k;
            wt[i] = idx > 0 ? g.zF[idx] : g.zF[n];
        }
    }
    void saturation_to_pressure() {  // soil_hydraulic_closures.jl:102-129
        NF por = porosity(p);
        NF z_ref = g.zF[Nz + 1];
        TRM_OMP_FOR
        for (long i = col_lo(); i < col_hi(); ++i) {
            NF z0 = wt[i];
            for (int k = 1; k <= Nz; ++k) {
                NF z = g.zC[k];
                NF psim = swrc_psi(p, sat[C(k, i)] * por, por);
                NF psiz = z - z_ref;
                NF psih = jl_max(NF(0), z0 - z);
                psi[C(k, i)] = psih + psim + psiz;
            }
        }
    }
    void pressure_to_saturation() {  // soil_hydraulic_closures.jl:74-100
        NF por = porosity(p);
        NF z_ref = g.zF[Nz + 1];
        TRM_OMP_FOR
        for (long i = col_lo(); i < col_hi(); ++i) {
            NF z0 = wt[i];
            for (int k = 1; k <= Nz; ++k) {
                NF z = g.zC[k];
                NF psiz = z - z_ref;
                NF psih = jl_max(NF(0), z0 - z);
                NF psim = psi[C(k, i)] - psih - psiz;
                sat[C(k, i)] = swrc_theta(p, psim, por) / por;
            }
        }
    }
    // ---- energy closure (soil_energy_closures.jl:99-126 / 64-97) ------------
    void energy_to_temperature_all() {
        NF por = porosity(p), org = organic_fraction(p);
        NF L = p.rho_w * p.Lsl;
        const long i0_ = col_lo(), i1_ = col_hi();
        for (int k = 1; k <= Nz; ++k)
            TRM_OMP_FOR
            for (long i = i0_; i < i1_; ++i) {
                NF u = U[C(k, i)], s = sat[C(k, i)];
                NF Ltheta = L * s * por;
                NF l = liquid_water_fraction<NF, MF>(u, Ltheta);
                liq[C(k, i)] = l;
                NF Cv = heat_capacity(p, volumetric_fractions(por, s, l, org, &status));
                T[C(k, i)] = energy_to_temperature(u, Ltheta, Cv);
            }
    }
    void temperature_to_energy_all() {
        NF por = porosity(p), org = organic_fraction(p);
        NF L = p.rho_w * p.Lsl;
        const long i0_ = col_lo(), i1_ = col_hi();
        for (int k = 1; k <= Nz; ++k)
            TRM_OMP_FOR
            for (long i = i0_; i < i1_; ++i) {
                NF t = T[C(k, i)], s = sat[C(k, i)];
                NF l = (t >= NF(0)) ? NF(1) : NF(0);
                liq[C(k, i)] = l;
                NF Cv = heat_capacity(p, volumetric_fractions(por, s, l, org, &status));
                U[C(k, i)] = t * Cv - L * s * por * (NF(1) - l);
            }
    }
    void closure() {  // soil_coupled.jl:99-107: hydrology, then energy
        if (richards()) {
            adjust_saturation_profile();
            compute_water_table();
            saturation_to_pressure();
        }
        energy_to_temperature_all();
    }
    void invclosure() {  // soil_coupled.jl:115-122
        if (richards()) {
            pressure_to_saturation();
            adjust_saturation_profile();
            compute_water_table();
        }
        temperature_to_energy_all();
    }

    // ---- initialize!(state, model) process part ----------------
    // The user/model initialisers (set! of temperature, saturation, ...) are
    // applied by the harness through set_field beforehand.
    void initialize_processes() {
        if (richards()) {  // soil_hydrology_rre.jl:33-47
            adjust_saturation_profile();
            compute_water_table();
            saturation_to_pressure();
            compute_hydraulics();
        } else {  // soil_hydrology.jl:113-117
            compute_hydraulics();
            compute_water_table();
        }
        temperature_to_energy_all();  // soil_energy.jl:64-77
    }

    // ---- time steppers ------------------------------------------------------
    void tick(double dt) { time += dt; iteration += 1; }
    void timestep_euler(double dt, bool finalize) {  // forward_euler.jl:19-31, model_integrator.jl:124-131
        update_state(true);
        explicit_step(NF(dt));
        closure();
        tick(dt);
        if (finalize) compute_auxiliary();
    }
    // The same step, cache-blocked ("fused driver" of BASELINE.md section 4.2): every pass of the step runs over one
    // block of columns while that block's rows sit in cache, blocks spread over the OpenMP threads.  Same passes, same
    // arithmetic, same order per column: results are identical to timestep_euler (tests/test_oracle_known_answers.py).
    void steps_blocked(double dt, long nsteps, long block) {
        const long nb = (Nh + block - 1) / block;
        for (long s = 0; s < nsteps; ++s) {
            update_inputs();
            TRM_OMP_FOR
            for (long b = 0; b < nb; ++b) {
                range_lo() = b * block;
                range_hi() = std::min(Nh, (b + 1) * block);
                update_state(true, false);
                explicit_step(NF(dt));
                closure();
                range_lo() = 0;
                range_hi() = -1;
            }
            tick(dt);
        }
    }
    void run(double dt, long steps) {  // model_integrator.jl:72-88
        for (long s = 0; s < steps; ++s) timestep_euler(dt, false);
        compute_auxiliary();
    }
    // average_tendencies! (heun.jl:27-35); the stage's status flags join the state's
    void average_tendencies(const Oracle& stage) {
        for (size_t n = 0; n < G_U.size(); ++n) G_U[n] = (G_U[n] + stage.G_U[n]) / NF(2);
        if (richards()) {
            for (size_t n = 0; n < G_sat.size(); ++n) G_sat[n] = (G_sat[n] + stage.G_sat[n]) / NF(2);
            for (size_t n = 0; n < G_S.size(); ++n) G_S[n] = (G_S[n] + stage.G_S[n]) / NF(2);
        }
        if (veg_on)
            for (long i = 0; i < Nh; ++i) {
                G_w_can[i] = (G_w_can[i] + stage.G_w_can[i]) / NF(2);
                veg.G_C_veg[i] = (veg.G_C_veg[i] + stage.veg.G_C_veg[i]) / NF(2);
                veg.G_nu[i] = (veg.G_nu[i] + stage.veg.G_nu[i]) / NF(2);
            }
        status |= stage.status;
    }
    void timestep_heun(double dt, bool finalize) {  // heun.jl:37-71
        update_state(true);
        Oracle stage = *this;  // copyto!(stage, state)
        stage.explicit_step(NF(dt));
        stage.closure();
        stage.tick(dt);
        stage.update_state(true);
        average_tendencies(stage);
        explicit_step(NF(dt));
        closure();
        tick(dt);
        if (finalize) compute_auxiliary();
    }
};

}  // namespace trm_oracle
