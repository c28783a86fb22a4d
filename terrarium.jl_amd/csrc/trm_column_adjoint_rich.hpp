// trm_column_adjoint_rich.hpp -- reverse-mode gradients of the heat + Richards ForwardEuler run (TRM_OPT_DERIVATIVE_RICHARDS_ADJOINT:
// trm_step_record and trm_adjoint_backward on a context with RichardsEq; DESIGN 4.8 "Richards").
//
// The sweep is the transpose of the linear map k_column_tangent_rich applies (trm_column_tangent_rich.hpp), branch for branch: given the
// cotangents (wU, wsat, wT, wliq, wpsi) of the final (U_n, sat_n, T_n, liq_n, psi_n) it returns gU = dL/dU_0 and gsat = dL/dsat_0, L the
// sum of the five inner products.  One forward step of the tangent at the state (U_k, sat_k) is
//   (dliq, dT) = closure_tangent_rich(dU, dsat),  dpsi = pressure_head_tangent(dsat)
//   (dgU, dgS) = tendency_tangent_rich(dsat, dT, dliq, dpsi)
//   dU' = dU + dgU dt,  dsat' = repair_tangent(dsat + dgS dt)
// and backwards, for the cotangents (lamU', lamS') of (dU', dsat'):
//   repair      mS = R^T lamS': the primal repair is replayed forward on the pre-repair saturation sat_k + gS dt, which keeps one decision
//               per lane and pass (x > 0 of the over-pass, y > 0 of the under-pass; a tie: 0), the levels each pass walked, the top
//               overflow and the bottom clamp; the transposed passes run in reverse order -- clamp, overflow, the under-pass bottom-up,
//               the over-pass top-down -- with shfl_from and the same div_const(. dzc, dz, rdz) factors
//   tendencies  heat: the face cotangents of the heat-only sweep (adjoint_step, trm_column_adjoint.hpp) under the mirror halo, the
//               cotangent of dkappa onto the three fraction tangents; water: the cotangent of dKs_lo goes to the operand min_tangent
//               selected (a tie: the second), through the upwind choice and the face minimum down to dKc; that of dg_lo to dpsi and dpsi_m
//   closures    hydraulic_conductivity_tangent and pressure_head_tangent are linear in their seeds: their slopes are the tangent
//               functions' own values at unit seeds.  closure_tangent_rich has two inputs and is transposed through dLth, dC and the
//               fractions (closure_transpose_rich)
// Constants (the boundary fluxes, vwc_forcing) drop out.  Where the tangent gives 0 for a zero operand whatever the factor (pow_tangent),
// the route gives 0 for a zero cotangent, and for a zero fraction coefficient in front of a conductivity slope: zero cotangents give
// exactly zero gradients and scaling by a power of two scales bit for bit.  A cell the primal flags as an illegal composition gives NaN.
// Every coefficient is a function of (U_k, sat_k) BEFORE step k: k_column_record_rich is the multi-step primal that stores both into tape
// slot k ([2][Nh][Nzp]) before every step; the sweep forms T, liq, psi, the water table, the fractions, Kc, the tendencies and the
// pre-repair saturation again with the column program's own building blocks, so they are the primal's bits.  T, liq and psi of a launch's
// first state are taken to be the closures of the stored U and sat, as k_column_tangent_rich takes them.
// lamU and lamS stay in registers over the taped steps of a launch, newest first; each lane owns its cell, nothing is atomic.
//
// Hydraulic parameters (PARAMS; TRM_OPT_DERIVATIVE_RICHARDS_PARAMS, DESIGN 4.8 "Richards parameters").  The step's transpose holds Kcbar, the
// cotangent of the cell's hydraulic conductivity, and psibar, that of its pressure head; dL/dp of a hydraulic parameter p is the sum over the
// taped steps and the cells of Kcbar dKc/dp + psibar dpsi/dp, plus wpsi dpsi/dp at the stored final state (the fold).  Each lane forms the
// slopes of its own cell from the primal's intermediates (r, u, g, x, xe, ie, t, I_ice), adds its terms to one register per parameter the
// instance reads, newest step first, and carries them from launch to launch through per-cell arrays; k_hyd_param_reduce adds a column's
// cells from the bottom up.
//   psi, Brooks-Corey   theta_res through dr/dtheta_res = (r - 1) / theta_span; psi_s: -r^(-1/lambda), -1 where the primal takes
//                       theta >= por; lambda through the exponent, d(-1/lambda) = dlambda / lambda^2
//   psi, van Genuchten  theta_res through r; alpha: -psi_m / alpha; n through both exponents, d(-1/m) = dn / (n - 1)^2 and
//                       d(1/n) = -dn / n^2; every slope 0 in a saturated cell
//   Kc, linear          K_sat: water / por
//   Kc, Mualem          K_sat: Kc's factors without it, the sign of fabs kept; impedance: -ln 10 (1 - liq) Kc on every path of
//                       ice_impedance; n through e1 = n / (n + 1) and e2 = (n - 1) / n, de1 = dn / (n + 1)^2, de2 = dn / n^2
// The compile-time-exponent instances have the exponent slopes all the same: the instance is chosen by the value.
// Conventions: d(x^a)/da = x^a ln x (fp64 log), and 0 where the power itself is 0 (a frozen cell's x = 0; the Mualem term at x = 1); a
// zero cotangent in front of a slope gives 0 whatever the slope, so zero cotangents give exactly zero gradients and scaling them by a
// power of two scales the gradients bit for bit; a cell the primal flags as an illegal composition gives NaN.  lamU and lamS are
// formed by the operations of the sweep without the parameters: gU and gsat are its bits.
//
// Soil-moisture records (RECORD; TRM_OPT_DERIVATIVE_RICHARDS_RECORD, DESIGN 4.8 "Richards records").  The record is the heat-only path's
// (RecordArgs, RecordSample, record_fetch, record_residual: trm_column_adjoint.hpp), with the taped saturation passed where that path
// passes the temperature: the loss gains 1/2 w (sat_p - sat_obs)^2 on the record's levels at its positions.  Saturation is a state
// variable, so a sample is a cotangent of the state itself: the owning lane adds w (sat_p - sat_obs) to lamS, through no closure, and
// the sample has no direct term in the hydraulic-parameter sums -- they feel it through lamS in the steps below.  Position p < n enters
// right behind adjoint_step_rich of the step at (U_p, sat_p), from the `sat` the loop already holds; position n enters in the fold from
// the stored sat_n, in front of the fold's own terms.  The sums of a cell are therefore in the order sample of n, fold, steps > p, sample
// of p, step p - 1, ..., whatever the launches: gradients, residuals and misfit do not depend on TRM_OPT_STEPS_PER_LAUNCH or on how the
// trm_step_record calls were split.  One lane owns a cell and a position occurs once: nothing is atomic, nothing goes to LDS.
#pragma once
#include "trm_column_adjoint.hpp"
#include "trm_column_tangent_rich.hpp"

namespace trm {

// Fourth kernel argument of k_column_record_rich: slot s of the launch holds U at tape + 2 s slot_elems and sat slot_elems behind it
struct RichTapeArgs {
    double* tape;
    long long slot_elems;     // Nh * Nzp
};
// ... and of k_column_adjoint_rich: the five cotangent fields (lU and lsat carry lam between launches) and the launch's slots
struct RichSweepArgs {
    double *lU, *lsat, *lT, *lliq, *lpsi;
    const double* tape;
    long long slot_elems;
    int fold;                 // 1 in the first launch of a sweep: wT, wliq, wpsi through the closures of the stored state, zero after
};

// The hydraulic parameters in the order of TRM_HYDRAULIC_PARAM_* (which counts from TRM_THERMAL_PARAM_COUNT on)
enum { HP_K_SAT = 0, HP_THETA_RES = 1, HP_BC_PSI_S = 2, HP_BC_LAMBDA = 3, HP_VG_ALPHA = 4, HP_VG_N = 5, HP_IMPEDANCE = 6, HP_COUNT = 7 };
// Fifth kernel argument of k_column_adjoint_rich_params and first of k_hyd_param_reduce: the per-cell accumulators, [Nh][Nzp] each
struct HydParamPtrs {
    double* g[HP_COUNT];
};
// the sums a lane carries, one register pair each (named members, not an array: nothing here is ever indexed at run time); an instance
// touches the parameters its hydraulics read (hyd_param_mask), the others are dead registers
struct HydParamSums {
    double K_sat, theta_res, bc_psi_s, bc_lambda, vg_alpha, vg_n, impedance;
};
// the parameters an instance's hydraulics can read, a bit per HP_*: the reference default reads the Brooks-Corey curve and K_sat, n = 2
// the van Genuchten pair; the run-time instance decides per launch and leaves the sums of the others at their stored zeros
template <int HYD> constexpr unsigned hyd_param_mask();
// a launch's first and last act on the sums: from and to the per-cell arrays `hp` at element e, the parameters of the instance alone
#define TRM_HYD_SUMS(F) F(HP_K_SAT, K_sat) F(HP_THETA_RES, theta_res) F(HP_BC_PSI_S, bc_psi_s) F(HP_BC_LAMBDA, bc_lambda) F(HP_VG_ALPHA, vg_alpha) F(HP_VG_N, vg_n) F(HP_IMPEDANCE, impedance)
// (`fresh`: the first launch of a sweep starts every sum from 0, whatever an earlier sweep left in the arrays)
template <int HYD> TRM_DEV void hyd_sums_load(HydParamSums& acc, const HydParamPtrs& hp, size_t e, bool fresh) {
    constexpr unsigned mask = hyd_param_mask<HYD>();
#define TRM_HYD_LOAD(Q, NAME) acc.NAME = ((mask >> Q & 1u) && !fresh) ? hp.g[Q][e] : 0.0;
    TRM_HYD_SUMS(TRM_HYD_LOAD)
#undef TRM_HYD_LOAD
}
template <int HYD> TRM_DEV void hyd_sums_store(const HydParamSums& acc, const HydParamPtrs& hp, size_t e) {
    constexpr unsigned mask = hyd_param_mask<HYD>();
#define TRM_HYD_STORE(Q, NAME) if (mask >> Q & 1u) hp.g[Q][e] = acc.NAME;
    TRM_HYD_SUMS(TRM_HYD_STORE)
#undef TRM_HYD_STORE
}
// (the loads are waited for where this stands)
template <int HYD> TRM_DEV void hyd_sums_use(const HydParamSums& acc) {
    constexpr unsigned mask = hyd_param_mask<HYD>();
#define TRM_HYD_USE(Q, NAME) if (mask >> Q & 1u) asm volatile("" ::"v"(acc.NAME));
    TRM_HYD_SUMS(TRM_HYD_USE)
#undef TRM_HYD_USE
}
template <int HYD> constexpr unsigned hyd_param_mask() {
    return HYD == HYD_BC_LINEAR ? (1u << HP_K_SAT | 1u << HP_THETA_RES | 1u << HP_BC_PSI_S | 1u << HP_BC_LAMBDA)
         : HYD == HYD_VG_N2   ? (1u << HP_K_SAT | 1u << HP_THETA_RES | 1u << HP_VG_ALPHA | 1u << HP_VG_N | 1u << HP_IMPEDANCE)
                              : (1u << HP_COUNT) - 1u;
}

// the boundary inputs both kernels hold over a launch, as k_column_tangent_rich forms them
TRM_DEV ColumnBC<double> rich_column_bc(const View<double>& v, const LaneInfo& ln, int ii) {
    ColumnBC<double> bc;
    bc.bTb = v.bc.kind[2][0] == 1 ? bcval(v, 2, 0)[ii] : 0.0;
    bc.bTt = v.bc.kind[2][1] == 1 ? bcval(v, 2, 1)[ii] : 0.0;
    bc.has_U = true;
    bc.has_S = true;
    double eU_b = 0.0, eU_t = 0.0, eS_b = 0.0, eS_t = 0.0;
    if (v.bc.kind[0][0] == 2) eU_b = flux_term_bottom_nsz(bcval(v, 0, 0)[ii], v.g);
    if (v.bc.kind[1][0] == 2) eS_b = flux_term_bottom_nsz(bcval(v, 1, 0)[ii], v.g);
    if (v.bc.kind[0][1] == 2) eU_t = -flux_term_top_nsz(bcval(v, 0, 1)[ii], v.g);
    if (v.bc.kind[1][1] == 2) eS_t = -flux_term_top_nsz(bcval(v, 1, 1)[ii], v.g);
    const double tU_term = ln.is_top ? eU_t : 0.0, tS_term = ln.is_top ? eS_t : 0.0;
    bc.flux_U = ln.is_bot ? eU_b : tU_term;
    bc.flux_S = ln.is_bot ? eS_b : tS_term;
    return bc;
}

// `a.nsteps` ForwardEuler steps of the heat + Richards state, (U_k, sat_k) stored into tape slot k before step k: the primal half of
// k_column_tangent_rich, operation for operation, so every array, the per-column water fields and the status are trm_step's bit for bit.
template <int HYD, int LPC>
__global__ void __launch_bounds__(TRM_STEP_BLOCK) k_column_record_rich(View<double> v, DevParams<double> p, ColumnArgs<double> a, RichTapeArgs aa) {
    using NF = double;
    int ii;
    size_t e;
    const LaneInfo ln = derivative_lane<LPC>(v, ii, e);
    const int Nz = v.Nz;
    uint32_t viol = 0;
    bool bad = false;

    Cell<NF> c;
    c.U = v.U[e];
    c.sat = v.sat[e];
    c.psi = v.psi[e];
    c.T = v.T[e];
    c.liq = v.liq[e];
    const LevelGeom<NF> L = level_geom(v, ln.k);
    NF S = v.S[ii];
    const ColumnBC<NF> bc = rich_column_bc(v, ln, ii);

    Cell<NF> n = c;
    Frac<NF> f_new = fractions_unchecked(p, c.sat, c.liq);
    NF gU_out = 0.0, gS_out = 0.0, GS_out = 0.0, z0 = 0.0;
    NF* slot = aa.tape + e;
    for (int step = 0; step < a.nsteps; ++step) {
        if (step > 0) c = n;
        if (ln.act) {
            slot[0] = c.U;
            slot[aa.slot_elems] = c.sat;
        }
        slot += 2 * aa.slot_elems;
        const Frac<NF> f = f_new;
        const Tendency<NF> t = column_tendencies<NF, true, HYD, LPC>(v, p, L, ln, c, bc.bTb, bc.bTt, true, viol, &f);
        NF gU = t.gU, gS = t.gS;
        const NF over = column_advance<NF, true, LPC>(v, L, ln, Nz, bc, c.U, c.sat, gU, gS, a.dt, n, z0, bad);
        GS_out = NF(0) + jl_min(NF(0), S);
        S = (S + GS_out * a.dt) + over;
        f_new = column_closure<NF, true, HYD>(p, L, z0, n, viol);
        gU_out = gU;
        gS_out = gS;
    }
    // hydraulic_conductivity of the new state (a finalizing step: compute_auxiliary!)
    const NF Kc_new = conductivity_hydraulic<NF, HYD, false>(p, n.liq, f_new);
    const NF Kc_new_m = shfl_up1<NF, LPC>(Kc_new);
    const NF Kmin_new = jl_min(Kc_new, Kc_new_m);
    const NF Kf_out = (ln.is_bot || ln.is_top) ? Kc_new : Kmin_new;
    if (ln.act) {
        v.U[e] = n.U;
        v.T[e] = n.T;
        v.liq[e] = n.liq;
        v.sat[e] = n.sat;
        v.psi[e] = n.psi;
        v.G_U[e] = gU_out;
        v.G_sat[e] = gS_out;
        v.Kf[e] = Kf_out;
        if (ln.is_top) {
            v.Kf_top[ii] = Kc_new;
            v.S[ii] = S;
            v.wt[ii] = z0;
            v.G_S[ii] = GS_out;
        }
        viol |= bad ? 1u : 0u;
    }
    if (viol && ln.act) atomicOr(v.status, viol);
}

// The transpose of repair_tangent: `s` is the pre-repair saturation the primal's repair received, `lam` the cotangent of the repaired
// tangent; returns the cotangent of the tangent that went in.  The forward half is repair_tangent's replay of the primal without the
// tangent beside it; it keeps this lane's decision of either pass and the levels each pass walked (wave-uniform).
template <int LPC>
TRM_DEV double repair_transpose(double s, double lam, const LaneInfo& ln, int Nz, const LevelGeom<double>& L) {
    const int k = ln.k;
    const bool is_bot = ln.is_bot, is_top = ln.is_top;
    const unsigned long long m_act = ln.m_act, m_top = ln.m_top, m_bot = ln.m_bot;
    const unsigned long long any_over = wave_ballot(s > 1.0) & m_act & ~m_top;
    const unsigned long long any_bad = any_over | (wave_ballot(s < 0.0) & m_act & ~m_bot);
    s = is_bot ? s : s + 0.0;
    bool d_over = false, d_under = false;
    int o_first = 0, o_last = -1, u_first = 0, u_last = 1;      // (an empty pass: last behind first)
    double dzc = 0.0, dz_up = 0.0, rdz_up = 0.0, dz_dn = 0.0, rdz_dn = 0.0;
    if (any_bad != 0ull) {
        dzc = L.dzc;
        const double rdzc = L.rdzc;
        const double dz_up_n = shfl_dn1<double, LPC>(dzc), rdz_up_n = shfl_dn1<double, LPC>(rdzc);
        const double dz_dn_n = shfl_up1<double, LPC>(dzc), rdz_dn_n = shfl_up1<double, LPC>(rdzc);
        const bool edge_up = k >= Nz - 1;
        dz_up = edge_up ? dzc : dz_up_n;
        rdz_up = edge_up ? rdzc : rdz_up_n;
        dz_dn = is_bot ? dzc : dz_dn_n;
        rdz_dn = is_bot ? rdzc : rdz_dn_n;
        if (any_over != 0ull) {
            const unsigned long long lv = level_bits<LPC>(any_over);
            double carry = 0.0;
            o_first = __builtin_ctzll(lv);
            for (int q = o_first; q < Nz - 1; ++q) {
                double cout = 0.0;
                if (k == q) {
                    s = s + carry;
                    const double x = s - 1.0;
                    const double ex = jl_max(x, 0.0);
                    d_over = x > 0.0;
                    s = s - ex;
                    cout = div_const(ex * dzc, dz_up, rdz_up);
                }
                carry = shfl_from<double, LPC>(cout, q);
                o_last = q;
                if ((lv >> (q + 1)) == 0ull && wave_ballot(!(carry == 0.0)) == 0ull) break;
            }
            if (is_top) s = s + carry;
        }
        const unsigned long long any_under = wave_ballot(!(jl_max(-s, 0.0) == 0.0)) & m_act & ~m_bot;
        if (any_under != 0ull) {
            const unsigned long long lv = level_bits<LPC>(any_under);
            double pend = 0.0;
            u_first = 63 - __builtin_clzll(lv);
            for (int q = u_first; q >= 1; --q) {
                double pout = 0.0;
                if (k == q) {
                    s = s - pend;
                    const double y = -s;
                    const double d = jl_max(y, 0.0);
                    d_under = y > 0.0;
                    s = s + d;
                    pout = div_const(d * dzc, dz_dn, rdz_dn);
                }
                pend = shfl_from<double, LPC>(pout, q);
                u_last = q;
                if ((lv & ((1ull << q) - 1ull)) == 0ull && wave_ballot(!(pend == 0.0)) == 0ull) break;
            }
            if (is_bot) s = s - pend;
        }
    }
    const double x_top = s - 1.0;
    const bool top_over = is_top && x_top > 0.0;
    s = s - (is_top ? jl_max(x_top, 0.0) : 0.0);
    const bool bot_clamp = is_bot && !(s > 0.0);
    // backwards: the clamp leaves nothing of the bottom cell's cotangent, the overflow nothing of the top cell's
    lam = bot_clamp ? 0.0 : lam;
    lam = top_over ? 0.0 : lam;
    // the under-pass, bottom-up: level q handed -(its tangent) w_q down to level q - 1 where y > 0, and kept none of it
    for (int q = u_last; q <= u_first; ++q) {
        const double pb = -shfl_from<double, LPC>(lam, q - 1);
        if (k == q && d_under) lam = -div_const(pb * dzc, dz_dn, rdz_dn);
    }
    // the over-pass, top-down: level q handed its tangent w_q up to level q + 1 where x > 0, and kept none of it
    for (int q = o_last; q >= o_first; --q) {
        const double cb = shfl_from<double, LPC>(lam, q + 1);
        if (k == q && d_over) lam = div_const(cb * dzc, dz_up, rdz_up);
    }
    return lam;
}

// whether conductivity_hydraulic's composition test passes in the cell (hydraulic_conductivity_tangent gives NaN where it does not)
template <int HYD> TRM_DEV bool hydraulic_legal(const DevParams<double>& p, const Frac<double>& f) {
    const bool vg = HYD == HYD_VG_N2 || (HYD == HYD_GENERIC && p.unsat_k != 0);
    if (!vg) return true;
    const double x = div_const(f.water, p.por, p.rpor);
    return x >= 0.0 && x <= 1.0;
}

// The transpose of closure_tangent_rich together with fractions_tangent at (U, sat), whose closure formed liq, T and C.  In: the
// cotangents of dT (Tbar), of dliq (lbar), of the three fraction tangents through finite coefficients (wbar, ibar, abar), and of dwater
// through the hydraulic conductivity's slope (wK: not finite in a frozen or dry cell under van Genuchten-Mualem, where the tangent's
// operand dwater is an exact zero -- such a route gives 0).  Out: their shares of the cotangents of dU and dsat.
TRM_DEV void closure_transpose_rich(const DevParams<double>& p, double U, double sat, double liq, double T, double C, double Tbar, double lbar, double wbar,
                                    double ibar, double abar, double wK, double& uOut, double& sOut) {
    const double Lth = p.L * sat * p.por;
    const double nLth = -Lth;
    const bool thawed = U >= 0.0, frozen = U < nLth;
    const bool phase = !(thawed || frozen || nLth == 0.0);
    const double den = nLth + Limits<double>::eps();
    const double q = div_nr(U, den);
    // dT = (num - T dC) / C
    const double n1 = (thawed || frozen) ? div_nr(Tbar, C) : 0.0;
    const double Cbar = -(T * n1);
    const double w = wbar + p.c_water * Cbar, i = ibar + p.c_ice * Cbar, a = abar + p.c_air * Cbar;
    // dwater = por (dsat liq + sat dliq), dice = por (dsat (1 - liq) - sat dliq), dair = -por dsat
    const double sK = liq == 0.0 ? 0.0 : p.por * (liq * wK);
    const double lK = sat == 0.0 ? 0.0 : p.por * (sat * wK);
    const double sF = p.por * (liq * w + (1.0 - liq) * i) - p.por * a + sK;
    const double lb = lbar + p.por * (sat * w - sat * i) + lK;
    // dliq = -(dU + q dLth) / den in phase change, 0 elsewhere
    const double m = phase ? -div_nr(lb, den) : 0.0;
    const double Lbar = (frozen ? n1 : 0.0) + (phase ? q * m : 0.0);
    uOut = n1 + m;
    sOut = sF + (p.L * p.por) * Lbar;
}

// the cotangent of dpsi onto dsat: the slope is pressure_head_tangent's value at a unit seed
template <int HYD> TRM_DEV double pressure_head_transpose(const DevParams<double>& p, double sat, double psibar) {
    return psibar == 0.0 ? 0.0 : pressure_head_tangent<HYD>(p, sat, 1.0) * psibar;
}

// d(x^a)/da da for xa = x^a as the primal formed it: xa ln x da, and 0 where the power is 0
TRM_DEV double pow_exponent_tangent(double x, double xa, double da) { return xa == 0.0 ? 0.0 : (xa * log(x)) * da; }

// psibar dpsi/dp of pressure_head<double, HYD, true>(p, sat, ...) for the retention curve's parameters: a step's terms of their sums (the
// other members 0).  Terms are formed in locals and leave in one place, so that the sums stay in registers wherever this is inlined.
template <int HYD> TRM_DEV HydParamSums pressure_head_param_terms(const DevParams<double>& p, double sat, double psibar) {
    double t_res = 0.0, t_psi_s = 0.0, t_lam = 0.0, t_alpha = 0.0, t_n = 0.0;
    const double theta = sat * p.por;
    const bool unsat = theta < p.por;
    const bool vg = HYD == HYD_VG_N2 || (HYD == HYD_GENERIC && p.swrc == 1);
    if (psibar != 0.0 && (unsat || !vg)) {
        const double r = div_const_nsz(theta - p.theta_res, p.theta_span, p.rtheta_span);
        const double dr = div_const(r - 1.0, p.theta_span, p.rtheta_span);       // dr/dtheta_res
        if (vg) {
            const double n = HYD == HYD_VG_N2 ? 2.0 : p.vg_n.y;
            double u, g;
            if (HYD == HYD_VG_N2) {
                const double rr = div_nr(1.0, r);
                u = rr * rr;
                g = sqrt_(u - 1.0);
            } else {
                u = jl_pow(r, p.vg_neg_inv_m);
                g = jl_pow(u - 1.0, p.vg_inv_n);
            }
            const double um1 = u - 1.0, nm1 = n - 1.0;
            const double du_r = pow_tangent(r, u, p.vg_neg_inv_m.y, dr);
            // d(-1/m) = dn / (n - 1)^2, d(1/n) = -dn / n^2
            const double du_n = pow_exponent_tangent(r, u, div_nr(1.0, nm1 * nm1));
            const double dg_n = pow_exponent_tangent(um1, g, -div_nr(1.0, n * n)) + pow_tangent(um1, g, p.vg_inv_n.y, du_n);
            t_res = psibar * (p.neg_inv_alpha * pow_tangent(um1, g, p.vg_inv_n.y, du_r));
            t_alpha = psibar * -div_nr(p.neg_inv_alpha * g, p.vg_alpha);
            t_n = psibar * (p.neg_inv_alpha * dg_n);
        } else {
            const double ra = HYD == HYD_BC_LINEAR ? pow_int_m5(r) : jl_pow(r, p.bc_neg_inv_lambda);
            const double lam = p.bc_lambda.y;
            // d(-1/lambda) = dlambda / lambda^2
            const double d_res = -p.bc_psi_s * pow_tangent(r, ra, p.bc_neg_inv_lambda.y, dr);
            const double d_lam = -p.bc_psi_s * pow_exponent_tangent(r, ra, div_nr(1.0, lam * lam));
            t_psi_s = psibar * (unsat ? -ra : -1.0);
            t_res = unsat ? psibar * d_res : 0.0;
            t_lam = unsat ? psibar * d_lam : 0.0;
        }
    }
    return HydParamSums{0.0, t_res, t_psi_s, t_lam, t_alpha, t_n, 0.0};
}

// Kcbar dKc/dp of conductivity_hydraulic<double, HYD, false>(p, liq, f) = Kc for the conductivity's parameters, likewise; `legal`:
// hydraulic_legal of the cell
template <int HYD>
TRM_DEV HydParamSums hydraulic_conductivity_param_terms(const DevParams<double>& p, double liq, const Frac<double>& f, double Kc, double Kcbar, bool legal) {
    const bool vg = HYD == HYD_VG_N2 || (HYD == HYD_GENERIC && p.unsat_k != 0);
    const bool zero = Kcbar == 0.0;
    double t_ksat, t_n = 0.0, t_imp = 0.0;
    if (!vg) {
        t_ksat = zero ? 0.0 : Kcbar * div_nr(f.water, f.water + f.ice + f.air);
    } else {
        const double n = HYD == HYD_VG_N2 ? 2.0 : p.vg_n.y;
        const double x = div_const(f.water, p.por, p.rpor);
        const double I_ice = ice_impedance(p, liq);
        double xe, ie;
        if (HYD == HYD_VG_N2) {
            const double c = cbrt_(x);
            xe = c * c;
            ie = sqrt_(1.0 - xe);
        } else {
            xe = jl_pow(x, p.vgk_e1);
            ie = jl_pow(1.0 - xe, p.vgk_e2);
        }
        const double inner = 1.0 - xe, t = 1.0 - ie;
        const double sx = sqrt_(x), tt = t * t;
        const double B = I_ice * sx * tt, A = p.K_sat * B;
        // de1 = dn / (n + 1)^2, de2 = dn / n^2
        const double np1 = n + 1.0;
        const double dinner = -pow_exponent_tangent(x, xe, div_nr(1.0, np1 * np1));
        const double dt = -(pow_exponent_tangent(inner, ie, div_nr(1.0, n * n)) + pow_tangent(inner, ie, p.vgk_e2.y, dinner));
        const double dA_n = p.K_sat * (I_ice * sx * (2.0 * t * dt));
        const double d_ksat = A < 0.0 ? -B : B;
        const double d_n = A < 0.0 ? -dA_n : dA_n;
        const double d_imp = -((2.302585092994046 * (1.0 - liq)) * Kc);
        const double nan = Limits<double>::nan();
        t_ksat = legal ? (zero ? 0.0 : Kcbar * d_ksat) : nan;
        t_n = legal ? (zero ? 0.0 : Kcbar * d_n) : nan;
        t_imp = legal ? (zero ? 0.0 : Kcbar * d_imp) : nan;
    }
    return HydParamSums{t_ksat, 0.0, 0.0, 0.0, 0.0, t_n, t_imp};
}
// acc += t, the parameters of the instance alone
template <int HYD> TRM_DEV void hyd_sums_add(HydParamSums& acc, const HydParamSums& t) {
    constexpr unsigned mask = hyd_param_mask<HYD>();
#define TRM_HYD_ADD(Q, NAME) if (mask >> Q & 1u) acc.NAME = acc.NAME + t.NAME;
    TRM_HYD_SUMS(TRM_HYD_ADD)
#undef TRM_HYD_ADD
}

// PARAMS: the cell's terms of the hydraulic-parameter gradients go onto `acc` beside it
template <int HYD, int LPC, bool PARAMS = false>
TRM_DEV void adjoint_step_rich(const View<double>& v, const DevParams<double>& p, const LevelGeom<double>& L, const LaneInfo& ln, int Nz, double U, double sat,
                               double dt, const ColumnBC<double>& bc, double& lamU, double& lamS, HydParamSums* acc = nullptr) {
    const bool is_bot = ln.is_bot, is_top = ln.is_top;
    // ---- the primal of the step, by the column program's building blocks
    uint32_t viol = 0;
    Cell<double> c;
    c.U = U;
    c.sat = sat;
    const Frac<double> f = energy_closure_wave<double, 0>(p, U, sat, c.liq, c.T, viol);
    const double z0 = water_table<double, LPC>(sat, ln.m_act, ln.lane, L);
    c.psi = pressure_head<double, HYD, true>(p, sat, L.zC, L.psiz, z0);
    const double C = heat_capacity(p, f);
    const Tendency<double> t = column_tendencies<double, true, HYD, LPC>(v, p, L, ln, c, bc.bTb, bc.bTt, true, viol, &f);
    double gS = t.gS;
    gS += bc.flux_S;
    // ---- the repair, transposed
    const double mS = repair_transpose<LPC>(sat + gS * dt, lamS, ln, Nz, L);
    // ---- the heat faces: the heat-only sweep's under the mirror halo
    const double T = c.T, kap = conductivity(p, f);
    const double T_sh = shfl_up1<double, LPC>(T), kap_sh = shfl_up1<double, LPC>(kap);
    double T_b = T, T_t = T;
    const int kb = v.bc.kind[2][0], kt = v.bc.kind[2][1];
    if (kb == 1) T_b = T + div_const_nsz(T - bc.bTb, v.g.hdzf_bot, v.g.rhdzf_bot) * (-v.g.dzf_bot);
    if (kt == 1) T_t = T + div_const_nsz(bc.bTt - T, v.g.hdzf_top, v.g.rhdzf_top) * v.g.dzf_top;
    const double T_m = is_bot ? T_b : T_sh, kap_m = is_bot ? kap : kap_sh;
    const double mu = lamU * dt * L.rdzc;
    const double mu_sh = shfl_up1<double, LPC>(mu);
    const double phi_lo = is_bot ? mu : mu - mu_sh;
    const double phi_top = -mu;
    const double pA = phi_lo * (-0.5 * ((T - T_m) * L.rdzf_lo));
    const double pB = phi_lo * (-(0.5 * (kap + kap_m)) * L.rdzf_lo);
    const double pA_t = phi_top * (-0.5 * ((T_t - T) * L.rdzf_hi));
    const double pB_t = phi_top * (-(0.5 * (kap + kap)) * L.rdzf_hi);
    const double pA_sh = shfl_dn1<double, LPC>(pA), pB_sh = shfl_dn1<double, LPC>(pB);
    const double pB_val_b = kb == 1 ? -(div_const(pB, v.g.hdzf_bot, v.g.rhdzf_bot) * (-v.g.dzf_bot)) : 0.0;
    const double own_B = is_bot ? pB_val_b : pB;
    const double own_A = is_bot ? pA + pA : pA;
    const double pB_val_t = kt == 1 ? div_const(-pB_t, v.g.hdzf_top, v.g.rhdzf_top) * v.g.dzf_top : 0.0;
    const double up_B = is_top ? pB_val_t : -pB_sh;
    const double up_A = is_top ? pA_t + pA_t : pA_sh;
    const double Tbar = own_B + up_B;
    const double kbar = own_A + up_A;
    // dkappa = 2 s (sk_w dwater + sk_i dice + sk_a dair)
    const double sbar = (2.0 * conductivity_root(p, f)) * kbar;
    const double wbar = sbar * p.sk_water, ibar = sbar * p.sk_ice, abar = sbar * p.sk_air;
    // ---- the Darcy faces: the primal's selections formed again as tendency_tangent_rich forms them
    const double Kc = t.Kc;
    const double Kc_m = shfl_up1<double, LPC>(Kc);
    const bool edge = is_bot || is_top;
    const double Kf_lo = edge ? Kc : jl_min(Kc, Kc_m);
    const double Kf_up = shfl_up1<double, LPC>(Kf_lo), Kf_dn = shfl_dn1<double, LPC>(Kf_lo);
    const double psi_sh = shfl_up1<double, LPC>(c.psi);
    const double Kf_p = is_top ? Kc : Kf_dn;
    const double psi_m = is_bot ? c.psi : psi_sh;
    const double g_lo = (c.psi - psi_m) * L.rdzf_lo;
    const bool down = g_lo < 0.0;
    const double other = down ? Kf_up : Kf_p;
    const double Ks_lo = jl_min(Kf_lo, other);
    // dgS = div_const(-((dqW_hi - dqW_lo) rdzc), por): the cotangent of this lane's lower face flux
    const double muW = div_const(mS * dt, p.por, p.rpor) * L.rdzc;
    const double muW_sh = shfl_up1<double, LPC>(muW);
    const double phiW = is_bot ? muW : muW - muW_sh;
    // dqW_lo = -(dKs_lo g_lo + Ks_lo dg_lo)
    const double Ksbar = -(phiW * g_lo);
    const double gbar = -(phiW * Ks_lo);
    // dg_lo = (dpsi - dpsi_m) rdzf_lo; the bottom cell is its own psi_m
    const double pg = gbar * L.rdzf_lo;
    const double pg_sh = shfl_dn1<double, LPC>(pg);
    const double psibar = (is_bot ? 0.0 : pg) - (is_top ? 0.0 : pg_sh);
    // dKs_lo: min_tangent's first operand is `other` for a negative gradient, Kf_lo else; a tie takes the second
    const bool first = down ? other < Kf_lo : Kf_lo < other;
    const bool to_own = down ? !first : first;
    const double K_own = to_own ? Ksbar : 0.0;
    const double K_up = (down && first) ? Ksbar : 0.0;          // onto dKf_lo of the cell below
    const double K_p = (!down && !first) ? Ksbar : 0.0;         // onto dKf_lo of the cell above; the top cell: onto its own dKc
    const double K_up_sh = shfl_dn1<double, LPC>(K_up), K_p_sh = shfl_up1<double, LPC>(K_p);
    const double Kfbar = K_own + (is_top ? 0.0 : K_up_sh) + (is_bot ? 0.0 : K_p_sh);
    // dKf_lo = dKc at the edges, else min_tangent(Kc, Kc_m, dKc, dKc_m)
    const bool sel_own = edge || Kc < Kc_m;
    const double Kc_own = sel_own ? Kfbar : 0.0;
    const double Kc_dn = sel_own ? 0.0 : Kfbar;                 // onto dKc of the cell below
    const double Kc_dn_sh = shfl_dn1<double, LPC>(Kc_dn);
    const double Kcbar = Kc_own + (is_top ? K_p : Kc_dn_sh);
    // dKc = slope_w dwater + slope_l dliq: the tangent's own values at unit seeds
    const bool legal = hydraulic_legal<HYD>(p, f);
    const double slope_w = hydraulic_conductivity_tangent<HYD>(p, c.liq, f, 1.0, 0.0);
    const double slope_l = hydraulic_conductivity_tangent<HYD>(p, c.liq, f, 0.0, 1.0);
    const double wK = legal ? (Kcbar == 0.0 ? 0.0 : slope_w * Kcbar) : Limits<double>::nan();
    const double lK = legal ? (Kcbar == 0.0 ? 0.0 : slope_l * Kcbar) : Limits<double>::nan();
    // ---- the closures
    double uOut, sOut;
    closure_transpose_rich(p, U, sat, c.liq, T, C, Tbar, lK, wbar, ibar, abar, wK, uOut, sOut);
    lamU = lamU + uOut;
    lamS = mS + sOut + pressure_head_transpose<HYD>(p, sat, psibar);
    if constexpr (PARAMS) {
        hyd_sums_add<HYD>(*acc, hydraulic_conductivity_param_terms<HYD>(p, c.liq, f, Kc, Kcbar, legal));
        hyd_sums_add<HYD>(*acc, pressure_head_param_terms<HYD>(p, sat, psibar));
    }
}

// the sample `s` of the state whose saturation is `sat`: the owning lane writes the residual and adds the sample's cotangent to lamS
TRM_DEV void record_inject_rich(const RecordArgs& r, const RecordSample& s, double sat, double& lamS) {
    const double x = record_residual(r, s, sat);
    lamS = x != 0.0 ? lamS + x : lamS;      // (a gap adds nothing, not even the sign of a zero)
}

// what stands in for `hp` in a sweep without PARAMS (for `r` without RECORD: NoRecord)
struct NoHydParams {};

// The backward sweep over the `a.nsteps` tape slots of this launch, newest first; a.dt is their common dt.
// PARAMS (`hp`: HydParamPtrs, else NoHydParams): the lanes carry the sums of `hp` beside lamU and lamS, from the per-cell arrays and back
// to them (adjoint_step_rich's PARAMS); the first launch of a sweep starts them from 0 and adds the fold's wpsi dpsi/dp at the stored
// final state, behind the fold's own terms.
// RECORD (`r`: RecordArgs, else NoRecord): behind every step's adjoint_step_rich the sample of the step's position, fetched where the
// slot of that step is, a step ahead; the fold takes position `a.nsteps` of the launch (n) in front of its own terms.
// One program for the four kernels below.  Against four bodies of their own (the shape before) its 24 instances have the same occupancy,
// no scratch and at most as many VGPRs, give the same bits, and trm_adjoint_backward takes the same time within the run's noise in all
// six legs of profiles/tools/adjoint_richards_record_cost.py (EXPERIMENTS R30.1, profiles/r30/).
template <int HYD, int LPC, bool PARAMS, bool RECORD, class Hp, class Rec>
TRM_DEV void adjoint_rich_program(const View<double>& v, const DevParams<double>& p, const ColumnArgs<double>& a, const RichSweepArgs& aa, const Hp& hp, const Rec& r) {
    using NF = double;
    int ii;
    size_t e;
    const LaneInfo ln = derivative_lane<LPC>(v, ii, e);
    const int Nz = v.Nz;
    NF lamU = aa.lU[e], lamS = aa.lsat[e];
    int j = -1, row_next = -1;
    if constexpr (RECORD) j = ln.act ? r.row_of_level[ln.k] : -1;
    // the newest slot first; the loads of the slot below (RECORD: and of that step's sample) are issued before the arithmetic of a step
    const size_t stride = 2 * (size_t)aa.slot_elems;
    const NF* slot = aa.tape + (size_t)(a.nsteps > 0 ? a.nsteps - 1 : 0) * stride + e;
    NF U_next = a.nsteps > 0 ? slot[0] : 0.0, sat_next = a.nsteps > 0 ? slot[aa.slot_elems] : 0.0;
    RecordSample s_next;
    if constexpr (RECORD) {
        row_next = a.nsteps > 0 ? r.row_of_position[a.nsteps - 1] : -1;
        s_next = record_fetch(r, row_next, j, ii, v.Nh);
    }
    const LevelGeom<NF> L = level_geom(v, ln.k);
    const ColumnBC<NF> bc = rich_column_bc(v, ln, ii);
    HydParamSums acc;
    if constexpr (PARAMS) hyd_sums_load<HYD>(acc, hp, e, aa.fold != 0);
    if (aa.fold) {
        // the end of the run: wT, wliq and wpsi through the closures of the stored (U_n, sat_n); zero after
        const NF U = v.U[e], sat = v.sat[e], wT = aa.lT[e], wliq = aa.lliq[e], wpsi = aa.lpsi[e];
        RecordSample s_fold;
        if constexpr (RECORD) s_fold = record_fetch(r, r.row_of_position[a.nsteps], j, ii, v.Nh);
        uint32_t viol_in = 0;
        NF liq, T, uOut, sOut;
        const Frac<NF> f = energy_closure_wave<NF, 0>(p, U, sat, liq, T, viol_in);
        closure_transpose_rich(p, U, sat, liq, T, heat_capacity(p, f), wT, wliq, 0.0, 0.0, 0.0, 0.0, uOut, sOut);
        if constexpr (RECORD) record_inject_rich(r, s_fold, sat, lamS);
        lamU = lamU + uOut;
        lamS = lamS + sOut + pressure_head_transpose<HYD>(p, sat, wpsi);
        if constexpr (PARAMS) hyd_sums_add<HYD>(acc, pressure_head_param_terms<HYD>(p, sat, wpsi));
        if (ln.act) {
            aa.lT[e] = 0.0;
            aa.lliq[e] = 0.0;
            aa.lpsi[e] = 0.0;
        }
    }
    // Everything loaded so far is used here, in front of the loop: inside it the next slot's two loads (RECORD: and the next sample's) are
    // the only ones in flight, and the wait for them sits where their values are taken, behind the arithmetic of the step
    asm volatile("" ::"v"(lamU), "v"(lamS), "v"(L.rdzc), "v"(L.rdzf_lo), "v"(L.rdzf_hi), "v"(bc.bTb), "v"(bc.bTt), "v"(bc.flux_S));
    if constexpr (RECORD) asm volatile("" ::"v"(j));
    if constexpr (PARAMS) hyd_sums_use<HYD>(acc);
    for (int step = a.nsteps - 1; step >= 0; --step) {
        const NF U = U_next, sat = sat_next;
        const RecordSample s = s_next;
        const int row = row_next;
        if (step > 0) {
            slot -= stride;
            U_next = slot[0];
            sat_next = slot[aa.slot_elems];
            if constexpr (RECORD) {
                row_next = r.row_of_position[step - 1];
                s_next = record_fetch(r, row_next, j, ii, v.Nh);
            }
        }
        adjoint_step_rich<HYD, LPC, PARAMS>(v, p, L, ln, Nz, U, sat, a.dt, bc, lamU, lamS, PARAMS ? &acc : nullptr);
        if constexpr (RECORD)
            if (row >= 0) record_inject_rich(r, s, sat, lamS);
    }
    if (ln.act) {
        aa.lU[e] = lamU;
        aa.lsat[e] = lamS;
        if constexpr (PARAMS) hyd_sums_store<HYD>(acc, hp, e);
    }
}

// the four wrappers of adjoint_rich_program: the sweep alone, with the hydraulic-parameter sums `hp`, with the record `r`, with both
template <int HYD, int LPC>
__global__ void __launch_bounds__(TRM_STEP_BLOCK) k_column_adjoint_rich(View<double> v, DevParams<double> p, ColumnArgs<double> a, RichSweepArgs aa) {
    adjoint_rich_program<HYD, LPC, false, false>(v, p, a, aa, NoHydParams{}, NoRecord{});
}
template <int HYD, int LPC>
__global__ void __launch_bounds__(TRM_STEP_BLOCK) k_column_adjoint_rich_params(View<double> v, DevParams<double> p, ColumnArgs<double> a, RichSweepArgs aa, HydParamPtrs hp) {
    adjoint_rich_program<HYD, LPC, true, false>(v, p, a, aa, hp, NoRecord{});
}
template <int HYD, int LPC>
__global__ void __launch_bounds__(TRM_STEP_BLOCK) k_column_adjoint_rich_record(View<double> v, DevParams<double> p, ColumnArgs<double> a, RichSweepArgs aa, RecordArgs r) {
    adjoint_rich_program<HYD, LPC, false, true>(v, p, a, aa, NoHydParams{}, r);
}
template <int HYD, int LPC>
__global__ void __launch_bounds__(TRM_STEP_BLOCK) k_column_adjoint_rich_params_record(View<double> v, DevParams<double> p, ColumnArgs<double> a, RichSweepArgs aa, HydParamPtrs hp, RecordArgs r) {
    adjoint_rich_program<HYD, LPC, true, true>(v, p, a, aa, hp, r);
}

// trm_adjoint_backward's last launch with the hydraulic-parameter gradients open: one thread per column adds each parameter's cells from
// the bottom up -- out[q][Nh], q in the order of TRM_HYDRAULIC_PARAM_*.  A template, so that only the translation unit that launches it
// holds a copy.
template <class Ptrs> __global__ void __launch_bounds__(256) k_hyd_param_reduce(Ptrs g, double* out, long long Nh, int Nz, int Nzp) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= Nh) return;
    for (int q = 0; q < HP_COUNT; ++q) {
        const double* col = g.g[q] + (size_t)i * (size_t)Nzp;
        double s = 0.0;
        for (int k = 0; k < Nz; ++k) s = s + col[k];
        out[(size_t)q * (size_t)Nh + (size_t)i] = s;
    }
}

}  // namespace trm
