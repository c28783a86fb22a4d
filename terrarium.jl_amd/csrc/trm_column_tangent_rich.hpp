// trm_column_tangent_rich.hpp -- forward-mode tangents of the heat + Richards ForwardEuler step (TRM_OPT_DERIVATIVE_RICHARDS:
// trm_step_tangent and trm_tangent_closure on a context with RichardsEq; DESIGN 4.7 "Richards").
//
// The sibling of k_column_tangent (trm_column_tangent.hpp), a kernel of its own: the state (U, sat, T, liq, psi) and its tangent
// (dU, dsat, dT, dliq, dpsi) with respect to the initial internal energy and the initial saturation advance together, register-resident,
// one soil level per lane, fields and tangents written once per launch.  The primal is computed by the column program's own building
// blocks with RICHARDS = true -- column_tendencies, column_advance (repair_saturation, water_table), column_closure -- and reads and
// stores what the finalizing multi-step launch of trm_step(dt, n, 1) reads and stores, so after trm_step_tangent every array and the
// status are bit-identical to trm_step's.  The tangent is hand-written and follows the branch the primal takes in every cell, which is
// what Enzyme gives the reference (test/differentiability/soil_hydrology_diff.jl).  It is linear in (dU, dsat) with no additive
// constant: scaling both seeds by a power of two scales every tangent bit for bit.
//   fractions    dwater = por (dsat liq + sat dliq), dice = por (dsat (1 - liq) - sat dliq), dair = -por dsat
//   closure      L_theta = L sat por carries dL_theta = L por dsat; thawed: dT = (dU - T dC) / C; frozen: dT = (dU + dL_theta - T dC) / C;
//                phase change: dT = 0 and, with q = U / (-L_theta + eps), dliq = -(dU + q dL_theta) / (-L_theta + eps), 0 where
//                L_theta = 0 (the primal's safediv); dC = c_w dwater + c_i dice + c_a dair
//   conductivity dkappa = 2 s (sk_w dwater + sk_i dice + sk_a dair); the Richards halo is the edge cell (mirror): its tangent is the edge's
//   pressure     dpsi = dpsi_m/dtheta por dsat where the primal takes theta < por, 0 elsewhere; the water table is piecewise constant in
//                the saturation, so the hydrostatic term has tangent 0.  Powers: d(r^a) = a r^a / r dr (pow_tangent), for the
//                compile-time exponents and the run-time ones alike
//   hydraulic K  linear: K_sat dwater / por.  van Genuchten-Mualem: the product rule over I_ice, sqrt(x) and t^2, with
//                dI_ice = ln 10 Omega I_ice dliq on every path (the smooth function's derivative), the sign of fabs kept; a cell the
//                primal flags as an illegal composition (x outside [0, 1]) has NaN tangents
//   faces        the tangent of the operand jl_min / upwind_conductivity select; on a tie the second operand, as Base.min
//   Darcy flux   the product rule; the boundary flux on saturation and vwc_forcing are constants: 0
//   repair       replayed beside the primal's (repair_tangent below): the same operations on a copy of the pre-repair saturation decide the
//                branches, so the primal's bits cannot change.  Every max(x, 0) passes the tangent where x > 0 and gives 0 elsewhere, a
//                tie included: a carry or a deficit that is zero has a zero tangent, and the lane-serial passes cover exactly the levels
//                the primal's cover.  The top overflow removes its tangent from the top cell, the bottom clamp zeroes the bottom cell's.
// A power whose tangent operand is zero has tangent zero, also where a r^a / r is not finite (r = 0: a frozen or dry cell in
// sqrt(x); inner = 0: a saturated cell in the Mualem term, whose derivative is unbounded): zero seeds give exactly zero tangents.
// The tangent of surface_excess_water is NOT carried or stored: nothing in the soil column reads surface_excess_water.
#pragma once
#include "trm_column_tangent.hpp"

namespace trm {

// Fourth kernel argument of k_column_tangent_rich and third of k_closure_tangent_rich: the five tangent fields, [Nh][Nzp] like the state
struct RichTangentArgs {
    double *dU, *dsat, *dT, *dliq, *dpsi;
};

// d(r^a) for ra = r^a as the primal formed it: a ra / r dr, and 0 for dr = 0 wherever the factor is not finite
TRM_DEV double pow_tangent(double r, double ra, double a, double dr) { return dr == 0.0 ? 0.0 : (a * div_nr(ra, r)) * dr; }

struct FracTangent { double water, ice, air; };
TRM_DEV FracTangent fractions_tangent(const DevParams<double>& p, double sat, double liq, double dsat, double dliq) {
    FracTangent d;
    d.water = p.por * (dsat * liq + sat * dliq);
    d.ice = p.por * (dsat * (1.0 - liq) - sat * dliq);
    d.air = -(p.por * dsat);
    return d;
}

// tangent of the energy closure at (U, sat): liq, T and C are what the primal closure formed there
TRM_DEV FracTangent closure_tangent_rich(const DevParams<double>& p, double U, double sat, double liq, double T, double C, double dU, double dsat,
                                         double& dliq, double& dT) {
    const double Lth = p.L * sat * p.por;
    const double nLth = -Lth;
    const double dLth = (p.L * p.por) * dsat;
    const bool thawed = U >= 0.0, frozen = U < nLth;
    const double den = nLth + Limits<double>::eps();
    const double q = div_nr(U, den);
    dliq = (thawed || frozen || nLth == 0.0) ? 0.0 : -div_nr(dU + q * dLth, den);
    const FracTangent d = fractions_tangent(p, sat, liq, dsat, dliq);
    const double dC = p.c_water * d.water + p.c_ice * d.ice + p.c_air * d.air;
    const double num = frozen ? dU + dLth : dU;
    dT = (thawed || frozen) ? div_nr(num - T * dC, C) : 0.0;
    return d;
}

// dkappa of a cell with fractions f
TRM_DEV double conductivity_tangent_rich(const DevParams<double>& p, const Frac<double>& f, const FracTangent& d) {
    return 2.0 * conductivity_root(p, f) * (p.sk_water * d.water + p.sk_ice * d.ice + p.sk_air * d.air);
}

// dpsi of pressure_head<double, HYD, true>(p, sat, ...): the matric term alone
template <int HYD> TRM_DEV double pressure_head_tangent(const DevParams<double>& p, double sat, double dsat) {
    const double theta = sat * p.por, dtheta = dsat * p.por;
    const double r = div_const_nsz(theta - p.theta_res, p.theta_span, p.rtheta_span), dr = div_const(dtheta, p.theta_span, p.rtheta_span);
    const bool vg = HYD == HYD_VG_N2 || (HYD == HYD_GENERIC && p.swrc == 1);
    double dpsi;
    if (vg) {
        double u, g;
        if (HYD == HYD_VG_N2) {
            const double rr = div_nr(1.0, r);
            u = rr * rr;
            g = sqrt_(u - 1.0);
        } else {
            u = jl_pow(r, p.vg_neg_inv_m);
            g = jl_pow(u - 1.0, p.vg_inv_n);
        }
        const double du = pow_tangent(r, u, p.vg_neg_inv_m.y, dr);
        dpsi = p.neg_inv_alpha * pow_tangent(u - 1.0, g, p.vg_inv_n.y, du);
    } else {
        const double ra = HYD == HYD_BC_LINEAR ? pow_int_m5(r) : jl_pow(r, p.bc_neg_inv_lambda);
        dpsi = -p.bc_psi_s * pow_tangent(r, ra, p.bc_neg_inv_lambda.y, dr);
    }
    return theta < p.por ? dpsi : 0.0;
}

// I_ice of conductivity_vg, by its operations
TRM_DEV double ice_impedance(const DevParams<double>& p, double liq) {
    const double y = -p.impedance * (1.0 - liq);
    if (liq == 1.0) return 1.0;
    if (liq == 0.0 && p.impedance_int) return p.I_ice_frozen;
    const double yt = (double)(int)y;
    if (yt == y && y > -4096.0 && y < 4096.0) return pow_int(10.0, (int)y);
    return exp10_frac(y);
}
// dK of conductivity_hydraulic<double, HYD, false>(p, liq, f)
template <int HYD> TRM_DEV double hydraulic_conductivity_tangent(const DevParams<double>& p, double liq, const Frac<double>& f, double dwater, double dliq) {
    const bool vg = HYD == HYD_VG_N2 || (HYD == HYD_GENERIC && p.unsat_k != 0);
    if (!vg) return div_const(p.K_sat * dwater, p.por, p.rpor);
    const double x = div_const(f.water, p.por, p.rpor), dx = div_const(dwater, p.por, p.rpor);
    const double I_ice = ice_impedance(p, liq);
    const double dI = (2.302585092994046 * p.impedance) * I_ice * dliq;
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
    const double dinner = -pow_tangent(x, xe, p.vgk_e1.y, dx);
    const double dt = -pow_tangent(inner, ie, p.vgk_e2.y, dinner);
    const double sx = sqrt_(x), dsx = pow_tangent(x, sx, 0.5, dx);
    const double tt = t * t;
    const double A = p.K_sat * I_ice * sx * tt;
    const double dA = p.K_sat * (dI * sx * tt + I_ice * dsx * tt + I_ice * sx * (2.0 * t * dt));
    const double dK = A < 0.0 ? -dA : dA;
    return (x >= 0.0 && x <= 1.0) ? dK : Limits<double>::nan();
}

// the tangent of the operand jl_min(x, y) selects: x where x < y, else y (a tie: the second operand, as Base.min)
TRM_DEV double min_tangent(double x, double y, double dx, double dy) { return x < y ? dx : dy; }

// (dgU, dgS): the tangents of column_tendencies<double, true, HYD, LPC>'s tendencies of the cell c, without the constant boundary flux terms
// (branch-free boundary kinds).  The primal intermediates are formed again with the primal's operations; f are the cell's fractions, Kc is the primal's t.Kc.
template <int HYD, int LPC>
TRM_DEV void tendency_tangent_rich(const View<double>& v, const DevParams<double>& p, const LevelGeom<double>& L, const LaneInfo& ln, const Cell<double>& c,
                                   const Frac<double>& f, double Kc, double dsat, double dT, double dliq, double dpsi, double bTb, double bTt, double& dgU, double& dgS) {
    const FracTangent d = fractions_tangent(p, c.sat, c.liq, dsat, dliq);
    // ---- heat: tendency_tangent's face fluxes under the mirror halo, dkappa with the saturation's share
    const double kap = conductivity(p, f), dkap = conductivity_tangent_rich(p, f, d);
    const double T_sh = shfl_up1<double, LPC>(c.T), kap_sh = shfl_up1<double, LPC>(kap);
    const double dT_sh = shfl_up1<double, LPC>(dT), dkap_sh = shfl_up1<double, LPC>(dkap);
    double T_b = c.T, T_t = c.T, dT_b = dT, dT_t = dT;
    if (v.bc.kind[2][0] == 1) {
        T_b = c.T + div_const_nsz(c.T - bTb, v.g.hdzf_bot, v.g.rhdzf_bot) * (-v.g.dzf_bot);
        dT_b = dT + div_const(dT, v.g.hdzf_bot, v.g.rhdzf_bot) * (-v.g.dzf_bot);
    }
    if (v.bc.kind[2][1] == 1) {
        T_t = c.T + div_const_nsz(bTt - c.T, v.g.hdzf_top, v.g.rhdzf_top) * v.g.dzf_top;
        dT_t = dT + div_const(-dT, v.g.hdzf_top, v.g.rhdzf_top) * v.g.dzf_top;
    }
    const double T_m = ln.is_bot ? T_b : T_sh, kap_m = ln.is_bot ? kap : kap_sh;
    const double dT_m = ln.is_bot ? dT_b : dT_sh, dkap_m = ln.is_bot ? dkap : dkap_sh;
    const double dq_lo = -(0.5 * (dkap + dkap_m)) * ((c.T - T_m) * L.rdzf_lo) + -(0.5 * (kap + kap_m)) * ((dT - dT_m) * L.rdzf_lo);
    const double dq_sh = shfl_dn1<double, LPC>(dq_lo);
    const double dq_top = -(0.5 * (dkap + dkap)) * ((T_t - c.T) * L.rdzf_hi) + -(0.5 * (kap + kap)) * ((dT_t - dT) * L.rdzf_hi);
    const double dq_hi = ln.is_top ? dq_top : dq_sh;
    dgU = -((dq_hi - dq_lo) * L.rdzc);
    // ---- water: face conductivities, upwinding and the Darcy fluxes as column_tendencies forms them
    const double dKc = hydraulic_conductivity_tangent<HYD>(p, c.liq, f, d.water, dliq);
    const double Kc_m = shfl_up1<double, LPC>(Kc), dKc_m = shfl_up1<double, LPC>(dKc);
    const bool edge = ln.is_bot || ln.is_top;
    const double Kf_lo = edge ? Kc : jl_min(Kc, Kc_m), dKf_lo = edge ? dKc : min_tangent(Kc, Kc_m, dKc, dKc_m);
    const double Kf_up = shfl_up1<double, LPC>(Kf_lo), Kf_dn = shfl_dn1<double, LPC>(Kf_lo);
    const double dKf_up = shfl_up1<double, LPC>(dKf_lo), dKf_dn = shfl_dn1<double, LPC>(dKf_lo);
    const double psi_sh = shfl_up1<double, LPC>(c.psi), dpsi_sh = shfl_up1<double, LPC>(dpsi);
    const double Kf_p = ln.is_top ? Kc : Kf_dn, dKf_p = ln.is_top ? dKc : dKf_dn;
    const double psi_m = ln.is_bot ? c.psi : psi_sh, dpsi_m = ln.is_bot ? dpsi : dpsi_sh;
    const double g_lo = (c.psi - psi_m) * L.rdzf_lo, dg_lo = (dpsi - dpsi_m) * L.rdzf_lo;
    const bool down = g_lo < 0.0;
    const double other = down ? Kf_up : Kf_p, dother = down ? dKf_up : dKf_p;
    // (the reference's operand order: min(K[k-1], K[k]) for a negative gradient, min(K[k], K[k+1]) otherwise -- a tie takes the second)
    const double Ks_lo = jl_min(Kf_lo, other), dKs_lo = down ? min_tangent(other, Kf_lo, dother, dKf_lo) : min_tangent(Kf_lo, other, dKf_lo, dother);
    const double dqW_lo = -(dKs_lo * g_lo + Ks_lo * dg_lo);
    const double dqW_sh = shfl_dn1<double, LPC>(dqW_lo);
    // (the boundary face above the top cell: its head difference is psi - psi, with tangent 0, times min(K, 0) = 0 for a legal K)
    const double dqW_hi = ln.is_top ? 0.0 : dqW_sh;
    dgS = div_const(-((dqW_hi - dqW_lo) * L.rdzc), p.por, p.rpor);
}

// The tangent of repair_saturation<double, LPC>: its operations replayed on `s` (the pre-repair saturation sat0 + gS dt the primal's
// call received) with the tangent `ds` beside them.  `s` leaves as the primal's repaired saturation, bit for bit, and is used for nothing.
template <int LPC>
TRM_DEV double repair_tangent(double s, double ds, const LaneInfo& ln, int Nz, const LevelGeom<double>& L) {
    const int k = ln.k;
    const bool is_bot = ln.is_bot, is_top = ln.is_top;
    const unsigned long long m_act = ln.m_act, m_top = ln.m_top, m_bot = ln.m_bot;
    const unsigned long long any_over = wave_ballot(s > 1.0) & m_act & ~m_top;
    const unsigned long long any_bad = any_over | (wave_ballot(s < 0.0) & m_act & ~m_bot);
    s = is_bot ? s : s + 0.0;
    if (any_bad != 0ull) {
        const double dzc = L.dzc, rdzc = L.rdzc;
        const double dz_up_n = shfl_dn1<double, LPC>(dzc), rdz_up_n = shfl_dn1<double, LPC>(rdzc);
        const double dz_dn_n = shfl_up1<double, LPC>(dzc), rdz_dn_n = shfl_up1<double, LPC>(rdzc);
        const bool edge_up = k >= Nz - 1;
        const double dz_up = edge_up ? dzc : dz_up_n, rdz_up = edge_up ? rdzc : rdz_up_n;
        const double dz_dn = is_bot ? dzc : dz_dn_n, rdz_dn = is_bot ? rdzc : rdz_dn_n;
        if (any_over != 0ull) {
            const unsigned long long lv = level_bits<LPC>(any_over);
            double carry = 0.0, dcarry = 0.0;
            for (int q = __builtin_ctzll(lv); q < Nz - 1; ++q) {
                double cout = 0.0, dcout = 0.0;
                if (k == q) {
                    s = s + carry;
                    ds = ds + dcarry;
                    const double x = s - 1.0;
                    const double e = jl_max(x, 0.0), de = x > 0.0 ? ds : 0.0;
                    s = s - e;
                    ds = ds - de;
                    cout = div_const(e * dzc, dz_up, rdz_up);
                    dcout = div_const(de * dzc, dz_up, rdz_up);
                }
                carry = shfl_from<double, LPC>(cout, q);
                dcarry = shfl_from<double, LPC>(dcout, q);
                if ((lv >> (q + 1)) == 0ull && wave_ballot(!(carry == 0.0)) == 0ull) break;
            }
            if (is_top) {
                s = s + carry;
                ds = ds + dcarry;
            }
        }
        const unsigned long long any_under = wave_ballot(!(jl_max(-s, 0.0) == 0.0)) & m_act & ~m_bot;
        if (any_under != 0ull) {
            const unsigned long long lv = level_bits<LPC>(any_under);
            double pend = 0.0, dpend = 0.0;
            for (int q = 63 - __builtin_clzll(lv); q >= 1; --q) {
                double pout = 0.0, dpout = 0.0;
                if (k == q) {
                    s = s - pend;
                    ds = ds - dpend;
                    const double y = -s;
                    const double d = jl_max(y, 0.0), dd = y > 0.0 ? -ds : 0.0;
                    s = s + d;
                    ds = ds + dd;
                    pout = div_const(d * dzc, dz_dn, rdz_dn);
                    dpout = div_const(dd * dzc, dz_dn, rdz_dn);
                }
                pend = shfl_from<double, LPC>(pout, q);
                dpend = shfl_from<double, LPC>(dpout, q);
                if ((lv & ((1ull << q) - 1ull)) == 0ull && wave_ballot(!(pend == 0.0)) == 0ull) break;
            }
            if (is_bot) {
                s = s - pend;
                ds = ds - dpend;
            }
        }
    }
    // the top overflow takes its tangent with it; the bottom clamp leaves none
    const double x_top = s - 1.0;
    const double e_top = is_top ? jl_max(x_top, 0.0) : 0.0, de_top = (is_top && x_top > 0.0) ? ds : 0.0;
    s = s - e_top;
    ds = ds - de_top;
    ds = (is_bot && !(s > 0.0)) ? 0.0 : ds;
    return ds;
}

// `a.nsteps` ForwardEuler steps of the heat + Richards state and its tangent.  Reads and stores what the finalizing multi-step launch of
// trm_step reads and stores (k_column<double, true, HYD, LPC, DERIVE_NONE, PROG_MULTI, false>: the kinds read at run time, T / liq / psi as
// stored; saturation, pressure head, water table, surface_excess_water, hydraulic conductivity of the new state, the tendencies of the
// last step, the status) and the five tangents.
template <int HYD, int LPC>
__global__ void __launch_bounds__(TRM_STEP_BLOCK) k_column_tangent_rich(View<double> v, DevParams<double> p, ColumnArgs<double> a, RichTangentArgs ta) {
    using NF = double;
    constexpr int CPW = 64 / LPC;
    LaneInfo ln;
    ln.lane = threadIdx.x & 63;
    const int wave = (int)((blockIdx.x * (unsigned)TRM_STEP_BLOCK + threadIdx.x) >> 6);
    ln.k = ln.lane % LPC;
    const int sub = ln.lane / LPC;
    const int Nz = v.Nz, Nh = (int)v.Nh;
    ln.is_bot = ln.k == 0;
    ln.is_top = ln.k == Nz - 1;
    ln.m_bot = wave_ballot(ln.is_bot);
    ln.m_top = wave_ballot(ln.is_top);
    const int i = wave * CPW + sub;
    const bool colok = i < Nh;
    ln.act = colok && ln.k < Nz;
    ln.m_act = wave_ballot(colok) & wave_ballot(ln.k < Nz);
    const int ii = colok ? i : Nh - 1;                   // (tail lanes carry clamped copies and store nothing)
    const size_t e = (size_t)ii * (size_t)v.Nzp + (size_t)(ln.k < Nz ? ln.k : Nz - 1);
    uint32_t viol = 0;
    bool bad = false;

    Cell<NF> c;
    c.U = v.U[e];
    c.sat = v.sat[e];
    c.psi = v.psi[e];
    c.T = v.T[e];
    c.liq = v.liq[e];
    NF dU = ta.dU[e], dsat = ta.dsat[e];
    const LevelGeom<NF> L = level_geom(v, ln.k);
    NF S = v.S[ii];
    // the tangent of the incoming closures (T, liq and psi are the closures of the stored U and sat)
    NF dT, dliq, dpsi;
    {
        uint32_t viol_in = 0;
        NF liq0, T0;
        const Frac<NF> f0 = energy_closure_wave<NF, 0>(p, c.U, c.sat, liq0, T0, viol_in);
        closure_tangent_rich(p, c.U, c.sat, liq0, T0, heat_capacity(p, f0), dU, dsat, dliq, dT);
        dpsi = pressure_head_tangent<HYD>(p, c.sat, dsat);
    }
    // boundary inputs: constants over the launch, the compute_z_bcs! terms as the column program forms them
    ColumnBC<NF> bc;
    bc.bTb = v.bc.kind[2][0] == 1 ? bcval(v, 2, 0)[ii] : 0.0;
    bc.bTt = v.bc.kind[2][1] == 1 ? bcval(v, 2, 1)[ii] : 0.0;
    bc.has_U = true;
    bc.has_S = true;
    {
        NF eU_b = 0.0, eU_t = 0.0, eS_b = 0.0, eS_t = 0.0;
        if (v.bc.kind[0][0] == 2) eU_b = flux_term_bottom_nsz(bcval(v, 0, 0)[ii], v.g);
        if (v.bc.kind[1][0] == 2) eS_b = flux_term_bottom_nsz(bcval(v, 1, 0)[ii], v.g);
        if (v.bc.kind[0][1] == 2) eU_t = -flux_term_top_nsz(bcval(v, 0, 1)[ii], v.g);
        if (v.bc.kind[1][1] == 2) eS_t = -flux_term_top_nsz(bcval(v, 1, 1)[ii], v.g);
        const NF tU_term = ln.is_top ? eU_t : NF(0), tS_term = ln.is_top ? eS_t : NF(0);
        bc.flux_U = ln.is_bot ? eU_b : tU_term;
        bc.flux_S = ln.is_bot ? eS_b : tS_term;
    }

    Cell<NF> n = c;
    // (the fractions of the cell the tendencies see: fractions_unchecked of the stored cell, then the ones the step's closure formed --
    //  the same operands and operations, the same bits: what column_program hands over as `pre`)
    Frac<NF> f_new = fractions_unchecked(p, c.sat, c.liq);
    NF gU_out = 0.0, gS_out = 0.0, GS_out = 0.0, z0 = 0.0;
    for (int step = 0; step < a.nsteps; ++step) {
        if (step > 0) c = n;
        const Frac<NF> f = f_new;
        const Tendency<NF> t = column_tendencies<NF, true, HYD, LPC>(v, p, L, ln, c, bc.bTb, bc.bTt, true, viol, &f);
        NF dgU, dgS;
        tendency_tangent_rich<HYD, LPC>(v, p, L, ln, c, f, t.Kc, dsat, dT, dliq, dpsi, bc.bTb, bc.bTt, dgU, dgS);
        NF gU = t.gU, gS = t.gS;
        const NF over = column_advance<NF, true, LPC>(v, L, ln, Nz, bc, c.U, c.sat, gU, gS, a.dt, n, z0, bad);
        GS_out = NF(0) + jl_min(NF(0), S);
        S = (S + GS_out * a.dt) + over;
        f_new = column_closure<NF, true, HYD>(p, L, z0, n, viol);
        // (gS holds the boundary flux term now: c.sat + gS dt is the saturation the primal's repair received)
        dU = dU + dgU * a.dt;
        dsat = repair_tangent<LPC>(c.sat + gS * a.dt, dsat + dgS * a.dt, ln, Nz, L);
        closure_tangent_rich(p, n.U, n.sat, n.liq, n.T, heat_capacity(p, f_new), dU, dsat, dliq, dT);
        dpsi = pressure_head_tangent<HYD>(p, n.sat, dsat);
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
        ta.dU[e] = dU;
        ta.dsat[e] = dsat;
        ta.dT[e] = dT;
        ta.dliq[e] = dliq;
        ta.dpsi[e] = dpsi;
        viol |= bad ? 1u : 0u;
    }
    if (viol && ln.act) atomicOr(v.status, viol);
}

// trm_tangent_closure on a Richards context: (dT, dliq, dpsi) of the stored (U, sat) and (dU, dsat), one thread per cell of the device layout
template <int HYD> __global__ void __launch_bounds__(256) k_closure_tangent_rich(View<double> v, DevParams<double> p, RichTangentArgs ta) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)v.Nh * (size_t)v.Nzp || (int)(e % (size_t)v.Nzp) >= v.Nz) return;
    const double U = v.U[e], sat = v.sat[e];
    double liq, T;
    uint32_t viol = 0;
    energy_closure(p, U, sat, liq, T, viol);
    const double C = heat_capacity(p, fractions_unchecked(p, sat, liq));
    double dliq, dT;
    closure_tangent_rich(p, U, sat, liq, T, C, ta.dU[e], ta.dsat[e], dliq, dT);
    ta.dT[e] = dT;
    ta.dliq[e] = dliq;
    ta.dpsi[e] = pressure_head_tangent<HYD>(p, sat, ta.dsat[e]);
}

}  // namespace trm
