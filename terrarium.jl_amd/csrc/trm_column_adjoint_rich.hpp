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
#pragma once
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

// the transposed step at the taped state (U, sat): (lamU, lamS) of the state after the step -> of the state before it
template <int HYD, int LPC>
TRM_DEV void adjoint_step_rich(const View<double>& v, const DevParams<double>& p, const LevelGeom<double>& L, const LaneInfo& ln, int Nz, double U, double sat,
                               double dt, const ColumnBC<double>& bc, double& lamU, double& lamS) {
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
}

// The backward sweep over the `a.nsteps` tape slots of this launch, newest first; a.dt is their common dt.
template <int HYD, int LPC>
__global__ void __launch_bounds__(TRM_STEP_BLOCK) k_column_adjoint_rich(View<double> v, DevParams<double> p, ColumnArgs<double> a, RichSweepArgs aa) {
    using NF = double;
    int ii;
    size_t e;
    const LaneInfo ln = derivative_lane<LPC>(v, ii, e);
    const int Nz = v.Nz;
    NF lamU = aa.lU[e], lamS = aa.lsat[e];
    // the newest slot first; the loads of the slot below are issued before the arithmetic of a step
    const size_t stride = 2 * (size_t)aa.slot_elems;
    const NF* slot = aa.tape + (size_t)(a.nsteps > 0 ? a.nsteps - 1 : 0) * stride + e;
    NF U_next = a.nsteps > 0 ? slot[0] : 0.0, sat_next = a.nsteps > 0 ? slot[aa.slot_elems] : 0.0;
    const LevelGeom<NF> L = level_geom(v, ln.k);
    const ColumnBC<NF> bc = rich_column_bc(v, ln, ii);
    if (aa.fold) {
        // the end of the run: wT, wliq and wpsi through the closures of the stored (U_n, sat_n); zero after
        const NF U = v.U[e], sat = v.sat[e], wT = aa.lT[e], wliq = aa.lliq[e], wpsi = aa.lpsi[e];
        uint32_t viol_in = 0;
        NF liq, T, uOut, sOut;
        const Frac<NF> f = energy_closure_wave<NF, 0>(p, U, sat, liq, T, viol_in);
        closure_transpose_rich(p, U, sat, liq, T, heat_capacity(p, f), wT, wliq, 0.0, 0.0, 0.0, 0.0, uOut, sOut);
        lamU = lamU + uOut;
        lamS = lamS + sOut + pressure_head_transpose<HYD>(p, sat, wpsi);
        if (ln.act) {
            aa.lT[e] = 0.0;
            aa.lliq[e] = 0.0;
            aa.lpsi[e] = 0.0;
        }
    }
    // Everything loaded so far is used here, in front of the loop: inside it the next slot's two loads are the only ones in flight, and the
    // wait for them sits where their values are taken, behind the arithmetic of the step
    asm volatile("" ::"v"(lamU), "v"(lamS), "v"(L.rdzc), "v"(L.rdzf_lo), "v"(L.rdzf_hi), "v"(bc.bTb), "v"(bc.bTt), "v"(bc.flux_S));
    for (int step = a.nsteps - 1; step >= 0; --step) {
        const NF U = U_next, sat = sat_next;
        if (step > 0) {
            slot -= stride;
            U_next = slot[0];
            sat_next = slot[aa.slot_elems];
        }
        adjoint_step_rich<HYD, LPC>(v, p, L, ln, Nz, U, sat, a.dt, bc, lamU, lamS);
    }
    if (ln.act) {
        aa.lU[e] = lamU;
        aa.lsat[e] = lamS;
    }
}

}  // namespace trm
