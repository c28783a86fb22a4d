// trm_column_tangent.hpp -- forward-mode tangents of the heat-only ForwardEuler step (trm_step_tangent, trm_tangent_closure).
//
// The state (U, T, liq) of a SoilModel with NoFlow and its tangent (dU, dT, dliq) with respect to the initial internal energy advance
// together, register-resident, one soil level per lane: the temporal blocking of the multi-step program (PROG_MULTI), fields and
// tangents written once per launch.  The primal is computed by the column program's own building blocks -- column_tendencies (or
// column_tendencies_generic where a Gradient condition on temperature sends trm_step to k_step_wave), column_advance,
// column_closure -- so its bits are those of trm_step.  The tangent is hand-written and follows the branch the primal takes in
// every cell, which is what Enzyme gives the reference (test/differentiability/soil_energy_diff.jl):
//   closure      thawed / frozen: dT = dU / C, dliq = 0;  phase change: dT = 0 (T = 0 there), dliq = -dU / (-L_theta + eps),
//                0 where L_theta = 0 (the primal's safediv).  dC = (c_water - c_ice) sat por dliq vanishes wherever T depends on C.
//   conductivity kappa = s^2 with s = sum_i sqrt(k_i) theta_i:  dkappa = 2 s (sqrt(k_water) dwater + sqrt(k_ice) dice),
//                dwater = sat por dliq = -dice (NoFlow: sat is constant); the dry halo cell of the reference-zero policy has dkappa = 0
//   face flux    qT = -(kappa + kappa_m) / 2 * (T - T_m) * rdz: the product rule, halo values formed as the primal forms them
//   step         dU' = dU + dgU * dt (boundary values are constants: their tangent is 0 -- unless BCSEED, below)
// The kernels take what rides along as one template parameter, Ride R (trm_kernels.hpp), and TangentArgs<R> holds exactly that ride's parts:
//   R                  BCSEED  SERIES  PSEED   TangentArgs<R> = TangentFields +
//   RIDE_NONE            -       -       -     nothing
//   RIDE_BC              x       -       -     BcSeeds
//   RIDE_PARAM           x       -       x     BcSeeds, ParamSeeds s
//   RIDE_SERIES          x       x       -     BcSeeds, SeriesSeeds
//   RIDE_PARAM_SERIES    x       x       x     BcSeeds, SeriesSeeds, ParamSeeds s
// BCSEED (ride_has_bc: trm_tangent_bc_upload has seeded a boundary value): the per-column seeds dbTb, dbTt of the temperature values
// and dF_b, dF_t of the internal-energy fluxes enter where the primal reads the value,
//   Value     dT_t = dT + div_const(dbTt - dT, dzf / 2) dzf,   dT_b = dT + div_const(dT - dbTb, dzf / 2) (-dzf)
//   Gradient  dT_t = dT + dbTt dzf,   dT_b = dT + dbTb (-dzf)   (also where the primal knows a zero Gradient at the bottom and skips it)
//   Flux      dU' = dU + (dgU + dflux_U) dt,  dflux_U = flux_term_bottom(dF_b) on the bottom lane, -flux_term_top(dF_t) on the top lane
// and a pair whose kind reads no value has none.  The primal half is the same code.
// PSEED (ride_has_params: trm_tangent_param_set has seeded a thermal parameter; always together with BCSEED): the seeds of the eight
// numbers DevParams holds -- dsk_i of the square roots sk_i, ds0 of s0 = kterm_mineral + kterm_organic, dc_i, dC0 of C0 = cterm_mineral +
// cterm_organic -- ride in scalar registers and enter where the primal reads the parameter,
//   closure      thawed / frozen: T = N / C with N free of the parameters: dT += m dC_p, m = -(T / C), dC_p = dc_w water + dc_i ice +
//                dc_a air + dC0; phase change: T = 0 and liq is free of C: nothing
//   conductivity dkappa += 2 s (dsk_w water + dsk_i ice + dsk_a air + ds0)
//   dry halo     of the reference-zero policy: s_halo = sk_air por + s0, dkappa_halo = 2 s_halo (dsk_a por + ds0)
// Every tangent operation is linear in (dU, dT, dliq) and the seeds with no additive constant, so scaling the seeds by a power of two
// scales every tangent bit for bit.
// SERIES (ride_has_series, always together with BCSEED; trm_series_derivative.hpp): in front of every step the seriesed pairs among the four
// take the value of their series (the primal: as column_program<.., SERIES>) and the seed s[n1] w1 + s[n2] w2 of seeds shaped like the
// series, [nt][Nh]; a pair without a series keeps its constant value and its per-column seed.
// PSEED and SERIES (RIDE_PARAM_SERIES, TRM_OPT_DERIVATIVE_SERIES_PARAMS): the parameter terms of a step are formed at the boundary
// values the series gave that step -- the Value halos in (T - T_m) of dkappa's product, the dry halo's dkappa_halo -- and both families
// of seeds enter one dgU; the closure terms read no boundary value.
#pragma once
#include "trm_column.hpp"
#include "trm_series_derivative.hpp"

namespace trm {

// A part of a kernel-argument struct that a ride may not carry: the part, or an empty base of a type of its own (it takes no room)
template <class Part> struct Absent {};
template <bool HAS, class Part> using PartIf = std::conditional_t<HAS, Part, Absent<Part>>;

// Fourth kernel argument of k_column_tangent, TangentArgs<R>: the tangent fields ([Nh][Nzp] like the state) and trm_step's halo form,
struct TangentFields {
    double *dU, *dT, *dliq;
    int generic;      // 1: Gradient on temperature off the branch-free kinds (k_step_wave's halos, column_tendencies_generic)
};
// ride_has_bc: and the seeds of the boundary values, [Nh] each,
struct BcSeeds {
    const double *sTb, *sTt;   // d(temperature value) at the bottom / top: of a Value or a Gradient condition
    const double *sUb, *sUt;   // d(internal-energy flux) at the bottom / top
};
// ride_has_series: and the seeds of the seriesed pairs, [nt][Nh] each, by slot (null: the pair has no series)
struct SeriesSeeds {
    const double* sn[4];
};
// ride_has_params: and the seeds of the eight thermal numbers of DevParams (the host's chain rule took the ten parameters there), by value
struct ParamSeeds {
    double dsk_water, dsk_ice, dsk_air, ds0;
    double dc_water, dc_ice, dc_air, dC0;
};
struct ParamSeedsPart {
    ParamSeeds s;
};
template <Ride R>   // (the order a kernel reads by offset: fields, bc, series, params)
struct TangentArgs : TangentFields, PartIf<ride_has_bc(R), BcSeeds>, PartIf<ride_has_series(R), SeriesSeeds>, PartIf<ride_has_params(R), ParamSeedsPart> {};

// tangent of the energy closure at (U, sat) -- C is the heat capacity the primal closure formed
TRM_DEV void closure_tangent(const DevParams<double>& p, double U, double sat, double C, double dU, double& dliq, double& dT) {
    const double Lth = p.L * sat * p.por;
    const double nLth = -Lth;
    const bool thawed = U >= 0.0, frozen = U < nLth;
    dT = (thawed || frozen) ? div_nr(dU, C) : 0.0;
    dliq = (thawed || frozen || nLth == 0.0) ? 0.0 : -div_nr(dU, nLth + Limits<double>::eps());
}

// PSEED: what the heat-capacity seeds add to the closure's dT -- m dC_p with the slope m = -(T / C) (T = 0 in phase change: nothing)
TRM_DEV double closure_param_slope(double T, double C) { return -div_nr(T, C); }
TRM_DEV double heat_capacity_seed(const ParamSeeds& s, const Frac<double>& f) {
    return s.dc_water * f.water + s.dc_ice * f.ice + s.dc_air * f.air + s.dC0;
}
// s of kappa = s^2, as conductivity() forms it
TRM_DEV double conductivity_root(const DevParams<double>& p, const Frac<double>& f) {
    double s = p.sk_water * f.water;
    s = s + p.sk_ice * f.ice;
    s = s + p.sk_air * f.air;
    s = s + p.kterm_mineral;
    s = s + p.kterm_organic;
    return s;
}
// PSEED: what the conductivity seeds add to dkappa of a cell with fractions f
TRM_DEV double conductivity_seed(const DevParams<double>& p, const ParamSeeds& s, const Frac<double>& f) {
    return 2.0 * conductivity_root(p, f) * (s.dsk_water * f.water + s.dsk_ice * f.ice + s.dsk_air * f.air + s.ds0);
}

// dkappa of a cell with fractions f and tangent liquid fraction dliq (wi = sat * por)
TRM_DEV double conductivity_tangent(const DevParams<double>& p, const Frac<double>& f, double wi, double dliq) {
    double s = p.sk_water * f.water;
    s = s + p.sk_ice * f.ice;
    s = s + p.sk_air * f.air;
    s = s + p.kterm_mineral;
    s = s + p.kterm_organic;
    const double dwater = wi * dliq, dice = -(wi * dliq);
    return 2.0 * s * (p.sk_water * dwater + p.sk_ice * dice);
}

// dgU: the tangent of column_tendencies' (or column_tendencies_generic's) heat tendency, without the constant boundary flux terms.
// The primal intermediates (kappa, the halos) are formed again with the primal's operations.  BCSEED: dbTb, dbTt are the column's seeds of
// the temperature boundary values (0 for a kind that reads none).  PSEED: `ps` are the parameter seeds.
template <int LPC, bool BCSEED = false, bool PSEED = false>
TRM_DEV double tendency_tangent(const View<double>& v, const DevParams<double>& p, const LevelGeom<double>& L, const LaneInfo& ln, int ii,
                                const Cell<double>& c, double dT, double dliq, double bTb, double bTt, bool generic, double dbTb = 0.0,
                                double dbTt = 0.0, const ParamSeeds* ps = nullptr) {
    const Frac<double> f = fractions_unchecked(p, c.sat, c.liq);
    const double kap = conductivity(p, f);
    double dkap = conductivity_tangent(p, f, c.sat * p.por, dliq);
    if constexpr (PSEED) dkap = dkap + conductivity_seed(p, *ps, f);
    const double T_sh = shfl_up1<double, LPC>(c.T), kap_sh = shfl_up1<double, LPC>(kap);
    const double dT_sh = shfl_up1<double, LPC>(dT), dkap_sh = shfl_up1<double, LPC>(dkap);
    // temperature halos and their tangents (a Value condition extrapolates through a constant, a Gradient adds one)
    double T_b = c.T, T_t = c.T, dT_b = dT, dT_t = dT;
    const int kb = v.bc.kind[2][0], kt = v.bc.kind[2][1];
    if (generic) {
        T_b = halo_bottom(kb, bcval(v, 2, 0), ii, c.T, v.g);
        T_t = halo_top(kt, bcval(v, 2, 1), ii, c.T, v.g);
    } else {
        if (kb == 1) T_b = c.T + div_const_nsz(c.T - bTb, v.g.hdzf_bot, v.g.rhdzf_bot) * (-v.g.dzf_bot);
        if (kt == 1) T_t = c.T + div_const_nsz(bTt - c.T, v.g.hdzf_top, v.g.rhdzf_top) * v.g.dzf_top;
    }
    if constexpr (BCSEED) {
        if (kb == 1) dT_b = dT + div_const(dT - dbTb, v.g.hdzf_bot, v.g.rhdzf_bot) * (-v.g.dzf_bot);
        if (kt == 1) dT_t = dT + div_const(dbTt - dT, v.g.hdzf_top, v.g.rhdzf_top) * v.g.dzf_top;
        if (kb == 3) dT_b = dT + dbTb * (-v.g.dzf_bot);
        if (kt == 3) dT_t = dT + dbTt * v.g.dzf_top;
    } else {
        if (kb == 1) dT_b = dT + div_const(dT, v.g.hdzf_bot, v.g.rhdzf_bot) * (-v.g.dzf_bot);
        if (kt == 1) dT_t = dT + div_const(-dT, v.g.hdzf_top, v.g.rhdzf_top) * v.g.dzf_top;
    }
    // halo conductivity: the edge cell's under the mirror policy, the dry cell's (sat = 0: no water, no ice) otherwise
    const bool mirror = p.halo_policy == 1;
    const double kap_halo = mirror ? kap : conductivity(p, fractions_unchecked(p, 0.0, c.liq));
    double dkap_halo = mirror ? dkap : 0.0;
    if constexpr (PSEED) {   // (the dry cell's conductivity is constant in the state, not in the parameters)
        const double dkap_dry = conductivity_seed(p, *ps, fractions_unchecked(p, 0.0, c.liq));
        dkap_halo = mirror ? dkap : dkap_dry;
    }
    const double T_m = ln.is_bot ? T_b : T_sh, kap_m = ln.is_bot ? kap_halo : kap_sh;
    const double dT_m = ln.is_bot ? dT_b : dT_sh, dkap_m = ln.is_bot ? dkap_halo : dkap_sh;
    const double dq_lo = -(0.5 * (dkap + dkap_m)) * ((c.T - T_m) * L.rdzf_lo) + -(0.5 * (kap + kap_m)) * ((dT - dT_m) * L.rdzf_lo);
    const double dq_sh = shfl_dn1<double, LPC>(dq_lo);
    const double dq_top = -(0.5 * (dkap_halo + dkap)) * ((T_t - c.T) * L.rdzf_hi) + -(0.5 * (kap_halo + kap)) * ((dT_t - dT) * L.rdzf_hi);
    const double dq_hi = ln.is_top ? dq_top : dq_sh;
    return -((dq_hi - dq_lo) * L.rdzc);
}

// `a.nsteps` ForwardEuler steps of the state and its tangent; the outputs are those of a finalizing trm_step (the tendency of the
// last step, hydraulic_conductivity of the new state) and the three tangents.
// BCSEED: the boundary seeds are loaded once in front of the step loop.  PSEED: the parameter seeds are kernel arguments.  SERIES: values
// and seeds of the seriesed pairs are formed in front of every step; with PSEED the parameter terms take the step's boundary values.
template <int HYD, int LPC, Ride R>
__global__ void __launch_bounds__(TRM_STEP_BLOCK) k_column_tangent(View<double> v, DevParams<double> p, ColumnArgs<double> a, TangentArgs<R> ta) {
    constexpr bool BCSEED = ride_has_bc(R), PSEED = ride_has_params(R), SERIES = ride_has_series(R);
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
    const bool generic = ta.generic != 0;
    uint32_t viol = 0;
    bool bad = false;

    Cell<NF> c;
    c.U = v.U[e];
    c.sat = v.sat[e];
    c.T = v.T[e];
    c.liq = v.liq[e];
    c.psi = 0.0;
    NF dU = ta.dU[e];
    const LevelGeom<NF> L = level_geom(v, ln.k);
    // the tangent of the incoming closure (T and liq are the closure of the stored U)
    NF dT, dliq;
    {
        uint32_t viol_in = 0;
        NF liq0, T0;
        const Frac<NF> f0 = energy_closure_wave<NF, 0>(p, c.U, c.sat, liq0, T0, viol_in);
        const NF C0 = heat_capacity(p, f0);
        closure_tangent(p, c.U, c.sat, C0, dU, dliq, dT);
        if constexpr (PSEED) dT = dT + closure_param_slope(T0, C0) * heat_capacity_seed(ta.s, f0);
    }
    // boundary inputs: constants over the launch
    const NF bTb = v.bc.kind[2][0] == 1 ? bcval(v, 2, 0)[ii] : 0.0, bTt = v.bc.kind[2][1] == 1 ? bcval(v, 2, 1)[ii] : 0.0;
    ColumnBC<NF> bc;
    bc.bTb = bTb;
    bc.bTt = bTt;
    bc.flux_S = 0.0;
    bc.has_U = true;
    bc.has_S = false;
    {   // compute_z_bcs! terms as each program forms them (k_step_wave: flux_term_*; the column program: flux_term_*_nsz, selects)
        const bool bU = v.bc.kind[0][0] == 2, tU = v.bc.kind[0][1] == 2;
        if (generic) {
            NF fU = 0.0;
            if (ln.is_bot && bU) fU = flux_term_bottom(bcval(v, 0, 0)[ii], v.g);
            if (ln.is_top && tU) fU = -flux_term_top(bcval(v, 0, 1)[ii], v.g);
            bc.flux_U = fU;
        } else {
            NF eU_b = 0.0, eU_t = 0.0;
            if (bU) eU_b = flux_term_bottom_nsz(bcval(v, 0, 0)[ii], v.g);
            if (tU) eU_t = -flux_term_top_nsz(bcval(v, 0, 1)[ii], v.g);
            const NF tU_term = ln.is_top ? eU_t : NF(0);
            bc.flux_U = ln.is_bot ? eU_b : tU_term;
        }
    }
    // the seeds of the boundary values this column's kinds read: constants over the launch
    NF dbTb = 0.0, dbTt = 0.0, dflux_U = 0.0;
    if constexpr (BCSEED) {
        const int kb = v.bc.kind[2][0], kt = v.bc.kind[2][1];
        if (kb == 1 || kb == 3) dbTb = ta.sTb[ii];
        if (kt == 1 || kt == 3) dbTt = ta.sTt[ii];
        NF dU_b = 0.0, dU_t = 0.0;
        if (v.bc.kind[0][0] == 2) dU_b = flux_term_bottom(ta.sUb[ii], v.g);
        if (v.bc.kind[0][1] == 2) dU_t = -flux_term_top(ta.sUt[ii], v.g);
        const NF top_term = ln.is_top ? dU_t : NF(0);
        dflux_U = ln.is_bot ? dU_b : top_term;
    }

    const ParamSeeds* ps = nullptr;
    if constexpr (PSEED) ps = &ta.s;
    Cell<NF> n = c;
    Frac<NF> f_new{};
    NF gU_out = 0.0;
    for (int step = 0; step < a.nsteps; ++step) {
        if (step > 0) c = n;
        if constexpr (SERIES) series_boundary_step<true, true>(v, a, ln, ii, step, bc, ta.sn, dbTb, dbTt, dflux_U);
        const Frac<NF>* pre = step > 0 ? &f_new : nullptr;
        const Tendency<NF> t = generic ? column_tendencies_generic<NF, false, HYD, LPC>(v, p, L, ln, c, ii, (unsigned)(e * sizeof(NF)), false, viol)
                                       : column_tendencies<NF, false, HYD, LPC>(v, p, L, ln, c, bc.bTb, bc.bTt, false, viol, pre);
        // (the temperature values: the series' of this step, or the launch's constants)
        const NF dgU = tendency_tangent<LPC, BCSEED, PSEED>(v, p, L, ln, ii, c, dT, dliq, SERIES ? bc.bTb : bTb, SERIES ? bc.bTt : bTt, generic, dbTb, dbTt, ps);
        NF gU = t.gU, gS = t.gS, z0;
        column_advance<NF, false, LPC>(v, L, ln, Nz, bc, c.U, c.sat, gU, gS, a.dt, n, z0, bad);
        f_new = column_closure<NF, false, HYD>(p, L, z0, n, viol);
        if constexpr (BCSEED) dU = dU + (dgU + dflux_U) * a.dt;
        else dU = dU + dgU * a.dt;
        if constexpr (PSEED) {
            const NF C_new = heat_capacity(p, f_new);
            closure_tangent(p, n.U, n.sat, C_new, dU, dliq, dT);
            dT = dT + closure_param_slope(n.T, C_new) * heat_capacity_seed(ta.s, f_new);
        } else closure_tangent(p, n.U, n.sat, heat_capacity(p, f_new), dU, dliq, dT);
        gU_out = gU;
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
        v.G_U[e] = gU_out;
        v.Kf[e] = Kf_out;
        if (ln.is_top) v.Kf_top[ii] = Kc_new;
        ta.dU[e] = dU;
        ta.dT[e] = dT;
        ta.dliq[e] = dliq;
        viol |= bad ? 1u : 0u;
    }
    if (viol && ln.act) atomicOr(v.status, viol);
}

// trm_tangent_closure: (dT, dliq) of the stored (U, sat) and dU, one thread per cell of the device layout.  PSEED (trm_tangent_param_set):
// and the heat-capacity term.  A template, so that only the translation unit that launches it holds a copy.
template <Ride R> __global__ void __launch_bounds__(256) k_closure_tangent(View<double> v, DevParams<double> p, TangentArgs<R> ta) {
    constexpr bool PSEED = ride_has_params(R);
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)v.Nh * (size_t)v.Nzp || (int)(e % (size_t)v.Nzp) >= v.Nz) return;
    const double U = v.U[e], sat = v.sat[e];
    double liq, T;
    uint32_t viol = 0;
    energy_closure(p, U, sat, liq, T, viol);
    Frac<double> f = fractions_unchecked(p, sat, liq);
    const double C = heat_capacity(p, f);
    double dliq, dT;
    closure_tangent(p, U, sat, C, ta.dU[e], dliq, dT);
    if constexpr (PSEED) dT = dT + closure_param_slope(T, C) * heat_capacity_seed(ta.s, f);
    ta.dT[e] = dT;
    ta.dliq[e] = dliq;
}

}  // namespace trm
