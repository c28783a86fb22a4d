// trm_column_adjoint.hpp -- reverse-mode gradients of the heat-only ForwardEuler run (trm_step_record, trm_adjoint_backward).
//
// The adjoint is the transpose of the linear map k_column_tangent applies (trm_column_tangent.hpp): with the closure slopes
// dT = a dU, dliq = b dU of the branch the primal took and dkappa = c dliq, one forward step is dU' = dU + dt dgU(dT, dliq).  Backwards,
// for the cotangent lam' of dU':
//   mu      = lam' dt rdzc                                   (the cotangent of -(dq_hi - dq_lo))
//   phi     = mu - mu_below  (mu at the bottom face)         (the cotangent of a cell's lower face flux dq_lo; -mu of the top face flux)
//   dq_lo   = A (dkappa + dkappa_m) + B (dT - dT_m),  A = -0.5 (T - T_m) rdzf,  B = -0.5 (kappa + kappa_m) rdzf
//   kappa~  = phi A + (phi A)_above,   T~ = phi B - (phi B)_above
//   lam     = lam' + a T~ + b c kappa~
// The boundary faces use the transposed halo rules: a Value halo extrapolates through a constant (dT - dT_halo = +-dT dzf / (dzf / 2)),
// a Gradient halo copies the edge cell (no term), the mirror policy's halo conductivity is the edge cell's (its A counts twice), the dry
// halo cell of the reference-zero policy has dkappa = 0.  Flux boundary terms are constants.
// The sweeps take what rides along as one template parameter, Ride R (trm_kernels.hpp); SweepArgs<CKPT, R> holds exactly its parts:
//   R                  BCGRAD  SERIES  PGRAD   SweepArgs<CKPT, R> = TapeArgs<CKPT> +
//   RIDE_NONE            -       -       -     nothing
//   RIDE_BC              x       -       -     BcGradPtrs g
//   RIDE_PARAM           x       -       x     BcGradPtrs g, ParamGradPtrs pg
//   RIDE_SERIES          x       x       -     BcGradPtrs g, SeriesGradPtrs sg
//   RIDE_PARAM_SERIES    x       x       x     BcGradPtrs g, SeriesGradPtrs sg, ParamGradPtrs pg
// BCGRAD (ride_has_bc, trm_adjoint_bc_open): the sweep also forms dL/d(boundary value) of the four pairs (temperature, internal-energy flux) x (bottom,
// top), the transposes of the seed terms of k_column_tangent<.., BCSEED>: with pB / pB_t the cotangents of the boundary-face differences
//   Value     top  += div_const(pB_t, dzf / 2) dzf,   bottom += -(div_const(pB, dzf / 2) dzf)
//   Gradient  top  += pB_t dzf,                      bottom += pB dzf
//   Flux      top  += -flux_term_top(lam' dt),       bottom += flux_term_bottom(lam' dt)
// summed in registers of the edge lanes over the taped steps, newest first: the launch that folds starts from 0, every other launch from
// what the launch before stored, and the owning edge lane stores once at the end -- one strictly sequential sum per column and pair,
// whatever the split into launches or segments.  No atomics.  lam is formed by the operations it was.
// PGRAD (ride_has_params, trm_adjoint_param_open, always with BCGRAD): the sweep also forms the cotangents of the eight thermal numbers of DevParams, the
// transposes of the seed terms of k_column_tangent<.., PSEED>, per cell: with T~ and kappa~ of the cell as above, m = -(T / C) and s of
// kappa = s^2,
//   C~ = m T~        onto c_water (x water), c_ice (x ice), c_air (x air), C0          (the fold: m wT of the stored state)
//   s~ = 2 s kappa~  onto sk_water (x water), sk_ice (x ice), sk_air (x air), s0
//   dry halo (reference-zero policy): 2 s_halo pA on the bottom lane, 2 s_halo pA_t on the top lane, onto s0 and (x por) sk_air
// Each lane sums its own cell's eight values in registers over the taped steps, newest first, carried from launch to launch in eight
// fields [Nh][Nzp] like the boundary sums: strictly sequential per cell.  k_param_reduce sums a column's cells in ascending order and
// applies the host's chain rule to the ten parameters.
// SERIES (ride_has_series, TRM_OPT_DERIVATIVE_SERIES, always with BCGRAD; trm_series_derivative.hpp): the record evaluates the boundary series in front of
// every step as column_program<.., SERIES> does; the sweep takes each step's temperature values from the series again (fetched a step
// ahead, with the next tape slot) and a seriesed pair's term goes w1 term onto node n1 and w2 term onto node n2 of a [nt][Nh]
// accumulator instead of the per-column sum: the owning edge lane holds the two sums of the current bracket and stores / loads them
// where a step's row names other nodes, and at the end of the launch.
// PGRAD and SERIES (TRM_OPT_DERIVATIVE_SERIES_PARAMS): both; adjoint_step forms T_m, and with it the dry halo's pA and pA_t that feed the
// sums of s0 and sk_air, from the temperature values the series gave the step, not from the constants loaded in front of the loop.  The
// parameter sums do not feed lam: lam and the node sums are those of the SERIES sweep bit for bit.
// Every coefficient is a function of the state U_k BEFORE step k: k_column_record is the multi-step primal that stores U_k into tape
// slot k (the field layout [Nh][Nzp]) before every step; k_column_adjoint walks a block of slots backwards with lam in registers.
// closure_tangent and conductivity_tangent are linear in their seed, one scalar slope per cell: applied to a cotangent they are their
// own transposes, and the slopes are formed by the tangent's expressions.  No operation has an additive constant, so scaling the
// cotangents by a power of two scales the gradient bit for bit, and a zero cotangent gives a zero gradient.
#pragma once
#include "trm_column_tangent.hpp"

namespace trm {

// Fourth kernel argument of k_column_record (TapeArgs<STRIDED>) and of the sweeps (SweepArgs<CKPT, R>, below).  Either tape:
struct TapeFields {
    double *lU, *lT, *lliq;   // the cotangent fields ([Nh][Nzp] like the state); lU carries lam between launches
    double* tape;             // the slot of the first step of this launch; slot s of the launch at tape + s * slot_elems
    long long slot_elems;     // Nh * Nzp
    int generic;              // 1: Gradient on temperature off the branch-free kinds (k_step_wave's halos, column_tendencies_generic)
    int fold;                 // backward: 1 in the first launch of a sweep: lam_n = wU + a_n wT + b_n wliq of the stored state, wT = wliq = 0 after
};
// ... and, STRIDED (the checkpointed tape, trm_column_adjoint_ckpt.hpp: `tape` is the slot of the record's first store, or the segment's
// checkpoint): the step of the launch that stores first (>= nsteps: none does), and the interval K
template <bool STRIDED> struct TapeArgs : TapeFields {};
template <> struct TapeArgs<true> : TapeFields {
    int first, every;
};
// the boundary-gradient accumulators of a BCGRAD sweep, [Nh] each: dL/d(temperature value) and dL/d(internal-energy flux), bottom / top
struct BcGradPtrs {
    double *gTb, *gTt, *gUb, *gUt;
};
// a lane's running sums (the bottom lane owns Tb and Ub, the top lane Tt and Ut; the other lanes carry zeros)
struct BcGrad {
    double Tb = 0.0, Tt = 0.0, Ub = 0.0, Ut = 0.0;
};
// in front of the loop: 0 in the launch that folds, else what the launch before stored
TRM_DEV BcGrad bc_grad_load(const BcGradPtrs& g, int ii, int fold) {
    BcGrad acc;
    if (!fold) {
        acc.Tb = g.gTb[ii];
        acc.Tt = g.gTt[ii];
        acc.Ub = g.gUb[ii];
        acc.Ut = g.gUt[ii];
    }
    return acc;
}
// behind it: the owning edge lane alone (tail lanes carry clamped copies)
TRM_DEV void bc_grad_store(const BcGradPtrs& g, const LaneInfo& ln, int ii, const BcGrad& acc) {
    if (ln.act && ln.is_bot) {
        g.gTb[ii] = acc.Tb;
        g.gUb[ii] = acc.Ub;
    }
    if (ln.act && ln.is_top) {
        g.gTt[ii] = acc.Tt;
        g.gUt[ii] = acc.Ut;
    }
}

// SERIES, behind adjoint_step: this step's four terms (`term`: zero off the owning lanes) onto the node sums of the seriesed pairs and
// onto the per-column sums of the others
TRM_DEV void series_grad_step(const ColumnArgs<double>& a, const SeriesGradPtrs& g, const LaneInfo& ln, int ii, int step, const BcGrad& term,
                              BcGrad& acc, SeriesGrad& sg) {
    const SeriesTable<double>* tb = a.series;
    const SeriesRow* rows = a.series_rows + (size_t)step * (size_t)a.nseries;
    const bool own_b = ln.act && ln.is_bot, own_t = ln.act && ln.is_top;
    if (tb->base[SLOT_T_BOT]) series_sums_add(sg.s[SLOT_T_BOT], g.gn[SLOT_T_BOT], series_bracket(tb, rows, SLOT_T_BOT), own_b, ii, term.Tb);
    else acc.Tb = acc.Tb + term.Tb;
    if (tb->base[SLOT_T_TOP]) series_sums_add(sg.s[SLOT_T_TOP], g.gn[SLOT_T_TOP], series_bracket(tb, rows, SLOT_T_TOP), own_t, ii, term.Tt);
    else acc.Tt = acc.Tt + term.Tt;
    if (tb->base[SLOT_FU_BOT]) series_sums_add(sg.s[SLOT_FU_BOT], g.gn[SLOT_FU_BOT], series_bracket(tb, rows, SLOT_FU_BOT), own_b, ii, term.Ub);
    else acc.Ub = acc.Ub + term.Ub;
    if (tb->base[SLOT_FU_TOP]) series_sums_add(sg.s[SLOT_FU_TOP], g.gn[SLOT_FU_TOP], series_bracket(tb, rows, SLOT_FU_TOP), own_t, ii, term.Ut);
    else acc.Ut = acc.Ut + term.Ut;
}
// behind the loop: the held sums back to their nodes
TRM_DEV void series_grad_store(const ColumnArgs<double>& a, const SeriesGradPtrs& g, const LaneInfo& ln, int ii, const SeriesGrad& sg) {
    const SeriesTable<double>* tb = a.series;
    const bool own_b = ln.act && ln.is_bot, own_t = ln.act && ln.is_top;
    if (tb->base[SLOT_T_BOT]) series_sums_store(sg.s[SLOT_T_BOT], g.gn[SLOT_T_BOT], own_b, ii);
    if (tb->base[SLOT_T_TOP]) series_sums_store(sg.s[SLOT_T_TOP], g.gn[SLOT_T_TOP], own_t, ii);
    if (tb->base[SLOT_FU_BOT]) series_sums_store(sg.s[SLOT_FU_BOT], g.gn[SLOT_FU_BOT], own_b, ii);
    if (tb->base[SLOT_FU_TOP]) series_sums_store(sg.s[SLOT_FU_TOP], g.gn[SLOT_FU_TOP], own_t, ii);
}

// the per-cell parameter accumulators of a PGRAD sweep, [Nh][Nzp] each, in the order of ParamSeeds
struct ParamGradPtrs {
    double* g[8];
};
// Fourth kernel argument of k_column_adjoint (CKPT = false) / k_column_adjoint_ckpt (true): the tape, then what the ride carries
struct BcGradPart {
    BcGradPtrs g;
};
struct SeriesGradPart {
    SeriesGradPtrs sg;
};
struct ParamGradPart {
    ParamGradPtrs pg;
};
template <bool CKPT, Ride R>
struct SweepArgs : TapeArgs<CKPT>, PartIf<ride_has_bc(R), BcGradPart>, PartIf<ride_has_series(R), SeriesGradPart>, PartIf<ride_has_params(R), ParamGradPart> {};
// a lane's running sums for its own cell
struct ParamGrad {
    double sk_water = 0.0, sk_ice = 0.0, sk_air = 0.0, s0 = 0.0;
    double c_water = 0.0, c_ice = 0.0, c_air = 0.0, C0 = 0.0;
};
// in front of the loop: 0 in the launch that folds, else what the launch before stored
TRM_DEV ParamGrad param_grad_load(const ParamGradPtrs& g, size_t e, int fold) {
    ParamGrad acc;
    if (!fold) {
        acc.sk_water = g.g[0][e];
        acc.sk_ice = g.g[1][e];
        acc.sk_air = g.g[2][e];
        acc.s0 = g.g[3][e];
        acc.c_water = g.g[4][e];
        acc.c_ice = g.g[5][e];
        acc.c_air = g.g[6][e];
        acc.C0 = g.g[7][e];
    }
    return acc;
}
// behind it: every active lane owns its cell
TRM_DEV void param_grad_store(const ParamGradPtrs& g, const LaneInfo& ln, size_t e, const ParamGrad& acc) {
    if (ln.act) {
        g.g[0][e] = acc.sk_water;
        g.g[1][e] = acc.sk_ice;
        g.g[2][e] = acc.sk_air;
        g.g[3][e] = acc.s0;
        g.g[4][e] = acc.c_water;
        g.g[5][e] = acc.c_ice;
        g.g[6][e] = acc.c_air;
        g.g[7][e] = acc.C0;
    }
}
// C~ of a cell onto the heat-capacity sums
TRM_DEV void param_grad_add_C(ParamGrad& acc, const Frac<double>& f, double Cbar) {
    acc.c_water = acc.c_water + Cbar * f.water;
    acc.c_ice = acc.c_ice + Cbar * f.ice;
    acc.c_air = acc.c_air + Cbar * f.air;
    acc.C0 = acc.C0 + Cbar;
}

// `a.nsteps` ForwardEuler steps of the state, U_k stored into tape slot k before step k; the outputs are those of a finalizing trm_step.
// STRIDED (trm_column_adjoint_ckpt.hpp: the record of a checkpointed tape): U_k is stored before the steps
// aa.first, aa.first + aa.every, ... of the launch alone, into the slots from aa.tape on -- a wave-uniform branch, everything else the
// same.  (One kernel template and not a device function under two kernels: behind a call the existing instances came out of the
// register allocator with other registers and three more instructions; as a defaulted template parameter they compile to the code
// they had.)
// SERIES: the seriesed boundary values are formed in front of every step (series_boundary_step), the last step writes them back.
template <int HYD, int LPC, bool STRIDED, bool SERIES>
__global__ void __launch_bounds__(TRM_STEP_BLOCK) k_column_record(View<double> v, DevParams<double> p, ColumnArgs<double> a, TapeArgs<STRIDED> aa) {
    using NF = double;
    int ii;
    size_t e;
    const LaneInfo ln = derivative_lane<LPC>(v, ii, e);
    const bool generic = aa.generic != 0;
    uint32_t viol = 0;
    bool bad = false;

    Cell<NF> c;
    c.U = v.U[e];
    c.sat = v.sat[e];
    c.T = v.T[e];
    c.liq = v.liq[e];
    c.psi = 0.0;
    const LevelGeom<NF> L = level_geom(v, ln.k);
    // boundary inputs: constants over the launch
    NF bTb, bTt;
    temperature_boundary_values<false>(v, ii, generic, bTb, bTt);
    ColumnBC<NF> bc = heat_bc(v, ln, ii, generic, bTb, bTt);

    Cell<NF> n = c;
    Frac<NF> f_new{};
    NF gU_out = 0.0;
    NF* slot = aa.tape + e;
    int next = 0;
    if constexpr (STRIDED) next = aa.first;
    for (int step = 0; step < a.nsteps; ++step) {
        if (step > 0) c = n;
        if constexpr (STRIDED) {
            if (step == next) {
                if (ln.act) *slot = c.U;
                slot += aa.slot_elems;
                next += aa.every;
            }
        } else {
            if (ln.act) *slot = c.U;
            slot += aa.slot_elems;
        }
        if constexpr (SERIES) {
            NF unused_b = 0.0, unused_t = 0.0, unused_U = 0.0;
            series_boundary_step<false, true>(v, a, ln, ii, step, bc, nullptr, unused_b, unused_t, unused_U);
        }
        heat_step<HYD, LPC>(v, p, L, ln, ii, e, generic, bc, a.dt, c, step > 0, f_new, n, gU_out, viol, bad);
    }
    finalize_heat_outputs<HYD, LPC>(v, p, ln, ii, e, n, f_new, gU_out, viol, bad);
}

// the closure quantities a step forms at its state U_k: what an attached record's sample of position k is measured against
struct StepClosure {
    double T, C;
    Frac<double> f;
};
// the transposed step at the state U (the tape's U_k): lam' -> lam.  BCGRAD: and this step's terms onto `acc`; PGRAD: and onto `pacc`;
// KEEP: and T, C and the fractions of the cell into `*keep` (the record-reading sweeps; without it the pointer is not touched)
template <int LPC, bool BCGRAD = false, bool PGRAD = false, bool KEEP = false>
TRM_DEV double adjoint_step(const View<double>& v, const DevParams<double>& p, const LevelGeom<double>& L, const LaneInfo& ln, int ii,
                            double U, double sat, double lam, double dt, double bTb, double bTt, bool generic, BcGrad& acc, ParamGrad& pacc,
                            StepClosure* keep = nullptr) {
    // T, liq, C and kappa of the cell, as the tangent recomputes them
    uint32_t viol_in = 0;
    double liq, T;
    const Frac<double> f = energy_closure_wave<double, 0>(p, U, sat, liq, T, viol_in);
    const double C = heat_capacity(p, f);
    const double kap = conductivity(p, f);
    if constexpr (KEEP) {
        keep->T = T;
        keep->C = C;
        keep->f = f;
    }
    const double T_sh = shfl_up1<double, LPC>(T), kap_sh = shfl_up1<double, LPC>(kap);
    // temperature halos as the primal forms them
    double T_b = T, T_t = T;
    const int kb = v.bc.kind[2][0], kt = v.bc.kind[2][1];
    if (generic) {      // (k_step_wave's halos from the boundary values the kernel has loaded: no load inside the sweep but the tape's)
        T_b = halo_bottom(kb, &bTb, 0, T, v.g);
        T_t = halo_top(kt, &bTt, 0, T, v.g);
    } else {
        if (kb == 1) T_b = T + div_const_nsz(T - bTb, v.g.hdzf_bot, v.g.rhdzf_bot) * (-v.g.dzf_bot);
        if (kt == 1) T_t = T + div_const_nsz(bTt - T, v.g.hdzf_top, v.g.rhdzf_top) * v.g.dzf_top;
    }
    const bool mirror = p.halo_policy == 1;
    const double kap_halo = mirror ? kap : conductivity(p, fractions_unchecked(p, 0.0, liq));
    const double T_m = ln.is_bot ? T_b : T_sh, kap_m = ln.is_bot ? kap_halo : kap_sh;
    // cotangents of the face fluxes
    const double mu = lam * dt * L.rdzc;
    const double mu_sh = shfl_up1<double, LPC>(mu);
    const double phi_lo = ln.is_bot ? mu : mu - mu_sh;
    const double phi_top = -mu;
    // the lower face: pA is the cotangent of (dkappa + dkappa_m), pB of (dT - dT_m)
    const double pA = phi_lo * (-0.5 * ((T - T_m) * L.rdzf_lo));
    const double pB = phi_lo * (-(0.5 * (kap + kap_m)) * L.rdzf_lo);
    // the top boundary face (used by the top lane alone)
    const double pA_t = phi_top * (-0.5 * ((T_t - T) * L.rdzf_hi));
    const double pB_t = phi_top * (-(0.5 * (kap_halo + kap)) * L.rdzf_hi);
    const double pA_sh = shfl_dn1<double, LPC>(pA), pB_sh = shfl_dn1<double, LPC>(pB);
    // own share of the lower face: an interior cell is the `+` side; the bottom cell owns its halo (Value: dT - dT_b = dT dzf / (dzf / 2),
    // else 0; mirror: dkappa_halo = dkappa, else 0)
    const double pB_val_b = kb == 1 ? -(div_const(pB, v.g.hdzf_bot, v.g.rhdzf_bot) * (-v.g.dzf_bot)) : 0.0;
    const double own_B = ln.is_bot ? pB_val_b : pB;
    const double own_A = (ln.is_bot && mirror) ? pA + pA : pA;
    // share of the face above: the cell below a face is its `-` side in dT and its `+` side in dkappa; the top cell owns its halo
    // (Value: dT_t - dT = -dT dzf / (dzf / 2))
    const double pB_val_t = kt == 1 ? div_const(-pB_t, v.g.hdzf_top, v.g.rhdzf_top) * v.g.dzf_top : 0.0;
    const double up_B = ln.is_top ? pB_val_t : -pB_sh;
    const double up_A = ln.is_top ? (mirror ? pA_t + pA_t : pA_t) : pA_sh;
    if constexpr (BCGRAD) {
        double tb = 0.0, tt = 0.0, ub = 0.0, ut = 0.0;
        if (kb == 1) tb = -(div_const(pB, v.g.hdzf_bot, v.g.rhdzf_bot) * v.g.dzf_bot);
        if (kb == 3) tb = pB * v.g.dzf_bot;
        if (kt == 1) tt = div_const(pB_t, v.g.hdzf_top, v.g.rhdzf_top) * v.g.dzf_top;
        if (kt == 3) tt = pB_t * v.g.dzf_top;
        const double lam_dt = lam * dt;
        if (v.bc.kind[0][0] == 2) ub = flux_term_bottom(lam_dt, v.g);
        if (v.bc.kind[0][1] == 2) ut = -flux_term_top(lam_dt, v.g);
        acc.Tb = acc.Tb + (ln.is_bot ? tb : 0.0);
        acc.Ub = acc.Ub + (ln.is_bot ? ub : 0.0);
        acc.Tt = acc.Tt + (ln.is_top ? tt : 0.0);
        acc.Ut = acc.Ut + (ln.is_top ? ut : 0.0);
    }
    const double Tbar = own_B + up_B;
    const double kbar = own_A + up_A;
    if constexpr (PGRAD) {
        param_grad_add_C(pacc, f, closure_param_slope(T, C) * Tbar);
        const double sbar = 2.0 * conductivity_root(p, f) * kbar;
        double s_air = sbar * f.air, s_0 = sbar;
        if (!mirror) {   // the dry halo cells of the edge lanes
            const Frac<double> f_dry = fractions_unchecked(p, 0.0, liq);
            const double two_s = 2.0 * conductivity_root(p, f_dry);
            const double h = (ln.is_bot ? two_s * pA : 0.0) + (ln.is_top ? two_s * pA_t : 0.0);
            s_air = s_air + h * f_dry.air;
            s_0 = s_0 + h;
        }
        pacc.sk_water = pacc.sk_water + sbar * f.water;
        pacc.sk_ice = pacc.sk_ice + sbar * f.ice;
        pacc.sk_air = pacc.sk_air + s_air;
        pacc.s0 = pacc.s0 + s_0;
    }
    // through the slopes: liq~ = c kappa~, U~ = a T~ + b liq~ (closure_tangent and conductivity_tangent are their own transposes)
    const double lbar = conductivity_tangent(p, f, sat * p.por, kbar);
    double via_T, via_liq, unused_liq, unused_T;
    closure_tangent(p, U, sat, C, Tbar, unused_liq, via_T);
    closure_tangent(p, U, sat, C, lbar, via_liq, unused_T);
    return lam + via_T + via_liq;
}

// ---- attached records (trm_adjoint_observe_record; DESIGN 4.8 "Attached records") ----------------------------------------------------
// A temperature record attached to the open adjoint is read inside the backward launches: the loss gains 1/2 w (T_p - T_obs)^2 on the
// record's levels at its positions, and position p is injected by the launch that pulls back step p, right behind that step's
// adjoint_step, from the T, C and fractions the step has formed at U_p (StepClosure): lam gets a_p wT through closure_tangent, a
// parameter sweep closure_param_slope(T, C) wT through param_grad_add_C.  Position n enters with the fold (adjoint_fold's RECORD).
// The fifth kernel argument of the record-reading sweeps.  Lane = level: `row_of_level[Nz]` (-1: not observed) is read once per lane in
// front of the loop; `row_of_position` points at the entry of the launch's first step in the table of the whole tape ([n + 1], -1: no
// sample) and is indexed with the step of the launch, a wave-uniform index, so "is this step observed" is a scalar branch.  Arrays
// [npos][nlevels][Nh]: `observed`, `weight` (null: 1; a weight that is not > 0 counts as 0), and `residual`, where the owning lane
// writes T_p - T_obs (+0 for a gap).  One lane owns a cell and a position occurs once: nothing is atomic.
struct RecordArgs {
    const int32_t* row_of_level;
    const int32_t* row_of_position;
    const double* observed;
    const double* weight;
    double* residual;
    int nlevels;
};
// a lane's sample of one position, fetched a step ahead of its use (with the next tape slot)
struct RecordSample {
    double obs = 0.0, w = 0.0;
    size_t q = 0;
    bool have = false;      // this lane owns a sample of the position
    // w (T - T_obs), +0 for a gap (a NaN sample, a weight that is not > 0) and for a lane without a sample
    TRM_DEV double operator()(double T) const { return (have && obs == obs && w > 0.0) ? w * (T - obs) : 0.0; }
};
// `row`: the position's row of the record (wave-uniform, -1: none); `j`: the lane's row of the level list (-1: none, and for lanes that own no cell)
TRM_DEV RecordSample record_fetch(const RecordArgs& r, int row, int j, int ii, long long Nh) {
    RecordSample s;
    if (row >= 0) {
        s.have = j >= 0;
        if (s.have) {
            s.q = ((size_t)row * (size_t)r.nlevels + (size_t)j) * (size_t)Nh + (size_t)ii;
            s.obs = r.observed[s.q];
            s.w = r.weight ? r.weight[s.q] : 1.0;
        }
    }
    return s;
}
// the residual of the owning lane, and the sample's cotangent wT
TRM_DEV double record_residual(const RecordArgs& r, const RecordSample& s, double T) {
    const double wT = s(T);
    if (s.have) r.residual[s.q] = (s.obs == s.obs && s.w > 0.0) ? T - s.obs : 0.0;
    return wT;
}
// behind adjoint_step of the step at U_p: the sample of position p onto lam and, PGRAD, onto the heat-capacity sums
template <bool PGRAD>
TRM_DEV void record_inject(const DevParams<double>& p, const RecordArgs& r, const RecordSample& s, const StepClosure& cl, double U, double sat, double& lam,
                           ParamGrad& pacc) {
    const double wT = record_residual(r, s, cl.T);
    double via_T, unused_liq;
    closure_tangent(p, U, sat, cl.C, wT, unused_liq, via_T);
    lam = wT != 0.0 ? lam + via_T : lam;      // (a gap adds nothing, not even the sign of a zero)
    if constexpr (PGRAD) param_grad_add_C(pacc, cl.f, closure_param_slope(cl.T, cl.C) * wT);
}

// the end of the run: the cotangents of T_n and liq_n through the closure of the stored U_n, lam_n = wU + a_n wT + b_n wliq; wT = wliq = 0 after.
// PGRAD: and wT through the heat capacity of that closure onto `pacc`.  RECORD: and the cotangent of the record's sample `s` of position
// n, the launch's last, added to the final wT in front of the closure.  (Under `if constexpr` and not a plain parameter: with the
// parameter the parameter sweeps without a record came out of the compiler with the operands of two additions swapped.)
template <bool PGRAD, bool RECORD, class Rec>
TRM_DEV void adjoint_fold(const View<double>& v, const DevParams<double>& p, const LaneInfo& ln, size_t e, double sat, double& lam, double* lT,
                          double* lliq, ParamGrad& pacc, const Rec& r, const RecordSample& s) {
    using NF = double;
    const NF U = v.U[e], wT_final = lT[e], wliq = lliq[e];
    uint32_t viol_in = 0;
    NF liq, T, via_T, via_liq, unused_liq, unused_T;
    const Frac<NF> f = energy_closure_wave<NF, 0>(p, U, sat, liq, T, viol_in);
    const NF C = heat_capacity(p, f);
    NF wT = wT_final;
    if constexpr (RECORD) {
        const NF x = record_residual(r, s, T);
        wT = x != 0.0 ? wT_final + x : wT_final;               // (a gap adds nothing, not even the sign of a zero)
    }
    closure_tangent(p, U, sat, C, wT, unused_liq, via_T);
    closure_tangent(p, U, sat, C, wliq, via_liq, unused_T);
    lam = lam + via_T + via_liq;
    if constexpr (PGRAD) param_grad_add_C(pacc, f, closure_param_slope(T, C) * wT);
    if (ln.act) {
        lT[e] = 0.0;
        lliq[e] = 0.0;
    }
}

// The backward sweep over the `a.nsteps` tape slots of this launch, newest first; a.dt is their common dt.
// BCGRAD: the boundary gradients ride along.  PGRAD: and the per-cell parameter sums.  SERIES: a.series_rows holds the rows of this
// launch's taped steps, oldest first; the step's temperature values are fetched with the tape slot of the step, a step ahead of their use.
// RECORD (`r`: RecordArgs, else NoRecord): and behind every step's adjoint_step the sample of the step's position, fetched where the slot
// of that step is, a step ahead; the fold takes position `a.nsteps` of the launch (n).
template <int HYD, int LPC, Ride R, bool RECORD, class Rec>
TRM_DEV void adjoint_program(const View<double>& v, const DevParams<double>& p, const ColumnArgs<double>& a, const SweepArgs<false, R>& aa, const Rec& r) {
    constexpr bool BCGRAD = ride_has_bc(R), PGRAD = ride_has_params(R), SERIES = ride_has_series(R);
    using NF = double;
    int ii;
    size_t e;
    const LaneInfo ln = derivative_lane<LPC>(v, ii, e);
    const bool generic = aa.generic != 0;
    const NF sat = v.sat[e];
    NF lam = aa.lU[e];
    int j = -1, row_next = -1;
    if constexpr (RECORD) j = ln.act ? r.row_of_level[ln.k] : -1;
    // the newest slot first; the load of the slot below is issued before the arithmetic of a step
    const NF* slot = aa.tape + (size_t)(a.nsteps > 0 ? a.nsteps - 1 : 0) * (size_t)aa.slot_elems + e;
    NF U_next = a.nsteps > 0 ? *slot : 0.0;
    RecordSample s_next;
    if constexpr (RECORD) {
        row_next = a.nsteps > 0 ? r.row_of_position[a.nsteps - 1] : -1;
        s_next = record_fetch(r, row_next, j, ii, v.Nh);
    }
    const LevelGeom<NF> L = level_geom(v, ln.k);
    NF bTb, bTt;
    temperature_boundary_values<true>(v, ii, generic, bTb, bTt);
    ParamGrad pacc;
    if constexpr (PGRAD) pacc = param_grad_load(aa.pg, e, aa.fold);
    if (aa.fold) {
        RecordSample s_fold;
        if constexpr (RECORD) s_fold = record_fetch(r, r.row_of_position[a.nsteps], j, ii, v.Nh);
        adjoint_fold<PGRAD, RECORD>(v, p, ln, e, sat, lam, aa.lT, aa.lliq, pacc, r, s_fold);
    }
    BcGrad acc;
    if constexpr (BCGRAD) acc = bc_grad_load(aa.g, ii, aa.fold);
    // Everything loaded so far is used here, in front of the loop: inside it the next slot's load (SERIES: and the next temperature
    // values', RECORD: and the next sample's) is the only one in flight, and the wait for it sits where its value is taken, behind the
    // arithmetic of the step
    asm volatile("" ::"v"(sat), "v"(lam), "v"(L.rdzc), "v"(L.rdzf_lo), "v"(L.rdzf_hi), "v"(bTb), "v"(bTt));
    if constexpr (RECORD) asm volatile("" ::"v"(j));
    if constexpr (BCGRAD) asm volatile("" ::"v"(acc.Tb), "v"(acc.Tt), "v"(acc.Ub), "v"(acc.Ut));
    if constexpr (PGRAD)
        asm volatile("" ::"v"(pacc.sk_water), "v"(pacc.sk_ice), "v"(pacc.sk_air), "v"(pacc.s0), "v"(pacc.c_water), "v"(pacc.c_ice), "v"(pacc.c_air), "v"(pacc.C0));
    SeriesGrad sg;
    NF bTb_next = bTb, bTt_next = bTt;
    if constexpr (SERIES)
        if (a.nsteps > 0) series_temperatures(a, ii, a.nsteps - 1, bTb_next, bTt_next);
    for (int step = a.nsteps - 1; step >= 0; --step) {
        const NF U = U_next, sTb = bTb_next, sTt = bTt_next;
        const RecordSample s = s_next;
        const int row = row_next;
        if (step > 0) {
            slot -= aa.slot_elems;
            U_next = *slot;
            if constexpr (RECORD) {
                row_next = r.row_of_position[step - 1];
                s_next = record_fetch(r, row_next, j, ii, v.Nh);
            }
            if constexpr (SERIES) series_temperatures(a, ii, step - 1, bTb_next, bTt_next);
        }
        // (SERIES: the step's four terms go through `term` onto the node sums; else adjoint_step adds them onto `acc`)
        StepClosure cl;
        BcGrad term;
        lam = adjoint_step<LPC, BCGRAD, PGRAD, RECORD>(v, p, L, ln, ii, U, sat, lam, a.dt, sTb, sTt, generic, SERIES ? term : acc, pacc, &cl);
        if constexpr (SERIES) series_grad_step(a, aa.sg, ln, ii, step, term, acc, sg);
        if constexpr (RECORD)
            if (row >= 0) record_inject<PGRAD>(p, r, s, cl, U, sat, lam, pacc);
    }
    if constexpr (SERIES) series_grad_store(a, aa.sg, ln, ii, sg);
    if (ln.act) aa.lU[e] = lam;
    if constexpr (BCGRAD) bc_grad_store(aa.g, ln, ii, acc);
    if constexpr (PGRAD) param_grad_store(aa.pg, ln, e, pacc);
}

// the two wrappers of adjoint_program: without and with an attached record
template <int HYD, int LPC, Ride R>
__global__ void __launch_bounds__(TRM_STEP_BLOCK) k_column_adjoint(View<double> v, DevParams<double> p, ColumnArgs<double> a, SweepArgs<false, R> aa) {
    adjoint_program<HYD, LPC, R, false>(v, p, a, aa, NoRecord{});
}
template <int HYD, int LPC, Ride R>
__global__ void __launch_bounds__(TRM_STEP_BLOCK) k_column_adjoint_record(View<double> v, DevParams<double> p, ColumnArgs<double> a, SweepArgs<false, R> aa, RecordArgs r) {
    adjoint_program<HYD, LPC, R, true>(v, p, a, aa, r);
}

// the misfit of an attached record after a sweep: one thread per column sums 1/2 w r^2 over the residuals the sweep wrote, positions in
// ascending order, levels in list order, one term at a time (a weight that is not > 0 counts as 0; a gap's residual is +0).  A template
// like k_param_reduce, so that only the translation unit that launches it holds a copy.
template <class NF> __global__ void __launch_bounds__(256) k_record_misfit(const NF* __restrict__ residual, const NF* __restrict__ weight, NF* __restrict__ out,
                                                       long long Nh, int npos, int nlevels) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= Nh) return;
    double s = 0.0;
    for (int k = 0; k < npos; ++k)
        for (int j = 0; j < nlevels; ++j) {
            const size_t q = ((size_t)k * (size_t)nlevels + (size_t)j) * (size_t)Nh + (size_t)i;
            const double r = residual[q];
            double w = weight ? weight[q] : 1.0;
            if (!(w > 0.0)) w = 0.0;
            s = s + 0.5 * w * r * r;
        }
    out[i] = s;
}

// trm_adjoint_backward's last launch under PGRAD: one thread per column sums each of the eight fields over k = 0 ... Nz-1 in ascending
// order and applies the transposed chain rule of the host (ParamChain: the factors of make_dev_params) -- out[q][Nh], q in the order of
// trm_params (TRM_THERMAL_PARAM_*).  A template, so that only the translation unit that launches it holds a copy.
struct ParamChain {
    double w[10];   // d(derived number) / d(parameter q): 1 / (2 sk_i), frac / (2 sqrt(k)), 1, frac
};
template <class Ptrs> __global__ void __launch_bounds__(256) k_param_reduce(Ptrs g, ParamChain ch, double* out, long long Nh, int Nz, int Nzp) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= Nh) return;
    double sum[8];
    for (int q = 0; q < 8; ++q) {
        const double* col = g.g[q] + (size_t)i * (size_t)Nzp;
        double s = 0.0;
        for (int k = 0; k < Nz; ++k) s = s + col[k];
        sum[q] = s;
    }
    // k_water, k_ice, k_air, k_mineral, k_organic, c_water, c_ice, c_air, c_mineral, c_organic
    const int from[10] = {0, 1, 2, 3, 3, 4, 5, 6, 7, 7};
    for (int q = 0; q < 10; ++q) out[(size_t)q * (size_t)Nh + (size_t)i] = sum[from[q]] * ch.w[q];
}

}  // namespace trm
