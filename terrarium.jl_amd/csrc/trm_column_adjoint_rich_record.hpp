// trm_column_adjoint_rich_record.hpp -- the backward sweeps of the heat + Richards per-step tape that read an attached soil-moisture
// record inside the launch (TRM_OPT_DERIVATIVE_RICHARDS_RECORD together with TRM_OPT_DERIVATIVE_RICHARDS_ADJOINT; DESIGN 4.8 "Richards
// records").
//
// The record is the heat-only path's (RecordArgs, RecordSample, record_fetch, record_residual: trm_column_adjoint.hpp), with the taped
// saturation passed where that path passes the temperature: the loss gains 1/2 w (sat_p - sat_obs)^2 on the record's levels at its
// positions.  Saturation is a state variable, so a sample is a cotangent of the state itself: the owning lane adds w (sat_p - sat_obs)
// to lamS, through no closure, and the sample has no direct term in the hydraulic-parameter sums -- they feel it through lamS in the
// steps below.  Position p < n enters right behind adjoint_step_rich of the step at (U_p, sat_p), from the `sat` the loop already holds;
// position n enters in the fold from the stored sat_n, in front of the fold's own terms.  The sums of a cell are therefore in the order
// sample of n, fold, steps > p, sample of p, step p - 1, ..., whatever the launches: gradients, residuals and misfit do not depend on
// TRM_OPT_STEPS_PER_LAUNCH or on how the trm_step_record calls were split.  One lane owns a cell and a position occurs once: nothing is
// atomic, nothing goes to LDS.
//
// Kernel bodies of their own beside k_column_adjoint_rich and k_column_adjoint_rich_params, statement for statement: those kernels'
// instances are to stay the ones they are (see k_column_adjoint_rich_params).
#pragma once
#include "trm_column_adjoint.hpp"
#include "trm_column_adjoint_rich.hpp"

namespace trm {

// the sample `s` of the state whose saturation is `sat`: the owning lane writes the residual and adds the sample's cotangent to lamS
TRM_DEV void record_inject_rich(const RecordArgs& r, const RecordSample& s, double sat, double& lamS) {
    const double x = record_residual(r, s, sat);
    lamS = x != 0.0 ? lamS + x : lamS;      // (a gap adds nothing, not even the sign of a zero)
}

// k_column_adjoint_rich with the record `r` as its fifth argument
template <int HYD, int LPC>
__global__ void __launch_bounds__(TRM_STEP_BLOCK) k_column_adjoint_rich_record(View<double> v, DevParams<double> p, ColumnArgs<double> a, RichSweepArgs aa, RecordArgs r) {
    using NF = double;
    int ii;
    size_t e;
    const LaneInfo ln = derivative_lane<LPC>(v, ii, e);
    const int Nz = v.Nz;
    NF lamU = aa.lU[e], lamS = aa.lsat[e];
    const int j = ln.act ? r.row_of_level[ln.k] : -1;
    // the newest slot first; the loads of the slot below, and of that step's sample, are issued before the arithmetic of a step
    const size_t stride = 2 * (size_t)aa.slot_elems;
    const NF* slot = aa.tape + (size_t)(a.nsteps > 0 ? a.nsteps - 1 : 0) * stride + e;
    NF U_next = a.nsteps > 0 ? slot[0] : 0.0, sat_next = a.nsteps > 0 ? slot[aa.slot_elems] : 0.0;
    int row_next = a.nsteps > 0 ? r.row_of_position[a.nsteps - 1] : -1;
    RecordSample s_next = record_fetch(r, row_next, j, ii, v.Nh);
    const LevelGeom<NF> L = level_geom(v, ln.k);
    const ColumnBC<NF> bc = rich_column_bc(v, ln, ii);
    if (aa.fold) {
        // the end of the run: the sample of position n, then wT, wliq and wpsi through the closures of the stored (U_n, sat_n); zero after
        const NF U = v.U[e], sat = v.sat[e], wT = aa.lT[e], wliq = aa.lliq[e], wpsi = aa.lpsi[e];
        const RecordSample s_fold = record_fetch(r, r.row_of_position[a.nsteps], j, ii, v.Nh);
        uint32_t viol_in = 0;
        NF liq, T, uOut, sOut;
        const Frac<NF> f = energy_closure_wave<NF, 0>(p, U, sat, liq, T, viol_in);
        closure_transpose_rich(p, U, sat, liq, T, heat_capacity(p, f), wT, wliq, 0.0, 0.0, 0.0, 0.0, uOut, sOut);
        record_inject_rich(r, s_fold, sat, lamS);
        lamU = lamU + uOut;
        lamS = lamS + sOut + pressure_head_transpose<HYD>(p, sat, wpsi);
        if (ln.act) {
            aa.lT[e] = 0.0;
            aa.lliq[e] = 0.0;
            aa.lpsi[e] = 0.0;
        }
    }
    // Everything loaded so far is used here, in front of the loop: inside it the next slot's two loads and the next sample's are the only
    // ones in flight, and the wait for them sits where their values are taken, behind the arithmetic of the step
    asm volatile("" ::"v"(lamU), "v"(lamS), "v"(L.rdzc), "v"(L.rdzf_lo), "v"(L.rdzf_hi), "v"(bc.bTb), "v"(bc.bTt), "v"(bc.flux_S));
    asm volatile("" ::"v"(j));
    for (int step = a.nsteps - 1; step >= 0; --step) {
        const NF U = U_next, sat = sat_next;
        const RecordSample s = s_next;
        const int row = row_next;
        if (step > 0) {
            slot -= stride;
            U_next = slot[0];
            sat_next = slot[aa.slot_elems];
            row_next = r.row_of_position[step - 1];
            s_next = record_fetch(r, row_next, j, ii, v.Nh);
        }
        adjoint_step_rich<HYD, LPC>(v, p, L, ln, Nz, U, sat, a.dt, bc, lamU, lamS);
        if (row >= 0) record_inject_rich(r, s, sat, lamS);
    }
    if (ln.act) {
        aa.lU[e] = lamU;
        aa.lsat[e] = lamS;
    }
}

// k_column_adjoint_rich_params with the record `r` as its sixth argument.  The sample is kept as RecordSample keeps it -- the observed
// value, the weight and an index -- beside the sums of the parameters.
template <int HYD, int LPC>
__global__ void __launch_bounds__(TRM_STEP_BLOCK) k_column_adjoint_rich_params_record(View<double> v, DevParams<double> p, ColumnArgs<double> a, RichSweepArgs aa, HydParamPtrs hp, RecordArgs r) {
    using NF = double;
    int ii;
    size_t e;
    const LaneInfo ln = derivative_lane<LPC>(v, ii, e);
    const int Nz = v.Nz;
    NF lamU = aa.lU[e], lamS = aa.lsat[e];
    const int j = ln.act ? r.row_of_level[ln.k] : -1;
    const size_t stride = 2 * (size_t)aa.slot_elems;
    const NF* slot = aa.tape + (size_t)(a.nsteps > 0 ? a.nsteps - 1 : 0) * stride + e;
    NF U_next = a.nsteps > 0 ? slot[0] : 0.0, sat_next = a.nsteps > 0 ? slot[aa.slot_elems] : 0.0;
    int row_next = a.nsteps > 0 ? r.row_of_position[a.nsteps - 1] : -1;
    RecordSample s_next = record_fetch(r, row_next, j, ii, v.Nh);
    const LevelGeom<NF> L = level_geom(v, ln.k);
    const ColumnBC<NF> bc = rich_column_bc(v, ln, ii);
    HydParamSums acc;
    hyd_sums_load<HYD>(acc, hp, e, aa.fold != 0);
    if (aa.fold) {
        const NF U = v.U[e], sat = v.sat[e], wT = aa.lT[e], wliq = aa.lliq[e], wpsi = aa.lpsi[e];
        const RecordSample s_fold = record_fetch(r, r.row_of_position[a.nsteps], j, ii, v.Nh);
        uint32_t viol_in = 0;
        NF liq, T, uOut, sOut;
        const Frac<NF> f = energy_closure_wave<NF, 0>(p, U, sat, liq, T, viol_in);
        closure_transpose_rich(p, U, sat, liq, T, heat_capacity(p, f), wT, wliq, 0.0, 0.0, 0.0, 0.0, uOut, sOut);
        record_inject_rich(r, s_fold, sat, lamS);
        lamU = lamU + uOut;
        lamS = lamS + sOut + pressure_head_transpose<HYD>(p, sat, wpsi);
        hyd_sums_add<HYD>(acc, pressure_head_param_terms<HYD>(p, sat, wpsi));
        if (ln.act) {
            aa.lT[e] = 0.0;
            aa.lliq[e] = 0.0;
            aa.lpsi[e] = 0.0;
        }
    }
    asm volatile("" ::"v"(lamU), "v"(lamS), "v"(L.rdzc), "v"(L.rdzf_lo), "v"(L.rdzf_hi), "v"(bc.bTb), "v"(bc.bTt), "v"(bc.flux_S));
    asm volatile("" ::"v"(j));
    hyd_sums_use<HYD>(acc);
    for (int step = a.nsteps - 1; step >= 0; --step) {
        const NF U = U_next, sat = sat_next;
        const RecordSample s = s_next;
        const int row = row_next;
        if (step > 0) {
            slot -= stride;
            U_next = slot[0];
            sat_next = slot[aa.slot_elems];
            row_next = r.row_of_position[step - 1];
            s_next = record_fetch(r, row_next, j, ii, v.Nh);
        }
        adjoint_step_rich<HYD, LPC, true>(v, p, L, ln, Nz, U, sat, a.dt, bc, lamU, lamS, &acc);
        if (row >= 0) record_inject_rich(r, s, sat, lamS);
    }
    if (ln.act) {
        aa.lU[e] = lamU;
        aa.lsat[e] = lamS;
        hyd_sums_store<HYD>(acc, hp, e);
    }
}

}  // namespace trm
