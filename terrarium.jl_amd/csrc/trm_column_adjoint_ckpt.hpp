// trm_column_adjoint_ckpt.hpp -- the checkpointed tape of the reverse-mode gradients (trm_adjoint_open_checkpointed).
//
// The per-step tape of trm_column_adjoint.hpp keeps U_k of every step.  Here the record keeps U_c of every K-th step alone (a segment
// start), and the backward launch of a segment of m <= K steps forms the m - 1 states behind its checkpoint again before it walks
// them backwards: the primal step is re-run bit for bit (the library is built -ffp-contract=off, and the step is the sequence of
// column_tendencies / column_advance / column_closure the record ran), so the U_k adjoint_step sees are the recorded ones and the
// gradient is the per-step tape's bit for bit.
// The recomputed states live in dynamic LDS, seg[j * TRM_STEP_BLOCK + threadIdx.x]: 2 KiB per step and workgroup in both layouts.  A
// thread reads back only what it wrote: no barrier.  Lanes are 8 bytes apart: a ds_write_b64 group of 16 lanes covers 32 banks once, a
// ds_read_b64 group of 32 lanes 64 banks once -- conflict-free.
// Restart: (T_c, liq_c, Frac) of a checkpoint are the closure of (U_c, sat), column_closure<double, false, HYD>, which is what the
// record chain entered step c with for every c > 0 (the closure the step before ended with, or its stored result), and for the first
// state of a tape under the contract of trm_step_record: the stored T and liq are the closure of the stored U.
#pragma once
#include "trm_column_adjoint.hpp"

namespace trm {

// lam pulled back through one segment: the checkpoint U_c at ca.tape and the a.nsteps - 1 states behind it under a.dt.
// Dynamic LDS: a.nsteps * TRM_STEP_BLOCK doubles.
// The ride R and its flags are adjoint_program's (the table of trm_column_adjoint.hpp); the fourth argument is SweepArgs<true, R>.
// BCGRAD, PGRAD: the boundary gradients and the per-cell parameter sums as in adjoint_program, added in the same order.
// SERIES: a.series_rows holds the rows of the segment's steps, oldest first; the recompute
// loop evaluates the series as the record did, the backward loop takes the temperature values again and sums onto the nodes.
// PGRAD and SERIES: both, the parameter terms at each recomputed state's series temperatures.
// RECORD (`r`: RecordArgs, trm_column_adjoint.hpp; else NoRecord): and behind the adjoint_step of state j -- U_p is
// mine[j * TRM_STEP_BLOCK] -- the sample of the segment's position j; the fold takes position m of the segment (n).  The sample of a
// step is fetched a step ahead.  Nothing new goes to LDS.
template <int HYD, int LPC, Ride R, bool RECORD, class Rec>
TRM_DEV void adjoint_ckpt_program(const View<double>& v, const DevParams<double>& p, const ColumnArgs<double>& a, const SweepArgs<true, R>& ca, const Rec& r) {
    constexpr bool BCGRAD = ride_has_bc(R), PGRAD = ride_has_params(R), SERIES = ride_has_series(R);
    using NF = double;
    extern __shared__ double seg[];
    int ii;
    size_t e;
    const LaneInfo ln = derivative_lane<LPC>(v, ii, e);
    const bool generic = ca.generic != 0;
    const int m = a.nsteps;
    const NF sat = v.sat[e];
    NF lam = ca.lU[e];
    int jl = -1;
    if constexpr (RECORD) jl = ln.act ? r.row_of_level[ln.k] : -1;
    Cell<NF> c;
    c.U = m > 0 ? ca.tape[e] : 0.0;
    c.sat = sat;
    c.T = 0.0;
    c.liq = 0.0;
    c.psi = 0.0;
    const LevelGeom<NF> L = level_geom(v, ln.k);
    // (the recompute's column form reads the values of a Value condition alone: the sweep's form serves both)
    NF bTb, bTt;
    temperature_boundary_values<true>(v, ii, generic, bTb, bTt);
    ParamGrad pacc;
    if constexpr (PGRAD) pacc = param_grad_load(ca.pg, e, ca.fold);
    if (ca.fold) {
        RecordSample s_fold;
        if constexpr (RECORD) s_fold = record_fetch(r, r.row_of_position[m], jl, ii, v.Nh);
        adjoint_fold<PGRAD, RECORD>(v, p, ln, e, sat, lam, ca.lT, ca.lliq, pacc, r, s_fold);
    }
    BcGrad acc;
    if constexpr (BCGRAD) acc = bc_grad_load(ca.g, ii, ca.fold);

    // ---- recompute: U_c ... U_{c+m-1} into LDS; nothing is stored to memory and no flag is raised (the record run has raised them)
    NF* mine = seg + threadIdx.x;
    if (m > 1) {
        ColumnBC<NF> bc = heat_bc(v, ln, ii, generic, bTb, bTt);
        uint32_t viol = 0;
        bool bad = false;
        NF gU;
        Frac<NF> f = column_closure<NF, false, HYD>(p, L, 0.0, c, viol);
        for (int j = 0; j < m - 1; ++j) {
            mine[j * TRM_STEP_BLOCK] = c.U;
            if constexpr (SERIES) {
                NF unused_b = 0.0, unused_t = 0.0, unused_U = 0.0;
                series_boundary_step<false, false>(v, a, ln, ii, j, bc, nullptr, unused_b, unused_t, unused_U);
            }
            Cell<NF> n;      // (heat_step writes all five fields: column_advance U and sat, column_closure T, liq and psi)
            heat_step<HYD, LPC>(v, p, L, ln, ii, e, generic, bc, a.dt, c, true, f, n, gU, viol, bad);
            c = n;
        }
    }
    if (m > 0) mine[(m - 1) * TRM_STEP_BLOCK] = c.U;

    // ---- backward: the transposed steps at U_{c+m-1} ... U_c, RECORD: each followed by the sample of its position
    SeriesGrad sg;
    NF sTb = bTb, sTt = bTt;
    if constexpr (SERIES)
        if (m > 0) series_temperatures(a, ii, m - 1, sTb, sTt);
    int row_next = -1;
    RecordSample s_next;
    if constexpr (RECORD) {
        row_next = m > 0 ? r.row_of_position[m - 1] : -1;
        s_next = record_fetch(r, row_next, jl, ii, v.Nh);
    }
    for (int j = m - 1; j >= 0; --j) {
        const NF uTb = sTb, uTt = sTt;
        const RecordSample s = s_next;
        const int row = row_next;
        if (j > 0) {
            if constexpr (RECORD) {
                row_next = r.row_of_position[j - 1];
                s_next = record_fetch(r, row_next, jl, ii, v.Nh);
            }
            if constexpr (SERIES) series_temperatures(a, ii, j - 1, sTb, sTt);
        }
        const NF U = mine[j * TRM_STEP_BLOCK];
        StepClosure cl;
        BcGrad term;
        lam = adjoint_step<LPC, BCGRAD, PGRAD, RECORD>(v, p, L, ln, ii, U, sat, lam, a.dt, uTb, uTt, generic, SERIES ? term : acc, pacc, &cl);
        if constexpr (SERIES) series_grad_step(a, ca.sg, ln, ii, j, term, acc, sg);
        if constexpr (RECORD)
            if (row >= 0) record_inject<PGRAD>(p, r, s, cl, U, sat, lam, pacc);
    }
    if constexpr (SERIES) series_grad_store(a, ca.sg, ln, ii, sg);
    if (ln.act) ca.lU[e] = lam;
    if constexpr (BCGRAD) bc_grad_store(ca.g, ln, ii, acc);
    if constexpr (PGRAD) param_grad_store(ca.pg, ln, e, pacc);
}

// the two wrappers of adjoint_ckpt_program: without and with an attached record
template <int HYD, int LPC, Ride R>
__global__ void __launch_bounds__(TRM_STEP_BLOCK) k_column_adjoint_ckpt(View<double> v, DevParams<double> p, ColumnArgs<double> a, SweepArgs<true, R> ca) {
    adjoint_ckpt_program<HYD, LPC, R, false>(v, p, a, ca, NoRecord{});
}
template <int HYD, int LPC, Ride R>
__global__ void __launch_bounds__(TRM_STEP_BLOCK) k_column_adjoint_ckpt_record(View<double> v, DevParams<double> p, ColumnArgs<double> a, SweepArgs<true, R> ca, RecordArgs r) {
    adjoint_ckpt_program<HYD, LPC, R, true>(v, p, a, ca, r);
}

}  // namespace trm
