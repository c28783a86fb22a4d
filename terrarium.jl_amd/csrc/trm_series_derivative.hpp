// trm_series_derivative.hpp -- boundary time series inside the derivative kernels (TRM_OPT_DERIVATIVE_SERIES; DESIGN 4.7 / 4.8 "Series"),
// and, at the end, the building blocks every heat-only derivative kernel shares (the lane head, the boundary inputs, the primal step, the
// finalising tail).
//
// k_column_tangent, k_column_record, k_column_adjoint and k_column_adjoint_ckpt <.., SERIES> evaluate the boundary series of the four
// pairs the heat-only fast path reads -- SLOT_T_BOT, SLOT_T_TOP (Value), SLOT_FU_BOT, SLOT_FU_TOP (Flux) -- in front of every step, from
// the SeriesTable and the per-step SeriesRows the host lays out, exactly as column_program<.., SERIES> does (trm_column.hpp): the state
// they leave is that of trm_step with the same series, bit for bit.
// A series value is linear in its two bracketing nodes,
//   FieldTimeSeries  x = x2 f + x1 (1 - f)           w2 = f,      w1 = 1 - f
//   Raster           x = x1 + f (x2 - x1) / g        w2 = f / g,  w1 = 1 - w2
//   n1 == n2         x = x1                          w1 = 1, node n1 alone
// Forward: the step's seed is s[n1] w1 + s[n2] w2 of seeds shaped like the series, [nt][Nh] (series_seed).  Backward: the step's term
// of a seriesed pair goes w1 term onto node n1 and w2 term onto node n2 of an accumulator shaped like the series (SeriesNodeSums): the
// owning edge lane holds the two sums of the current bracket in registers and, when a step's row names other nodes, stores them and
// loads the new nodes' sums -- plain loads and stores, one lane per (node, column), launches stream-ordered: no atomics.  A sum always
// continues from the stored value, so each (node, column) sum is one strictly sequential sum, newest step first, whatever the split
// into launches or segments.  No operation adds a constant: scaling seeds or cotangents by a power of two scales the results bit for bit.
#pragma once
#include "trm_column.hpp"

namespace trm {

// the nodes a series' row names at one step and their weights (wave-uniform); n2 < 0: node n1 alone
struct SeriesBracket {
    long long n1, n2;   // element offsets n * Nh
    double w1, w2;
};
TRM_DEV SeriesBracket series_bracket(const SeriesTable<double>* tb, const SeriesRow* rows, int slot) {
    const SeriesRow r = rows[tb->row_of[slot]];
    SeriesBracket b;
    b.n1 = r.n1;
    b.n2 = -1;
    b.w1 = 1.0;
    b.w2 = 0.0;
    if (r.n1 != r.n2) {
        b.n2 = r.n2;
        b.w2 = tb->raster[slot] ? r.f / r.g : r.f;
        b.w1 = 1.0 - b.w2;
    }
    return b;
}
// the tangent of series_value: the step's seed of seeds `s` [nt][Nh]
TRM_DEV double series_seed(const double* s, const SeriesBracket& b, int ii) {
    const double s1 = s[b.n1 + ii];
    if (b.n2 < 0) return s1;
    return s1 * b.w1 + s[b.n2 + ii] * b.w2;
}

// update_inputs! of one step for the seriesed slots among the four (wave-uniform branches): the temperature values and this lane's
// compute_z_bcs! term.  TANGENT: and their seeds, `sn[slot]` [nt][Nh].  WRITEBACK: the last step of the launch leaves the evaluated
// values in the boundary value arrays, as after update_inputs!
template <bool TANGENT, bool WRITEBACK>
TRM_DEV void series_boundary_step(const View<double>& v, const ColumnArgs<double>& a, const LaneInfo& ln, int ii, int step, ColumnBC<double>& bc,
                                  const double* const* sn, double& dbTb, double& dbTt, double& dflux_U) {
    const SeriesTable<double>* tb = a.series;
    const SeriesRow* rows = a.series_rows + (size_t)step * (size_t)a.nseries;
    if (tb->base[SLOT_T_BOT]) {
        bc.bTb = series_value(tb, rows, SLOT_T_BOT, ii);
        if constexpr (TANGENT) dbTb = series_seed(sn[SLOT_T_BOT], series_bracket(tb, rows, SLOT_T_BOT), ii);
    }
    if (tb->base[SLOT_T_TOP]) {
        bc.bTt = series_value(tb, rows, SLOT_T_TOP, ii);
        if constexpr (TANGENT) dbTt = series_seed(sn[SLOT_T_TOP], series_bracket(tb, rows, SLOT_T_TOP), ii);
    }
    if (tb->base[SLOT_FU_BOT]) {
        const double e = flux_term_bottom(series_value(tb, rows, SLOT_FU_BOT, ii), v.g);
        if (ln.is_bot) bc.flux_U = e;
        if constexpr (TANGENT) {
            const double de = flux_term_bottom(series_seed(sn[SLOT_FU_BOT], series_bracket(tb, rows, SLOT_FU_BOT), ii), v.g);
            if (ln.is_bot) dflux_U = de;
        }
    }
    if (tb->base[SLOT_FU_TOP]) {
        const double e = -flux_term_top(series_value(tb, rows, SLOT_FU_TOP, ii), v.g);
        if (ln.is_top) bc.flux_U = e;
        if constexpr (TANGENT) {
            const double de = -flux_term_top(series_seed(sn[SLOT_FU_TOP], series_bracket(tb, rows, SLOT_FU_TOP), ii), v.g);
            if (ln.is_top) dflux_U = de;
        }
    }
    if constexpr (WRITEBACK) {
        if (step == a.nsteps - 1 && ln.act && ln.is_top) {
            for (int s = SLOT_T_BOT; s <= SLOT_FU_TOP; ++s)
                if (tb->base[s]) tb->dst[s][ii] = series_value(tb, rows, s, ii);
        }
    }
}

// the temperature boundary values of one step for the backward sweep (the transposed step reads no flux value)
TRM_DEV void series_temperatures(const ColumnArgs<double>& a, int ii, int step, double& bTb, double& bTt) {
    const SeriesTable<double>* tb = a.series;
    const SeriesRow* rows = a.series_rows + (size_t)step * (size_t)a.nseries;
    if (tb->base[SLOT_T_BOT]) bTb = series_value(tb, rows, SLOT_T_BOT, ii);
    if (tb->base[SLOT_T_TOP]) bTt = series_value(tb, rows, SLOT_T_TOP, ii);
}

// the node sums of one seriesed pair in the registers of its owning edge lane (`own`; every other lane carries zeros and touches no memory)
struct SeriesNodeSums {
    long long n1 = -1, n2 = -1;   // the bracket held (wave-uniform); -1: none
    double h1 = 0.0, h2 = 0.0;
};
TRM_DEV void series_sums_store(const SeriesNodeSums& s, double* g, bool own, int ii) {
    if (own) {
        if (s.n1 >= 0) g[s.n1 + ii] = s.h1;
        if (s.n2 >= 0) g[s.n2 + ii] = s.h2;
    }
}
// one step's term: w1 term onto node n1, w2 term onto node n2
TRM_DEV void series_sums_add(SeriesNodeSums& s, double* g, const SeriesBracket& b, bool own, int ii, double term) {
    if (b.n1 != s.n1 || b.n2 != s.n2) {
        series_sums_store(s, g, own, ii);
        s.n1 = b.n1;
        s.n2 = b.n2;
        s.h1 = own ? g[b.n1 + ii] : 0.0;
        s.h2 = (own && b.n2 >= 0) ? g[b.n2 + ii] : 0.0;
    }
    s.h1 = s.h1 + b.w1 * term;
    if (b.n2 >= 0) s.h2 = s.h2 + b.w2 * term;
}

// the node accumulators of a SERIES sweep, [nt][Nh] per seriesed pair in the order of the slots (null: the pair has no series)
struct SeriesGradPtrs {
    double* gn[4];
};
// the four pairs' held sums
struct SeriesGrad {
    SeriesNodeSums s[4];
};

// ---- what every heat-only derivative kernel is built from (the tangent programs of trm_column_tangent.hpp, k_column_record and the
// sweeps of trm_column_adjoint.hpp and trm_column_adjoint_ckpt.hpp): each written once ------------------------------------------------------------
// the fifth argument of a program that carries no record (a record's parts stand under `if constexpr (RECORD)`)
struct NoRecord {};

// what a lane-per-level kernel knows about its lane; `ii`: the lane's column, `e`: its cell
template <int LPC> TRM_DEV LaneInfo derivative_lane(const View<double>& v, int& ii, size_t& e) {
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
    ii = colok ? i : Nh - 1;                             // (tail lanes carry clamped copies and store nothing)
    e = (size_t)ii * (size_t)v.Nzp + (size_t)(ln.k < Nz ? ln.k : Nz - 1);
    return ln;
}

// The temperature boundary values of the column, constants over a launch.  The primal programs (SWEEP = false: the tangent, the record)
// take those of a Value condition alone: under the generic halos column_tendencies_generic and tendency_tangent read the value arrays
// themselves.  The sweeps (SWEEP = true) take those of a Gradient condition as well where the halos are generic: adjoint_step forms
// k_step_wave's halos from what the kernel has loaded, so that the tape's is the only load inside the sweep.
template <bool SWEEP> TRM_DEV void temperature_boundary_values(const View<double>& v, int ii, bool generic, double& bTb, double& bTt) {
    const int kb = v.bc.kind[2][0], kt = v.bc.kind[2][1];
    const bool gradient = SWEEP && generic;
    bTb = (kb == 1 || (gradient && kb == 3)) ? bcval(v, 2, 0)[ii] : 0.0;
    bTt = (kt == 1 || (gradient && kt == 3)) ? bcval(v, 2, 1)[ii] : 0.0;
}

// the boundary inputs of a heat-only launch
TRM_DEV ColumnBC<double> heat_bc(const View<double>& v, const LaneInfo& ln, int ii, bool generic, double bTb, double bTt) {
    using NF = double;
    ColumnBC<NF> bc;
    bc.bTb = bTb;
    bc.bTt = bTt;
    bc.flux_S = 0.0;
    bc.has_U = true;
    bc.has_S = false;
    // compute_z_bcs! terms as each program forms them (k_step_wave: flux_term_*; the column program: flux_term_*_nsz, selects)
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
    return bc;
}

// One primal ForwardEuler step of the cell `c` under `bc`, by the column program's own building blocks (so its bits are trm_step's):
// the new cell into `n`, the step's tendency into `gU`, the fractions of the new state into `f`.  `have_f`: `f` holds the fractions of `c`
// (the step before left them there) and column_tendencies takes them from it.
// (Measured on the listings: with the fractions returned by value and a pointer argument, k_column_record without a stride came out with
// its first step peeled, 1 029 instructions instead of 668.)
template <int HYD, int LPC>
TRM_DEV void heat_step(const View<double>& v, const DevParams<double>& p, const LevelGeom<double>& L, const LaneInfo& ln, int ii, size_t e,
                       bool generic, const ColumnBC<double>& bc, double dt, const Cell<double>& c, bool have_f, Frac<double>& f, Cell<double>& n,
                       double& gU, uint32_t& viol, bool& bad) {
    using NF = double;
    const Frac<NF>* pre = have_f ? &f : nullptr;
    const Tendency<NF> t = generic ? column_tendencies_generic<NF, false, HYD, LPC>(v, p, L, ln, c, ii, (unsigned)(e * sizeof(NF)), false, viol)
                                   : column_tendencies<NF, false, HYD, LPC>(v, p, L, ln, c, bc.bTb, bc.bTt, false, viol, pre);
    NF g = t.gU, gS = t.gS, z0;
    column_advance<NF, false, LPC>(v, L, ln, v.Nz, bc, c.U, c.sat, g, gS, dt, n, z0, bad);
    f = column_closure<NF, false, HYD>(p, L, z0, n, viol);
    gU = g;
}

// the outputs of a finalizing trm_step: the new state, the tendency of the last step, hydraulic_conductivity of the new state
// (compute_auxiliary!) and the status flags
template <int HYD, int LPC>
TRM_DEV void finalize_heat_outputs(const View<double>& v, const DevParams<double>& p, const LaneInfo& ln, int ii, size_t e, const Cell<double>& n,
                                   const Frac<double>& f_new, double gU_out, uint32_t viol, bool bad) {
    using NF = double;
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
        viol |= bad ? 1u : 0u;
    }
    if (viol && ln.act) atomicOr(v.status, viol);
}

}  // namespace trm
