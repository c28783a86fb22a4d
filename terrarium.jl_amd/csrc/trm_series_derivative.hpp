// trm_series_derivative.hpp -- boundary time series inside the derivative kernels (TRM_OPT_DERIVATIVE_SERIES; DESIGN 4.7 / 4.8 "Series").
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

}  // namespace trm
