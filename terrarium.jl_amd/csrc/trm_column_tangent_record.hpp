// trm_column_tangent_record.hpp -- k_column_tangent with a tangent record attached (trm_tangent_record_attach; DESIGN 4.7 "Tangent
// records"): the same steps of the state and its tangent, and the temperature and its tangent stored at the record's levels behind every
// step whose position the record lists.  The forward twin of k_column_adjoint_record (trm_column_adjoint.hpp): a kernel of its own, so
// that the record-free instances of k_column_tangent stay what they are; every building block is shared with them.
#pragma once
#include "trm_column_tangent.hpp"

namespace trm {

// The fifth kernel argument.  Lane = level: `row_of_level[Nz]` (-1: not sampled) is read once per lane in front of the step loop;
// `row_of_position` points at the entry of the launch's first state in the table of the whole record ([last position + 1], -1: no sample)
// and is indexed with the step of the launch, a wave-uniform index, so "is this step sampled" is a scalar branch.  `T`, `dT`:
// [npos][nlevels][Nh], written by the lane that owns the cell.  One lane owns a cell and a position occurs once: nothing is atomic.
// `sample_entry`: the launch's first state is position 0 of the record's count (the first launch after an attach or a rewind) and is
// sampled too -- the T the entry closure forms at the stored U, and the entry dT.
struct TangentRecordArgs {
    const int32_t* row_of_level;
    const int32_t* row_of_position;
    double* T;
    double* dT;
    int nlevels;
    int sample_entry;
};
// the owning lane's stores of one sample; `row`: the position's row (wave-uniform, >= 0), `j`: the lane's row of the level list (-1: none)
TRM_DEV void tangent_record_store(const TangentRecordArgs& r, int row, int j, int ii, long long Nh, double T, double dT) {
    if (j >= 0) {
        const size_t q = ((size_t)row * (size_t)r.nlevels + (size_t)j) * (size_t)Nh + (size_t)ii;
        r.T[q] = T;
        r.dT[q] = dT;
    }
}

// k_column_tangent, and behind step s of the launch (position start + s + 1) the sample of that position: n.T and dT as the step's closure
// and its tangent have formed them, the PSEED term included.  What the launch leaves is what k_column_tangent leaves.
// Waves per SIMD: the record-free siblings run at 4 (108 ... 127 VGPRs) but for RIDE_PARAM_SERIES at 3 (140).  The sample's row and
// addresses cost two to nine registers; the floor of 4 keeps the instances without a series at 4 waves (RIDE_PARAM: 127 VGPRs instead of
// 129, no scratch).  With a series the floor of 4 spills (28 bytes of scratch): those two instances run at 3.
template <int HYD, int LPC, Ride R>
__global__ void __launch_bounds__(TRM_STEP_BLOCK) __attribute__((amdgpu_waves_per_eu(ride_has_series(R) ? 3 : 4)))
k_column_tangent_record(View<double> v, DevParams<double> p, ColumnArgs<double> a, TangentArgs<R> ta, TangentRecordArgs r) {
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
    const int j = ln.act ? r.row_of_level[ln.k] : -1;    // (-1 for lanes that own no cell: they store no sample)
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
        if (r.sample_entry) {
            const int row = r.row_of_position[0];
            if (row >= 0) tangent_record_store(r, row, j, ii, v.Nh, T0, dT);
        }
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
        // the sample of the position this step has reached (a scalar load and a scalar branch; the stores are the owning lanes')
        const int row = r.row_of_position[step + 1];
        if (row >= 0) tangent_record_store(r, row, j, ii, v.Nh, n.T, dT);
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

}  // namespace trm
