// trm_launch_observe.hip -- adjoint observations (trm_adjoint_observe, trm_adjoint_observe_misfit): the two kernels that let a
// loss read the run at taped positions and not at its end alone, and their launches.
//
// k_observe_misfit runs at registration: 1/2 w (T - T_obs)^2 of the stored temperature on the observed levels onto the per-column loss.
// k_observe_inject runs inside trm_adjoint_backward, when the sweep has pulled back every step >= p: the cotangent of the observation
// through the closure at U_p onto lam,
//   lU += wU + a_p wT + b_p wliq         (a_p, b_p: the closure slopes at U_p, the quantities adjoint_fold forms for the final state)
// and, with a parameter gradient open, wT through the heat capacity of that closure onto the per-cell parameter sums (the
// closure_param_slope / param_grad_add_C term of adjoint_fold<PGRAD>).  T, liq, the fractions and C come from energy_closure_wave,
// heat_capacity and closure_tangent: the functions the fold uses.  The misfit's wT is w (T - T_obs) with that T; a NaN in T_obs or a
// weight 0 gives wT = +0 and adds nothing to the loss.
// Layout: columns across lanes (the arrays of an observation are [nlevels][Nh], coalesced over Nh), blockIdx.y the level of the list
// for the injection; the levels of a list are distinct, so one lane owns a cell and nothing is atomic.  The misfit sums the levels of
// a column in list order in one lane.  The launches of one position run in registration order on the context stream: every sum is
// sequential in that order.
#include "trm_host.hpp"
#include "trm_column_adjoint.hpp"

namespace trm {

struct ObserveArgs {
    const double* U;         // U_p, [Nh][Nzp]: a tape slot, a checkpoint, or the context's U
    const int32_t* levels;   // [nlevels], strictly increasing, each in 0 ... Nz-1
    const double* a;         // [nlevels][Nh]: the cotangent (linear) or T_obs (misfit)
    const double* b;         // [nlevels][Nh]: the weights of a misfit, or null (1)
    double* lU;              // lam between the launches of the sweep
    int kind;                // TRM_ADJOINT_* or trm_ctx::OBSERVE_MISFIT
    int lam, params;         // which of the two shares this launch adds
};

// the cotangent of the misfit at one cell: w (T - T_obs), +0 for a gap in the record (NaN) or a weight 0
TRM_DEV double misfit_cotangent(double T, double obs, double w) { return (obs != obs || w == 0.0) ? 0.0 : w * (T - obs); }

template <bool PGRAD>
__global__ void __launch_bounds__(256) k_observe_inject(View<double> v, DevParams<double> p, ObserveArgs o, ParamGradPtrs pg) {
    const long i0 = (long)blockIdx.x * 256 + (long)threadIdx.x;
    const bool act = i0 < v.Nh;
    const long i = act ? i0 : v.Nh - 1;       // (tail lanes carry clamped copies and store nothing: the closure takes ballots)
    const int j = (int)blockIdx.y;
    const size_t e = (size_t)i * (size_t)v.Nzp + (size_t)o.levels[j];
    const size_t q = (size_t)j * (size_t)v.Nh + (size_t)i;
    const double U = o.U[e], sat = v.sat[e];
    uint32_t viol_in = 0;
    double liq, T, via_T, via_liq, unused_liq, unused_T;
    const Frac<double> f = energy_closure_wave<double, 0>(p, U, sat, liq, T, viol_in);
    const double C = heat_capacity(p, f);
    const double x = o.a[q];
    double wU = 0.0, wT = 0.0, wliq = 0.0;
    if (o.kind == trm_ctx::OBSERVE_MISFIT) wT = misfit_cotangent(T, x, o.b ? o.b[q] : 1.0);
    else if (o.kind == TRM_ADJOINT_INTERNAL_ENERGY) wU = x;
    else if (o.kind == TRM_ADJOINT_TEMPERATURE) wT = x;
    else wliq = x;
    closure_tangent(p, U, sat, C, wT, unused_liq, via_T);
    closure_tangent(p, U, sat, C, wliq, via_liq, unused_T);
    if (o.lam && act) o.lU[e] = o.lU[e] + (wU + via_T + via_liq);
    if constexpr (PGRAD) {
        if (o.params) {
            LaneInfo ln{};
            ln.act = act;
            ParamGrad acc = param_grad_load(pg, e, 0);
            param_grad_add_C(acc, f, closure_param_slope(T, C) * wT);
            param_grad_store(pg, ln, e, acc);
        }
    }
}

__global__ void __launch_bounds__(256) k_observe_misfit(const double* __restrict__ T, long Nh, int Nzp, const int32_t* __restrict__ levels, int nlevels,
                                                        const double* __restrict__ obs, const double* __restrict__ weight, double* __restrict__ loss) {
    const long i = (long)blockIdx.x * 256 + (long)threadIdx.x;
    if (i >= Nh) return;
    double s = loss[i];
    for (int j = 0; j < nlevels; ++j) {
        const size_t q = (size_t)j * (size_t)Nh + (size_t)i;
        const double x = obs[q], w = weight ? weight[q] : 1.0;
        if (x == x && w != 0.0) {
            const double r = T[(size_t)i * (size_t)Nzp + (size_t)levels[j]] - x;
            s = s + 0.5 * w * r * r;
        }
    }
    loss[i] = s;
}

}  // namespace trm

namespace trmh {

int ObserveLaunch::misfit(trm_ctx* c, const trm_ctx::Observation& o) {
    if (!c->d_misfit || !o.d_data || o.kind != trm_ctx::OBSERVE_MISFIT || o.nlevels < 1 || o.nlevels > c->Nz)
        return fail(c, TRM_EINVAL, "k_observe_misfit: no accumulator, or not a misfit observation");
    const View<double>& v = launch_args<double>(c).state;
    hipLaunchKernelGGL(k_observe_misfit, dim3((unsigned)((c->Nh + 255) / 256)), dim3(256), 0, c->stream, (const double*)v.T, (long)c->Nh, c->Nzp, o.levels(c->Nh),
                       o.nlevels, o.array(0, c->Nh), o.array(1, c->Nh), c->d_misfit);
    TRM_HIP(c, hipGetLastError());
    return TRM_OK;
}

int ObserveLaunch::inject(trm_ctx* c, const trm_ctx::Observation& o, const double* U_p, bool lam, bool params) {
    const bool pgrad = params && c->d_adj_param_out;
    if (!lam && !pgrad) return TRM_OK;
    if (!c->d_adj[TRM_ADJOINT_INTERNAL_ENERGY] || !o.d_data || o.nlevels < 1 || o.nlevels > c->Nz || o.kind < 0 || o.kind > trm_ctx::OBSERVE_MISFIT)
        return fail(c, TRM_EINVAL, "k_observe_inject: no adjoint is open, or a bad observation");
    const LaunchArgs<double>& la = launch_args<double>(c);
    ObserveArgs a;
    a.U = U_p ? U_p : la.state.U;
    a.levels = o.levels(c->Nh);
    a.a = o.array(0, c->Nh);
    a.b = o.kind == trm_ctx::OBSERVE_MISFIT ? o.array(1, c->Nh) : nullptr;
    a.lU = c->d_adj[TRM_ADJOINT_INTERNAL_ENERGY];
    a.kind = o.kind;
    a.lam = lam ? 1 : 0;
    a.params = pgrad ? 1 : 0;
    ParamGradPtrs pg{};
    const dim3 grid((unsigned)((c->Nh + 255) / 256), (unsigned)o.nlevels);
    if (pgrad) {
        for (int q = 0; q < 8; ++q) {
            if (!c->d_adj_param[q]) return fail(c, TRM_EINVAL, "k_observe_inject: no accumulators");
            pg.g[q] = c->d_adj_param[q];
        }
        hipLaunchKernelGGL((k_observe_inject<true>), grid, dim3(256), 0, c->stream, la.state, la.p, a, pg);
    } else hipLaunchKernelGGL((k_observe_inject<false>), grid, dim3(256), 0, c->stream, la.state, la.p, a, pg);
    TRM_HIP(c, hipGetLastError());
    return TRM_OK;
}

}  // namespace trmh
