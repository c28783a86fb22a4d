// trm_step_api.hip -- the step sequences of both precisions (Ops<NF>: which launches make one ForwardEuler or Heun step, in which order,
// and what they leave in the context's flags) and the entry points that run them: the reference-order calls, trm_step / trm_step_heun and
// their timed and two-call forms, the time averages, the vegetation set-up, and the n-context drivers of the two step calls.  Ops is named
// in this file alone.  The time averages sit here because the step sequences feed them; trm_step_all / trm_step_heun_all because they
// deal out launches by the steps one launch covers.  Host code alone: the kernels are launched by the trm_launch_*.hip files.
#include "trm_host.hpp"

using namespace trm;
using namespace trmh;

namespace {

// the fields trm_average_open takes: the soil state and its closures, surface excess water and water table, and the LandModel's
// surface diagnostics on a context with the surface energy balance -- never on a standalone VegetationModel
bool averageable(const trm_ctx* c, int field) {
    if (c->veg_mode == TRM_VEGETATION_STANDALONE || !c->state.f[field]) return false;
    const int s = accum_slot(field);
    if (s < 0) return false;
    return s < ACC_TS || c->params.seb != 0;
}

// Heun's path (Ops::heun_path).  One launch with both stages on the column in registers (Ops::fused_launch<PROG_HEUN>), by
// k_column / k_column_land / k_heun_generic (HEUN_ONE_LAUNCH) or the levels kernels (HEUN_LEVELS: 65 ... 256 levels; the stage's
// fields are allocated for them as for the reference-order kernels that ran there before them).  The stage's surface energy
// balance is not evaluated: its fluxes would only enter through compute_z_bcs!, which the reference runs for the state alone
// (heun.jl:54-69).  HEUN_COUPLED: the four launches of the vegetation-coupled LandModel, which store part of the stage.
// HEUN_REFERENCE: the reference-order kernels on a second copy of the state.
enum HeunPath { HEUN_ONE_LAUNCH, HEUN_LEVELS, HEUN_COUPLED, HEUN_REFERENCE };

// The step sequences of one precision.  The launches themselves are Unfused / Veg / ColumnLaunch / GenericLaunch / LevelsLaunch /
// LandLaunch / PackedLaunch (trm_host.hpp); the C ABI reaches the policies and the Unfused / Veg launches through Ops too.
template <class NF> struct Ops : StepPolicy<NF>, Unfused<NF>, Veg<NF> {
    using P = StepPolicy<NF>;
    using U = Unfused<NF>;
    using V = Veg<NF>;
    using P::tops_current; using P::averaging; using P::averages_in_launch; using P::program_applies; using P::single_step_program;

    // nsteps steps of the standalone VegetationModel; time series inputs are evaluated by the host between launches
    static int veg_step(trm_ctx* c, double dt, int nsteps, int finalize, bool heun) {
        c->last_program = TRM_PROGRAM_VEGETATION;
        int n = 0;
        while (n < nsteps) {
            const int m = c->series.empty() ? nsteps - n : 1;
            const int fin = (finalize && n + m == nsteps) ? 1 : 0;
            int rc = U::update_inputs(c, c->state, c->time);
            if (!rc) rc = V::vegetation(c, c->state, heun ? VEG_HEUN : VEG_EULER, dt, m, fin);
            if (rc) return rc;
            tick(c, dt, m);
            n += m;
        }
        return TRM_OK;
    }
    static int unfused_step(trm_ctx* c, double dt, int finalize) {
        c->last_program = TRM_PROGRAM_UNFUSED;
        int rc = U::update_state(c, c->state, true);
        if (!rc) rc = U::explicit_step(c, c->state, dt);
        if (!rc) rc = U::closure(c, c->state);
        if (!rc) rc = accumulate_after(c, dt);
        if (!rc && finalize) rc = U::compute_auxiliary(c, c->state);
        return rc;
    }
    // ---- time averages (trm_average_*, trm_average.hpp) ----------------------------------------------------------------------
    // One step's terms of every open accumulator from the fields as the step launch left them: one k_accumulate launch (per 32
    // accumulators), the windows advanced by dt.  Nothing while none is open.
    static int accumulate_after(trm_ctx* c, double dt) {
        if (!averaging(c)) return TRM_OK;
        AccumBatch b{};
        b.w = dt;
        for (auto& a : c->averages) {
            if (a.field < 0) continue;
            AccumEntry& e = b.e[b.count++];
            e.src = c->state.f[a.field];
            e.sum = a.d_sum;
            e.n = (long long)field_elems(c, a.field);
            e.pitch = is_3d(a.field) ? c->Nzp : 1;
            e.nz = is_3d(a.field) ? c->Nz : 1;
            e.src_double = 0;
            a.window += dt;
            a.steps += 1;
            if (b.count == ACC_BATCH) {
                if (int rc = AverageLaunch<NF>::accumulate(c, b)) return rc;
                b.count = 0;
            }
        }
        if (int rc = AverageLaunch<NF>::accumulate(c, b)) return rc;
        c->last_program |= TRM_PROGRAM_AVERAGES_AFTER_LAUNCH;
        return TRM_OK;
    }
    // k_column_accum: `nsteps` steps, partials added to the accumulators (one open accumulator of a field: straight into it; more:
    // into a zeroed scratch buffer, then one k_accumulate adds the scratch to each)
    static int multi_program_accum(trm_ctx* c, double dt, int finalize, int nsteps) {
        AccumArgs aa{};
        aa.dt = dt;
        aa.mask = 0;
        int handles[ACC_SLOTS] = {};
        for (const auto& a : c->averages) if (a.field >= 0) handles[accum_slot(a.field)] += 1;
        AccumBatch b{};
        b.w = 1.0;
        for (int sl = 0; sl < ACC_SLOTS; ++sl) {
            if (!handles[sl]) continue;
            aa.mask |= 1u << sl;
            const int f = accum_field(sl);
            if (handles[sl] == 1) {
                for (const auto& a : c->averages) if (a.field == f) aa.dst[sl] = a.d_sum;
                continue;
            }
            const size_t bytes = field_elems(c, f) * sizeof(double);
            if (!c->d_acc_partial[sl]) TRM_HIP(c, hipMalloc(&c->d_acc_partial[sl], bytes));
            TRM_HIP(c, hipMemsetAsync(c->d_acc_partial[sl], 0, bytes, c->stream));
            aa.dst[sl] = c->d_acc_partial[sl];
            for (const auto& a : c->averages) {
                if (a.field != f) continue;
                if (b.count == ACC_BATCH) return fail(c, TRM_EUNSUPPORTED, "more than 32 accumulators of fields that share a field");
                AccumEntry& e = b.e[b.count++];
                e.src = c->d_acc_partial[sl];
                e.sum = a.d_sum;
                e.n = (long long)field_elems(c, f);
                e.pitch = is_3d(f) ? c->Nzp : 1;
                e.nz = is_3d(f) ? c->Nz : 1;
                e.src_double = 1;
            }
        }
        int rc = TRM_OK;
        by_bool(P::richards(c), [&](auto RICH) { rc = ColumnAccumLaunch<NF, RICH()>::run(c, dt, finalize, nsteps, aa); });
        if (!rc) rc = AverageLaunch<NF>::accumulate(c, b);
        if (rc) return rc;
        for (auto& a : c->averages) {
            if (a.field < 0) continue;
            for (int j = 0; j < nsteps; ++j) a.window += dt;
            a.steps += nsteps;
        }
        return TRM_OK;
    }
    // ---- the fused step of the state: one sequence for every program -------------------------------------------------------
    // update_inputs! of the state; Heun: of the stage as well, at its clock t + dt (heun.jl:52); the multi-step program with time
    // series: the rows it interpolates itself instead
    template <int PROG> static int fused_prologue(trm_ctx* c, double dt, int nsteps) {
        if (PROG == PROG_MULTI && !c->series.empty()) return U::upload_series_rows(c, dt, nsteps);
        int rc = U::update_inputs(c, c->state, c->time);
        if (!rc && PROG == PROG_HEUN) rc = U::update_inputs(c, c->stage, c->time + dt);
        return rc;
    }
    // The launch of a fused step, by program.  ForwardEuler: the surface processes in the launch
    // (k_column_land / k_step_pk_land), 65 ... 256 levels (k_column_deep / k_column_wide), the packed fp32 step (k_step_pk), the generic
    // boundary kinds (k_step_wave) or k_column.  Heun: in the launch, levels, generic (k_heun_generic) or k_column.  The multi-step
    // program: the time averages accumulated in the launch (k_column_accum), levels or k_column.
    template <int PROG> static int step_launch(trm_ctx* c, const StepPlan& plan, double dt, int fin, int nsteps) {      // (plan: StepPolicy::plan_step)
        if (plan.route == ROUTE_SURFACE_IN_LAUNCH) return std::is_same<NF, float>::value ? PackedLaunch::step_land(c, dt, fin) : FrontLaunch::run(c, plan, dt, fin, PROG == PROG_HEUN);
        if (plan.route == ROUTE_ACCUM_IN_LAUNCH) return multi_program_accum(c, dt, fin, nsteps);
        if (plan.route == ROUTE_LEVELS) return levels_launch<NF>(c, PROG, P::generic_bcs(c), dt, fin, nsteps);
        if (plan.route == ROUTE_PACKED) return PackedLaunch::step(c, dt, fin);
        if (plan.route == ROUTE_GENERIC) return PROG == PROG_HEUN ? GenericLaunch<NF>::heun(c, dt, fin) : GenericLaunch<NF>::step(c, dt, fin);
        int rc = TRM_OK;
        by_bool(P::richards(c), [&](auto RICH) { rc = ColumnLaunch<NF, RICH(), PROG>::run(c, plan, dt, fin, nsteps); });
        return rc;
    }
    // What a fused launch leaves (rc: the launch's): the stored T / liq are the closure of the state once it has succeeded; the open
    // time averages take the step's terms (`accumulate`: the launch has not added them itself); only the finalizing launch stores
    // state.tendencies; the top-cell arrays describe the state after a successful LandModel launch.  Then, finalizing, the state's
    // surface processes once more (+ the 0-D auxiliaries of the coupled vegetation).
    static int fused_epilogue(trm_ctx* c, int rc, double dt, int fin, bool accumulate = true, bool deferred = false, bool psi_step = false) {
        if (!rc) c->closure_consistent = true;
        c->psi_consistent = !rc && psi_step;          // (pressure_head / water_table as a k_column ForwardEuler launch leaves them)
        if (!rc) c->closure_deferred = deferred;      // (every other launch has stored T / liq)
        if (!rc && accumulate) rc = accumulate_after(c, dt);
        c->tend_valid = fin != 0;
        c->top_valid = c->params.seb != 0 && !rc && tops_current(c);
        if (rc || !fin) return rc;
        if (P::coupled(c)) return V::surface_veg(c, c->state, true, false, 0.0);
        return c->params.seb ? U::surface(c, c->state, true) : TRM_OK;
    }
    // One fused launch of the columns the launch helpers currently address: one ForwardEuler or Heun step, or `nsteps` steps of the
    // multi-step program (PROG_MULTI; it carries the surface processes and the series itself).  The 0-D surface processes run as
    // their own small launch in front of the column kernel (LandModel; + the 0-D prognostics' step of the coupled vegetation) unless
    // the launch carries them (surface_in_launch).  (The per-cell plant_available_water field is materialised with the other per-cell
    // auxiliaries: by the finalizing launch, or every step under TRM_OPT_WRITE_KF_EVERY_STEP.)
    // `not_last`, `*interior`: Ops::step's two facts (StepPolicy::plan_step); `*interior` arrives as "the launch before was interior" and leaves as "this one was"
    template <int PROG> static int fused_launch(trm_ctx* c, double dt, int fin, int nsteps = 1, bool not_last = false, bool* interior = nullptr) {
        int rc = fused_prologue<PROG>(c, dt, nsteps);
        const StepPlan plan = P::plan_step(c, PROG, not_last, interior && *interior);
        const bool in_launch = plan.route == ROUTE_SURFACE_IN_LAUNCH, accum = plan.route == ROUTE_ACCUM_IN_LAUNCH;
        // T / liq left unstored by earlier launches: materialised in front of everything that reads them from the 3-D arrays -- any
        // step launch but a deriving one, the vegetation launches (never deriving), a surface launch that gathers the top cell from
        // the fields
        const bool surface_reads_fields = c->params.seb && !in_launch && !(c->top_valid && c->d_top3);
        if (!rc && c->closure_deferred && (surface_reads_fields || !plan.derives_unread)) rc = flush_closure(c);
        if (PROG != PROG_EULER && plan.check_entry && !rc) rc = fail(c, TRM_EINVAL, "trm_step: an interior launch must be followed by a ForwardEuler launch");
        if (!rc && plan.refusal) rc = fail(c, TRM_EINVAL, plan.refusal);
        if (!rc && PROG != PROG_MULTI && P::coupled(c)) rc = V::surface_veg(c, c->state, true, true, dt, c->opt_write_kf != 0);
        else if (!rc && PROG != PROG_MULTI && c->params.seb && !in_launch) rc = U::surface(c, c->state, true);
        if (!rc) rc = step_launch<PROG>(c, plan, dt, fin, nsteps);
        if (!rc && plan.psi_form == PSI_INTERIOR) c->interior_launches += 1;
        if (!rc && interior) *interior = plan.psi_form == PSI_INTERIOR;
        return fused_epilogue(c, rc, dt, fin, !accum, !plan.store_closure, plan.psi_step);
    }
    // ---- LandModel, per-step path: the surface processes of one half of the columns UNDER the column program of the other ----
    // (k_land_euler / k_land_pk, trm_column.hpp: one stream, two launches per step as before, each covering the soil columns
    // of one half and the 0-D surface processes of the other)
    static bool interleave_now(trm_ctx* c, int steps_left) {
        if (c->opt_pipeline == 0 || steps_left < 2 || averaging(c) || !c->params.seb || !P::richards(c) || P::coupled(c) || c->part_n[1] <= 0) return false;
        if (!c->series.empty() || P::generic_bcs(c) || c->Nz > 64) return false;      // (inputs constant over the call; one level per lane)
        if (std::is_same<NF, float>::value && !P::packed_path(c)) return false;        // (fp32 off the packed kernel: not instantiated)
        // Measured (profiles/r03/exp6_ab_land_interleaved.log, bench_default.json: land_interleaved): within +-2 % at 812 500 columns
        // (492 vs 497, 503 vs 511 us on one box; 523 vs 512 on another), +10 % at N145 and on its shards -- every launch carries ~4 us
        // of fixed cost, and two half-size column launches pay it twice where the k_surface launch they absorb was little more than
        // that fixed cost itself.  Not a win anywhere it was measured: AUTO (2) leaves it off; 1 forces it.
        return c->opt_pipeline == 1;
    }
    // `nsteps` >= 2 ForwardEuler steps of a bare-ground LandModel with constant inputs; columns of part `qcol` step, the surface
    // processes of part `qsurf` run beside them for ITS next column step:
    //     surf(A, 0) | col(A, 0) + surf(B, 0) | col(B, 0) + surf(A, 1) | ... | col(A, N-1) + surf(B, N-1) | col(B, N-1)
    static int land_steps_interleaved(trm_ctx* c, double dt, int nsteps, int finalize) {
        const bool top0 = c->top_valid, cc0 = c->closure_consistent;
        int rc = flush_closure(c);      // (part launches never defer)
        if (rc) return rc;
        {   // the state's surface processes for half A
            PartScope scope(c, 0);
            c->top_valid = top0;
            rc = U::surface(c, c->state, true);
        }
        for (int n = 0; n < nsteps && !rc; ++n) {
            const int fin = (finalize && n == nsteps - 1) ? 1 : 0;
            const bool tops = (n == 0) ? top0 : tops_current(c);     // what a surface evaluation of an UNSTEPPED / stepped half reads
            c->closure_consistent = (n == 0) ? cc0 : true;
            rc = LandLaunch<NF>::run(c, 0, 1, dt, fin, tops);
            if (rc) break;
            if (n < nsteps - 1) {
                rc = LandLaunch<NF>::run(c, 1, 0, dt, 0, tops_current(c));   // (half A has just been stepped: its top arrays are current)
            } else {
                PartScope scope(c, 1);
                rc = step_launch<PROG_EULER>(c, P::plan_step(c, PROG_EULER, false, false), dt, fin, 1);
            }
            tick(c, dt, 1);
        }
        return fused_epilogue(c, rc, dt, finalize);
    }
    static int steps_per_launch_now(trm_ctx* c) {
        return !program_applies(c) ? 1 : (c->opt_steps_per_launch > 0 ? c->opt_steps_per_launch : P::auto_steps_per_launch(c));
    }
    static int step(trm_ctx* c, double dt, int nsteps, int finalize) {
        if (c->veg_mode == TRM_VEGETATION_STANDALONE) return veg_step(c, dt, nsteps, finalize, false);
        if (c->opt_kernel != TRM_KERNEL_FUSED || P::levels_per_lane(c) == 0)      // (the reference-order kernels read T / liq as stored)
            if (int rf = flush_closure(c)) return rf;
        // the fused kernels map one soil level to one lane (two for 65 ... 128 levels, four for 129 ... 256); anything deeper takes the
        // reference-order kernels.
        const bool fused = c->opt_kernel == TRM_KERNEL_FUSED && P::levels_per_lane(c) > 0;
        // Resident-column multi-step program: legal when nothing the host evaluates changes between the steps of a launch --
        // constants, or device-resident time series the program interpolates itself -- and the branch-free boundary kinds apply.
        // (columns of 65 ... 128 levels: contexts without the surface energy balance and without series)
        const bool program_ok = program_applies(c);
        // open time averages that the multi-step program cannot accumulate itself: one launch per step, k_accumulate behind each
        const bool avg = averaging(c), avg_in_launch = avg && program_ok && averages_in_launch(c);
        const int spl = (avg && !avg_in_launch) ? 1 : steps_per_launch_now(c);
        int n = 0, rc = TRM_OK;
        bool behind_interior = false;      // (the launch before was interior: psi, K, the water-table-derived fields in memory are stale until the call's last launch)
        while (n < nsteps && !rc) {
            int m = std::min(spl, nsteps - n);
            const int fin = (finalize && n + m == nsteps) ? 1 : 0;
            if (!fused) {
                rc = U::update_inputs(c, c->state, c->time);
                c->top_valid = false;
                c->tend_valid = true;
                if (!rc) rc = unfused_step(c, dt, fin);
                if (!rc) c->closure_consistent = true;   // closure! has just run
                c->psi_consistent = false;
            } else if (m > 1 || (program_ok && single_step_program(c))) {
                rc = fused_launch<PROG_MULTI>(c, dt, fin, m, false, &behind_interior);
            } else if (interleave_now(c, nsteps - n)) {
                // every remaining step of the call in one go (the clock is ticked inside)
                m = nsteps - n;
                rc = land_steps_interleaved(c, dt, m, finalize);
                n += m;
                continue;
            } else {
                // (interior launches: inside this call only, never its last launch, never finalizing)
                rc = fused_launch<PROG_EULER>(c, dt, fin, 1, n + m < nsteps && !fin, &behind_interior);
            }
            if (rc) break;
            tick(c, dt, m);
            n += m;
        }
        if (behind_interior) {
            // A launch failed behind interior launches (the loop cannot end otherwise: the call's last launch is never interior): pressure_head,
            // water-table and hydraulic_conductivity arrays are those of an earlier step.  Rebuilt here from the stored state with the
            // reference-order kernels, whatever they return -- the caller gets the error of the launch that failed.
            c->psi_consistent = false;
            const std::string err = c->err;
            if (!flush_closure(c) && !U::closure_hydrology(c, c->state, true, false)) (void)U::hydraulics(c, c->state);
            c->err = err;
            if (!rc) rc = fail(c, TRM_EINVAL, "trm_step: the call ended on an interior launch");
        }
        return rc;
    }

    // ---- Heun (heun.jl:37-71), reference-order kernels on a second copy of the state -----------------
    // copyto!(stage, state) (heun.jl:45) for what the stage's predictor step reads before its own closure! and update_state!
    // overwrite it: every per-column field, and of the per-cell fields the prognostics and their tendencies.  temperature,
    // liquid fraction, pressure head, hydraulic conductivity and plant available water of the stage are outputs of
    // closure!(stage) / compute_auxiliary!(stage) and are never read before that (k_explicit_step reads U, sat, S, Ts, the
    // tendencies and the boundary fluxes only): 4 of 9 per-cell copies instead of all of them.
    // `everything`: the per-cell closure and auxiliary fields too -- the two-call Heun, where the caller's functions may READ the
    // stage's fields before update_state!(stage) has recomputed them and must find what the reference's copyto! left there.
    static int copy_state_to_stage(trm_ctx* c, bool everything = false) {
        for (int f = 0; f < TRM_FIELD_COUNT; ++f) {
            if (!c->state.f[f] || !c->stage.f[f]) continue;
            if (f == TRM_FIELD_VWC_FORCING && c->stage_vwc_own) continue;      // (the caller's stage buffer: refresh_user_stage_buffers)
            const bool needed = everything || !is_3d(f) || f == TRM_FIELD_INTERNAL_ENERGY || f == TRM_FIELD_SATURATION_WATER_ICE ||
                                f == TRM_FIELD_TEND_INTERNAL_ENERGY || f == TRM_FIELD_TEND_SATURATION_WATER_ICE;
            if (needed) TRM_HIP(c, hipMemcpyAsync(c->stage.f[f], c->state.f[f], field_elems(c, f) * sizeof(NF), hipMemcpyDeviceToDevice, c->stream));
        }
        if (everything && c->state.kf_top && c->stage.kf_top)
            TRM_HIP(c, hipMemcpyAsync(c->stage.kf_top, c->state.kf_top, (size_t)c->Nh * sizeof(NF), hipMemcpyDeviceToDevice, c->stream));
        return TRM_OK;
    }
    // Heun of the vegetation-coupled LandModel in four launches (heun.jl:37-71 with land_model.jl:79-97).  The soil column's
    // two stages stay in registers (k_column<PROG_HEUN>); what the 0-D processes need AT the stage -- the stage's saturation,
    // liquid fraction, temperature, surface excess water -- is the only part of it that is stored.  The final soil state does not
    // depend on the stage's 0-D evaluation (its boundary fluxes are the state's, heun.jl:64-69), so the order is:
    //   1. k_surface_veg(state): auxiliaries, first-stage 0-D tendencies, PREDICTED 0-D prognostics -> stage arrays
    //   2. k_column<PROG_HEUN>: the soil step; stage soil fields -> stage arrays
    //   3. k_surface_veg(stage): auxiliaries and 0-D tendencies at the stage (inputs evaluated at t + dt)
    //   4. k_heun_average_0d: averaged tendencies, explicit step of canopy water, vegetation carbon, area fraction
    static int heun_step_coupled_fused(trm_ctx* c, double dt, int finalize) {
        int rc = fused_prologue<PROG_HEUN>(c, dt, 1);
        if (!rc) rc = flush_closure(c);
        if (rc) return fused_epilogue(c, rc, dt, finalize);
        const VegView<NF> vs = P::veg_view(c, c->state);
        VegView<NF> vg = P::veg_view(c, c->stage);
        View<NF> sv = cached_view<NF>(c, c->stage);
        // inputs of the stage: its own arrays where a time series feeds them (evaluated at t + dt above), else the state's
        auto fed = [&](int field) {
            for (const auto& sr : c->series) if (!sr.is_bc && sr.field == field) return true;
            return false;
        };
        const View<NF>& v0 = cached_view<NF>(c, c->state);
        if (!fed(TRM_FIELD_AIR_TEMPERATURE)) sv.Tair = v0.Tair;
        if (!fed(TRM_FIELD_AIR_PRESSURE)) sv.pres = v0.pres;
        if (!fed(TRM_FIELD_WINDSPEED)) sv.wind = v0.wind;
        if (!fed(TRM_FIELD_SPECIFIC_HUMIDITY)) sv.qair = v0.qair;
        if (!fed(TRM_FIELD_RAINFALL)) sv.rain = v0.rain;
        if (!fed(TRM_FIELD_SURFACE_SHORTWAVE_DOWN)) sv.swd = v0.swd;
        if (!fed(TRM_FIELD_SURFACE_LONGWAVE_DOWN)) sv.lwd = v0.lwd;
        if (!fed(TRM_FIELD_ALBEDO)) sv.albedo = v0.albedo;
        if (!fed(TRM_FIELD_EMISSIVITY)) sv.emissivity = v0.emissivity;
        vg.Tair = sv.Tair; vg.pres = sv.pres; vg.qair = sv.qair; vg.swd = sv.swd;
        if (!fed(TRM_FIELD_CO2)) vg.CO2 = vs.CO2;
        if (!fed(TRM_FIELD_DAILY_LEAF_RESPIRATION)) vg.daily_Rd = vs.daily_Rd;
        if (!fed(TRM_FIELD_STEM_AREA_INDEX)) vg.SAI = vs.SAI;
        SurfaceVegArgs<NF> a{};
        a.dt = (NF)dt;
        a.richards = P::richards(c) ? 1 : 0;
        a.from_state = 1;
        a.top_arrays = (c->top_valid && tops_current(c)) ? 1 : 0;
        a.advance = 3;
        a.store_paw = c->opt_write_kf != 0;
        a.st_w_can = vg.w_can; a.st_C_veg = vg.C_veg; a.st_nu = vg.nu; a.st_An = vg.An; a.st_Ts = sv.Ts;
        rc = V::surface_veg_launch(c, v0, vs, a);
        if (!rc) rc = step_launch<PROG_HEUN>(c, P::plan_step(c, PROG_HEUN, false, false), dt, finalize, 1);
        if (!rc) {
            SurfaceVegArgs<NF> b{};
            b.dt = (NF)dt;
            b.richards = a.richards;
            b.from_state = 1;
            b.top_arrays = 0;
            b.advance = 2;
            b.store_paw = 0;
            rc = V::surface_veg_launch(c, sv, vg, b);
        }
        if (!rc) rc = V::heun_average_0d(c, vs, vg, dt);
        return fused_epilogue(c, rc, dt, finalize);
    }
    // Stage buffers the caller of the two-call Heun has been handed (trm_stage_bc_device_ptr, the stage's vwc_forcing) hold
    // what it wrote for ITS last stage.  Whenever the library forms a stage on its own they are the state's values again: the
    // stage's predictor runs at the state's clock (heun.jl:47-50).
    static int refresh_user_stage_buffers(trm_ctx* c) {
        for (int a = 0; a < TRM_BCV_COUNT; ++a)
            for (int b = 0; b < 2; ++b)
                if (c->stage_bc_user[a][b] && c->bc_value_stage[a][b] && c->bc_value[a][b])
                    TRM_HIP(c, hipMemcpyAsync(c->bc_value_stage[a][b], c->bc_value[a][b], (size_t)c->Nh * sizeof(NF), hipMemcpyDeviceToDevice, c->stream));
        if (c->stage_vwc_own && c->stage.f[TRM_FIELD_VWC_FORCING])
            TRM_HIP(c, hipMemcpyAsync(c->stage.f[TRM_FIELD_VWC_FORCING], c->state.f[TRM_FIELD_VWC_FORCING], field_elems(c, TRM_FIELD_VWC_FORCING) * sizeof(NF), hipMemcpyDeviceToDevice, c->stream));
        return TRM_OK;
    }
    // heun.jl:41-52: the first half of timestep!(integrator, ::Heun) on the reference-order kernels
    static int heun_predict(trm_ctx* c, double dt, bool copy_everything = false) {
        int rc = U::update_inputs(c, c->state, c->time);
        if (!rc) rc = U::update_state(c, c->state, true);
        if (!rc) rc = copy_state_to_stage(c, copy_everything);
        if (!rc) rc = refresh_user_stage_buffers(c);
        if (!rc) rc = U::update_inputs(c, c->stage, c->time);   // the stage's clock is still t for its predictor step (heun.jl:47-50)
        if (!rc) rc = U::explicit_step(c, c->stage, dt);
        if (!rc) rc = U::closure(c, c->stage);
        if (!rc) rc = U::update_inputs(c, c->stage, c->time + dt);   // the stage's clock has ticked (heun.jl:52)
        return rc;
    }
    // heun.jl:54-71: the second half
    // update_state!(stage) up to and including compute_auxiliary!(stage) (heun.jl:54, state_variables.jl:72-80): what a forcing
    // function evaluated inside compute_tendencies!(stage) finds in `fields`
    static int heun_stage_auxiliary(trm_ctx* c) {
        int rc = U::reset_tendencies(c, c->stage);
        if (!rc) rc = U::compute_auxiliary(c, c->stage);
        return rc;
    }
    static int heun_correct(trm_ctx* c, double dt, int finalize, bool stage_auxiliary_done = false) {
        int rc = stage_auxiliary_done ? U::compute_tendencies(c, c->stage) : U::update_state(c, c->stage, true);
        if (!rc) rc = U::average(c, TRM_FIELD_TEND_INTERNAL_ENERGY);
        if (!rc && P::richards(c)) rc = U::average(c, TRM_FIELD_TEND_SATURATION_WATER_ICE);
        if (!rc && P::richards(c)) rc = U::average(c, TRM_FIELD_TEND_SURFACE_EXCESS_WATER);
        if (P::coupled(c))
            for (int f : {TRM_FIELD_TEND_CANOPY_WATER, TRM_FIELD_TEND_CARBON_VEGETATION, TRM_FIELD_TEND_VEGETATION_AREA_FRACTION})
                if (!rc) rc = U::average(c, f);
        if (!rc) rc = U::explicit_step(c, c->state, dt);
        if (!rc) rc = U::closure(c, c->state);
        if (!rc) rc = accumulate_after(c, dt);
        if (!rc && finalize) rc = U::compute_auxiliary(c, c->state);
        return rc;
    }
    // the path of one Heun step (HeunPath); trm_step_heun allocates the stage's fields for every path but HEUN_ONE_LAUNCH
    static int heun_path(const trm_ctx* c) {
        if (c->opt_kernel != TRM_KERNEL_FUSED || P::levels_per_lane(c) == 0) return HEUN_REFERENCE;
        if (P::coupled(c)) return P::generic_bcs(c) ? HEUN_REFERENCE : HEUN_COUPLED;
        return P::levels_per_lane(c) > 1 ? HEUN_LEVELS : HEUN_ONE_LAUNCH;
    }
    static int heun_step(trm_ctx* c, double dt, int finalize) {
        if (int rr = refresh_user_stage_buffers(c)) return rr;
        const int path = heun_path(c);
        if (path == HEUN_ONE_LAUNCH || path == HEUN_LEVELS) return fused_launch<PROG_HEUN>(c, dt, finalize);
        if (path == HEUN_COUPLED) return heun_step_coupled_fused(c, dt, finalize);
        c->top_valid = false;
        c->tend_valid = true;
        c->closure_consistent = true;   // (ends with closure!)
        c->psi_consistent = false;
        c->last_program = TRM_PROGRAM_UNFUSED;
        int rc = heun_predict(c, dt);
        if (!rc) rc = heun_correct(c, dt, finalize);
        return rc;
    }
};

// the step sequences of the context's precision: f(Ops<double>{}) or f(Ops<float>{}), whose static members they are; returns what f returns
template <class F> auto with_ops(const trm_ctx* c, F&& f) {
    return by_precision(c->precision, [&](auto nf) { return f(Ops<typename decltype(nf)::type>{}); });
}

// ---- vegetation set-up (trm_set_vegetation; a template cannot stand beside it inside extern "C") ------------------------------------
// static root fractions: density at the cell centres x thickness, normalised over the column (root_distribution.jl:45-63)
template <class NF> int upload_root_fraction(trm_ctx* c) {
    const VegDev<NF> p = StepPolicy<NF>::veg_dev(c);
    std::vector<NF> R((size_t)c->Nz);
    NF total = NF(0);
    for (int k = 0; k < c->Nz; ++k) {
        const NF z = (NF)c->h_zC[k], dz = (NF)c->h_dzc[k];
        R[k] = (NF(0.5) * (p.root_a * std::exp(p.root_a * z) + p.root_b * std::exp(p.root_b * z))) * dz;
    }
    for (int k = 0; k < c->Nz; ++k) total = total + R[k];
    std::vector<NF> per_level((size_t)c->Nz);
    for (int k = 0; k < c->Nz; ++k) per_level[k] = R[k] / total;
    if (!c->d_rootf) TRM_HIP(c, hipMalloc(&c->d_rootf, (size_t)c->Nz * sizeof(NF)));
    TRM_HIP(c, hipMemcpyAsync(c->d_rootf, per_level.data(), (size_t)c->Nz * sizeof(NF), hipMemcpyHostToDevice, c->stream));
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    std::vector<NF> host((size_t)c->Nz * c->Nh);
    for (int k = 0; k < c->Nz; ++k)
        for (long i = 0; i < c->Nh; ++i) host[(size_t)k * c->Nh + i] = R[k] / total;
    return upload_field(c, TRM_FIELD_ROOT_FRACTION, host.data());
}

}  // namespace

extern "C" {

int trm_initialize(trm_ctx* c) {
    TRM_ENTER(c);
    c->top_valid = false;
    c->closure_consistent = false;   // temperature is the user's, internal_energy follows from it
    state_changed(c);
    return finish(c, with_ops(c, [&](auto ops) { return ops.initialize(c); }));
}
int trm_update_inputs(trm_ctx* c) {
    TRM_ENTER(c);
    return finish(c, with_ops(c, [&](auto ops) { return ops.update_inputs(c, c->state, c->time); }));
}
int trm_update_state(trm_ctx* c, int compute_tendencies) {
    TRM_ENTER(c);
    c->tend_valid = true;
    c->psi_consistent = false;      // (the auxiliary fields are the reference-order kernels' from here on: the next step launch reads them as stored)
    if (c->veg_mode == TRM_VEGETATION_STANDALONE) {
        int rc = with_ops(c, [&](auto ops) { return ops.update_inputs(c, c->state, c->time); });
        if (!rc) rc = compute_tendencies ? with_ops(c, [&](auto ops) { return ops.vegetation(c, c->state, VEG_UPDATE, 0.0, 1, 0); }) : with_ops(c, [&](auto ops) { return ops.vegetation(c, c->state, VEG_AUX, 0.0, 1, 0); });
        return finish(c, rc);
    }
    int rc = with_ops(c, [&](auto ops) { return ops.update_inputs(c, c->state, c->time); });
    if (rc) return rc;
    return finish(c, with_ops(c, [&](auto ops) { return ops.update_state(c, c->state, compute_tendencies != 0); }));
}
int trm_compute_auxiliary(trm_ctx* c) {
    TRM_ENTER(c);
    c->psi_consistent = false;      // (likewise)
    if (c->veg_mode == TRM_VEGETATION_STANDALONE) return finish(c, with_ops(c, [&](auto ops) { return ops.vegetation(c, c->state, VEG_AUX, 0.0, 1, 0); }));
    return finish(c, with_ops(c, [&](auto ops) { return ops.compute_auxiliary(c, c->state); }));
}
int trm_compute_tendencies(trm_ctx* c) {
    TRM_ENTER(c);
    if (c->veg_mode == TRM_VEGETATION_STANDALONE) return finish(c, with_ops(c, [&](auto ops) { return ops.vegetation(c, c->state, VEG_TEND, 0.0, 1, 0); }));
    return finish(c, with_ops(c, [&](auto ops) { return ops.compute_tendencies(c, c->state); }));
}
int trm_reset_tendencies(trm_ctx* c) {
    TRM_ENTER(c);
    c->tend_valid = true;
    return finish(c, with_ops(c, [&](auto ops) { return ops.reset_tendencies(c, c->state); }));
}
int trm_explicit_step(trm_ctx* c, double dt) {
    TRM_ENTER(c);
    if (c->veg_mode == TRM_VEGETATION_STANDALONE) return finish(c, with_ops(c, [&](auto ops) { return ops.vegetation(c, c->state, VEG_EXPLICIT, dt, 1, 0); }));
    c->top_valid = false;
    c->closure_consistent = false;
    state_changed(c);
    return finish(c, with_ops(c, [&](auto ops) { return ops.explicit_step(c, c->state, dt); }));
}
int trm_closure(trm_ctx* c) {
    TRM_ENTER(c);
    c->top_valid = false;
    c->closure_consistent = true;
    c->psi_consistent = false;
    return finish(c, with_ops(c, [&](auto ops) { return ops.closure(c, c->state); }));
}
int trm_invclosure(trm_ctx* c) {
    TRM_ENTER(c);
    c->top_valid = false;
    c->closure_consistent = false;
    state_changed(c);
    return finish(c, with_ops(c, [&](auto ops) { return ops.invclosure(c, c->state); }));
}

int trm_step(trm_ctx* c, double dt, int nsteps, int finalize) {
    TRM_ENTER_KEEP(c);
    c->heun_pending = false;
    if (nsteps < 0) return fail(c, TRM_EINVAL, "trm_step: nsteps < 0");
    state_changed(c);
    return finish(c, with_ops(c, [&](auto ops) { return ops.step(c, dt, nsteps, finalize); }));
}

namespace {
// The timed entry points return as soon as the stop event has completed: the host POLLS it (a blocking wait is woken by an
// interrupt some 10-20 us later, which a caller's wall clock around a short run of steps would see).
int wait_polling(trm_ctx* c, hipEvent_t ev) {
    for (;;) {
        const hipError_t e = hipEventQuery(ev);
        if (e == hipSuccess) {
            (void)hipGetLastError();   // (hipErrorNotReady of the polls is not an error: do not leave it for the next launch check)
            return TRM_OK;
        }
        if (e != hipErrorNotReady) TRM_HIP(c, e);
    }
}
// the end of both timed entry points: the stop event behind the steps, the wait for it, the time since ev0
int timed_tail(trm_ctx* c, float* ms) {
    TRM_HIP(c, hipEventRecord(c->ev1, c->stream));
    if (int rw = wait_polling(c, c->ev1)) return rw;
    TRM_HIP(c, hipEventElapsedTime(ms, c->ev0, c->ev1));
    return TRM_OK;
}
}  // namespace

int trm_step_timed(trm_ctx* c, double dt, int nsteps, int finalize, float* ms) {
    TRM_ENTER_KEEP(c);
    c->heun_pending = false;
    if (nsteps < 0 || !ms) return fail(c, TRM_EINVAL, "trm_step_timed: bad argument");
    state_changed(c);
    TRM_HIP(c, hipEventRecord(c->ev0, c->stream));
    int rc = with_ops(c, [&](auto ops) { return ops.step(c, dt, nsteps, finalize); });
    if (rc) return rc;
    return timed_tail(c, ms);
}

namespace {
// the stage's fields: a second copy of the state (fields enabled since the last call included)
int ensure_stage(trm_ctx* c) {
    int rc = alloc_fields(c, c->stage);
    if (rc) return rc;
    if (!c->has_stage) c->args_valid = false;
    c->has_stage = true;
    return TRM_OK;
}
}  // namespace

int trm_step_heun(trm_ctx* c, double dt, int nsteps, int finalize) {
    TRM_ENTER(c);
    if (nsteps < 0) return fail(c, TRM_EINVAL, "trm_step_heun: nsteps < 0");
    state_changed(c);
    if (c->veg_mode == TRM_VEGETATION_STANDALONE) return finish(c, with_ops(c, [&](auto ops) { return ops.veg_step(c, dt, nsteps, finalize, true); }));
    // (HeunPath: the stage's fields exist for every path but the one launch of <= 64 levels, which keeps the stage in registers)
    if (with_ops(c, [&](auto ops) { return ops.heun_path(c); }) != HEUN_ONE_LAUNCH)
        if (int rc = ensure_stage(c)) return rc;
    for (int n = 0; n < nsteps; ++n) {
        int fin = (finalize && n == nsteps - 1) ? 1 : 0;
        int rc = with_ops(c, [&](auto ops) { return ops.heun_step(c, dt, fin); });
        if (rc) return rc;
        tick(c, dt, 1);
    }
    return finish(c, TRM_OK);
}

int trm_step_heun_timed(trm_ctx* c, double dt, int nsteps, int finalize, float* ms) {
    TRM_ENTER(c);
    if (nsteps < 0 || !ms) return fail(c, TRM_EINVAL, "trm_step_heun_timed: bad argument");
    const int async = c->opt_async;
    c->opt_async = 1;                       // (no synchronisation between the two event records)
    TRM_HIP(c, hipEventRecord(c->ev0, c->stream));
    const int rc = trm_step_heun(c, dt, nsteps, finalize);
    c->opt_async = async;
    if (rc) return rc;
    return timed_tail(c, ms);
}

// ---- Heun in two calls: the caller evaluates state-dependent forcings / boundary values at the stage in between ------------
int trm_heun_predict(trm_ctx* c, double dt) {
    TRM_ENTER_HEUN(c);
    if (c->veg_mode == TRM_VEGETATION_STANDALONE) return fail(c, TRM_EUNSUPPORTED, "trm_heun_predict: the standalone VegetationModel has no state-dependent callbacks; use trm_step_heun");
    if (int rc = ensure_stage(c)) return rc;
    c->top_valid = false;
    c->tend_valid = true;
    c->closure_consistent = false;     // (the state is untouched so far; the flag is set again by trm_heun_correct)
    state_changed(c);
    const int rc = with_ops(c, [&](auto ops) { return ops.heun_predict(c, dt, true); });
    if (rc) return rc;
    c->heun_pending = true;
    c->heun_stage_aux = false;
    c->heun_dt = dt;
    return finish(c, TRM_OK);
}

int trm_heun_stage_auxiliary(trm_ctx* c) {
    TRM_ENTER_HEUN(c);
    if (!c->heun_pending) return fail(c, TRM_EINVAL, "trm_heun_stage_auxiliary: call trm_heun_predict first");
    if (c->heun_stage_aux) return TRM_OK;
    const int rc = with_ops(c, [&](auto ops) { return ops.heun_stage_auxiliary(c); });
    if (rc) return rc;
    c->heun_stage_aux = true;
    return finish(c, TRM_OK);
}

int trm_heun_correct(trm_ctx* c, double dt, int finalize) {
    TRM_ENTER_HEUN(c);
    if (!c->heun_pending) return fail(c, TRM_EINVAL, "trm_heun_correct: call trm_heun_predict first");
    if (dt != c->heun_dt) return fail(c, TRM_EINVAL, "trm_heun_correct: dt differs from the dt of trm_heun_predict");
    c->heun_pending = false;
    state_changed(c);
    const int rc = with_ops(c, [&](auto ops) { return ops.heun_correct(c, dt, finalize, c->heun_stage_aux); });
    c->heun_stage_aux = false;
    if (rc) return rc;
    c->top_valid = false;
    c->tend_valid = true;
    c->closure_consistent = true;      // (ends with closure!)
    c->psi_consistent = false;
    tick(c, dt, 1);
    return finish(c, TRM_OK);
}

int trm_stage_field_device_ptr(trm_ctx* c, int field, void** dev, int64_t* pitch_elems) {
    TRM_ENTER_HEUN(c);
    if (!dev || !valid_field(field)) return fail(c, TRM_EINVAL, "trm_stage_field_device_ptr: bad argument");
    if (!c->state.f[field]) return fail(c, TRM_EINVAL, "trm_stage_field_device_ptr: the field exists only after trm_set_vegetation");
    if (int rc = ensure_stage(c)) return rc;
    if (field == TRM_FIELD_VWC_FORCING && !c->stage_vwc_own) {
        if (!c->opt_vwc_field) return fail(c, TRM_EINVAL, "trm_stage_field_device_ptr: upload TRM_FIELD_VWC_FORCING (or set TRM_OPT_VWC_FORCING_FIELD) first");
        TRM_HIP(c, hipMemcpyAsync(c->stage.f[field], c->state.f[field], field_elems(c, field) * c->esize, hipMemcpyDeviceToDevice, c->stream));
        c->stage_vwc_own = true;
        c->args_valid = false;
    }
    *dev = c->stage.f[field];
    if (pitch_elems) *pitch_elems = is_3d(field) ? c->Nzp : 1;
    return TRM_OK;
}

int trm_stage_bc_device_ptr(trm_ctx* c, int var, int side, void** dev) {
    TRM_ENTER_HEUN(c);
    if (!dev || var < 0 || var >= TRM_BCV_COUNT || (side != TRM_TOP && side != TRM_BOTTOM)) return fail(c, TRM_EINVAL, "trm_stage_bc_device_ptr: bad argument");
    if (c->bc_kind[var][side] == TRM_BC_NOFLUX || !c->bc_value[var][side]) return fail(c, TRM_EINVAL, "trm_stage_bc_device_ptr: the condition carries no values (set it with trm_set_bc first)");
    for (const auto& sr : c->series)
        if (sr.is_bc && sr.var == var && sr.side == side) return fail(c, TRM_EINVAL, "trm_stage_bc_device_ptr: the boundary values are evaluated from a time series at both stages");
    c->bc_zero_gradient[var][side] = false;      // (the stage's values become the caller's)
    const size_t bytes = (size_t)c->Nh * c->esize;
    if (!c->bc_value_stage[var][side]) {
        TRM_HIP(c, hipMalloc(&c->bc_value_stage[var][side], bytes));
        c->args_valid = false;
    }
    if (!c->stage_bc_user[var][side]) {
        TRM_HIP(c, hipMemcpyAsync(c->bc_value_stage[var][side], c->bc_value[var][side], bytes, hipMemcpyDeviceToDevice, c->stream));
        c->stage_bc_user[var][side] = true;
    }
    *dev = c->bc_value_stage[var][side];
    return TRM_OK;
}

// ---- time averages ---------------------------------------------------------------------------------------------------------
static trm_ctx::Average* average_of(trm_ctx* c, int h, const char* who) {
    if (h < 0 || h >= (int)c->averages.size() || c->averages[(size_t)h].field < 0) {
        fail(c, TRM_EINVAL, std::string(who) + ": not an open accumulator handle");
        return nullptr;
    }
    return &c->averages[(size_t)h];
}
int trm_average_open(trm_ctx* c, int field, int* handle) {
    TRM_ENTER_HEUN(c);
    if (!handle || !valid_field(field)) return fail(c, TRM_EINVAL, "trm_average_open: bad argument");
    if (!averageable(c, field))
        return fail(c, TRM_EUNSUPPORTED, "trm_average_open: this field cannot be averaged (soil state, closures, surface excess water, water "
                                         "table, and the LandModel's surface diagnostics can)");
    size_t h = 0;
    while (h < c->averages.size() && c->averages[h].field >= 0) ++h;
    if (h == c->averages.size()) c->averages.emplace_back();
    trm_ctx::Average& a = c->averages[h];
    const size_t bytes = field_elems(c, field) * sizeof(double);
    TRM_HIP(c, hipMalloc(&a.d_sum, bytes));
    TRM_HIP(c, hipMemsetAsync(a.d_sum, 0, bytes, c->stream));
    a.field = field;
    a.window = 0.0;
    a.steps = 0;
    *handle = (int)h;
    return finish(c, TRM_OK);
}
int trm_average_reset(trm_ctx* c, int handle) {
    TRM_ENTER_HEUN(c);
    trm_ctx::Average* a = average_of(c, handle, "trm_average_reset");
    if (!a) return TRM_EINVAL;
    TRM_HIP(c, hipMemsetAsync(a->d_sum, 0, field_elems(c, a->field) * sizeof(double), c->stream));
    a->window = 0.0;
    a->steps = 0;
    return finish(c, TRM_OK);
}
int trm_average_read(trm_ctx* c, int handle, void* host, double* window_seconds, int64_t* steps) {
    TRM_ENTER_HEUN(c);
    trm_ctx::Average* a = average_of(c, handle, "trm_average_read");
    if (!a) return TRM_EINVAL;
    if (!host) return fail(c, TRM_EINVAL, "trm_average_read: host is NULL");
    if (a->steps == 0) return fail(c, TRM_ESTALE, "trm_average_read: the window holds no step yet");
    const size_t n = field_elems(c, a->field);
    std::vector<double> sum(n);
    TRM_HIP(c, hipMemcpyAsync(sum.data(), a->d_sum, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    // mean = sum / window, rounded once to the context precision; [rows][Nh] as trm_download
    const long rows = is_3d(a->field) ? c->Nz : 1, pitch = is_3d(a->field) ? c->Nzp : 1;
    for (long k = 0; k < rows; ++k)
        for (long i = 0; i < c->Nh; ++i) {
            const double m = sum[(size_t)i * pitch + k] / a->window;
            if (c->precision == TRM_F64) ((double*)host)[(size_t)k * c->Nh + i] = m;
            else ((float*)host)[(size_t)k * c->Nh + i] = (float)m;
        }
    if (window_seconds) *window_seconds = a->window;
    if (steps) *steps = a->steps;
    return TRM_OK;
}
int trm_average_close(trm_ctx* c, int handle) {
    TRM_ENTER_HEUN(c);
    trm_ctx::Average* a = average_of(c, handle, "trm_average_close");
    if (!a) return TRM_EINVAL;
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    TRM_HIP(c, hipFree(a->d_sum));
    *a = trm_ctx::Average{};
    return TRM_OK;
}

// ---- vegetation ---------------------------------------------------------------------------
int trm_default_vegetation_params(trm_vegetation_params* p) {
    if (!p) return TRM_EINVAL;
    // photosynthesis.jl:17-68
    p->tau25 = 2600.0; p->Kc25 = 30.0; p->Ko25 = 3.0e4; p->q10_tau = 0.57; p->q10_Kc = 2.1; p->q10_Ko = 1.2; p->alpha_leaf = 0.17;
    p->alpha_a = 0.5; p->alpha_C3 = 0.08; p->cq = 4.6e-6; p->k_ext = 0.5; p->T_CO2_high = 42.0; p->T_CO2_low = -4.0;
    p->T_photos_high = 30.0; p->T_photos_low = 15.0; p->theta_r = 0.7;
    p->g1 = 2.3; p->g_min = 0.5;                                              // stomatal_conductance.jl:16-24
    p->cn_sapwood = 330.0; p->cn_root = 29.0; p->aws = 10.0;                  // autotrophic_respiration.jl:14-23
    p->SLA = 10.0; p->awl = 2.0; p->LAI_min = 1.0; p->LAI_max = 6.0; p->gamma_L = 0.3; p->gamma_R = 0.3; p->gamma_S = 0.05;   // carbon_dynamics.jl:18-43
    p->nu_seed = 0.001; p->gamma_v_min = 0.002;                               // vegetation_dynamics.jl:15-22
    p->root_a = 7.0; p->root_b = 2.0;                                         // root_distribution.jl:23-29
    p->wilting_point = 0.05; p->field_capacity = 0.25;                        // soil_hydraulic_properties.jl:74-80
    p->C_mass = 12.0;                                                         // physical_constants.jl:50
    p->alpha_int = 0.2; p->canopy_k_ext = 0.5; p->w_can_max = 2.0e-4; p->tau_w = 86400.0;   // canopy_interception.jl:37-49
    p->C_can = 0.006;                                                         // canopy_evapotranspiration.jl:33-40
    return TRM_OK;
}

int trm_set_vegetation(trm_ctx* c, const trm_vegetation_params* p, int mode) {
    TRM_ENTER(c);
    if (!p || mode < TRM_VEGETATION_OFF || mode > TRM_VEGETATION_COUPLED) return fail(c, TRM_EINVAL, "trm_set_vegetation: bad argument");
    if (mode == TRM_VEGETATION_COUPLED && !c->params.seb)
        return fail(c, TRM_EINVAL, "trm_set_vegetation: TRM_VEGETATION_COUPLED needs a LandModel context (surface_energy_balance = 1)");
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    c->veg_params = *p;
    const bool first = c->veg_mode == TRM_VEGETATION_OFF && mode != TRM_VEGETATION_OFF && !c->state.f[TRM_FIELD_ROOT_FRACTION];
    c->veg_mode = mode;
    c->args_valid = false;
    if (mode == TRM_VEGETATION_OFF) return TRM_OK;
    int rc = alloc_fields(c, c->state);          // the 3-D vegetation fields
    if (rc) return rc;
    if (first) {
        // input defaults: CO2 380 ppm (prescribed_atmosphere.jl:14), soil moisture limiting factor 1 (photosynthesis.jl:76),
        // ground temperature 10 degC (autotrophic_respiration.jl:38)
        const struct { int f; double v; } defaults[] = {{TRM_FIELD_CO2, 380.0}, {TRM_FIELD_SOIL_MOISTURE_LIMITING_FACTOR, 1.0},
                                                       {TRM_FIELD_VEGETATION_GROUND_TEMPERATURE, 10.0}};
        for (auto& d : defaults) {
            rc = fill_input_row(c, d.f, d.v);
            if (rc) return rc;
        }
    }
    return by_precision(c->precision, [&](auto nf) { return upload_root_fraction<typename decltype(nf)::type>(c); });
}

int trm_compute_plant_available_water(trm_ctx* c) {
    TRM_ENTER(c);
    if (c->veg_mode == TRM_VEGETATION_OFF) return fail(c, TRM_EINVAL, "trm_compute_plant_available_water: call trm_set_vegetation first");
    return finish(c, with_ops(c, [&](auto ops) { return ops.plant_available_water(c, c->state, true); }));
}

namespace {
int step_all(trm_ctx** ctxs, int n, const char* who, int (*step)(trm_ctx*, double, int, int), double dt, int nsteps, int finalize) {
    if (int rc = check_ctx_list(ctxs, n, who)) return rc;
    // every context is stepped without waiting for it (each on its own stream, each device running its shard), then ONE wait
    // per context -- unless the caller drives them asynchronously anyway
    std::vector<int> async((size_t)n);
    int rc = TRM_OK;
    // The steps are dealt to the devices launch by launch -- every context receives the steps of ONE of its launches (1, or up to
    // 50 with the resident program) before the next context is visited -- so that all devices start at once instead of device
    // d waiting for the host to have enqueued all nsteps launches of devices 0 .. d - 1.  Same results as one call per context
    // (a call of m steps equals m calls of one step, bit for bit).
    // A context that launches per step (steps_per_launch = 1, or a model the resident program does not take: generic boundary
    // kinds, the coupled vegetation, Heun) would receive 50 launches before the next device is visited: the chunk is the smallest
    // number of steps ONE launch of any context covers.
    int chunk = 50;
    const bool heun = step == trm_step_heun;
    for (int i = 0; i < n; ++i) {
        async[(size_t)i] = ctxs[i]->opt_async;
        ctxs[i]->opt_async = 1;
        chunk = std::min(chunk, heun ? 1 : with_ops(ctxs[i], [&](auto ops) { return ops.steps_per_launch_now(ctxs[i]); }));
    }
    int failed = -1;
    for (int done = 0; done < nsteps && !rc; done += chunk) {
        const int m = std::min(chunk, nsteps - done);
        const int fin = (finalize && done + m == nsteps) ? 1 : 0;
        for (int i = 0; i < n && !rc; ++i) {
            rc = step(ctxs[i], dt, m, fin);
            if (rc) failed = i;
        }
    }
    if (nsteps == 0 && finalize)
        for (int i = 0; i < n && !rc; ++i) {
            rc = step(ctxs[i], dt, 0, finalize);
            if (rc) failed = i;
        }
    for (int i = 0; i < n; ++i) ctxs[i]->opt_async = async[(size_t)i];
    for (int i = 0; i < n; ++i) {
        if (async[(size_t)i] && failed < 0) continue;
        const int rs = trm_synchronize(ctxs[i]);      // (also after a failure: nothing is left running behind the caller's back)
        if (!rc) { rc = rs; if (rs) failed = i; }
    }
    if (failed >= 0) {
        // the contexts stand at different clocks now: say which one failed and where every one stands (its message moves to
        // the first context, where a caller that holds only the list looks)
        std::string msg = std::string(who) + ": context " + std::to_string(failed) + " failed: " + ctxs[failed]->err + " [iterations:";
        for (int i = 0; i < n; ++i) msg += " " + std::to_string((long long)ctxs[i]->iteration);
        msg += "]";
        for (int i = 0; i < n; ++i) ctxs[i]->err = msg;
    }
    return rc;
}
}  // namespace
int trm_step_all(trm_ctx** ctxs, int n, double dt, int nsteps, int finalize) {
    return step_all(ctxs, n, "trm_step_all", trm_step, dt, nsteps, finalize);
}
int trm_step_heun_all(trm_ctx** ctxs, int n, double dt, int nsteps, int finalize) {
    return step_all(ctxs, n, "trm_step_heun_all", trm_step_heun, dt, nsteps, finalize);
}

}  // extern "C"
