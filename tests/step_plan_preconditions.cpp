// Exercises the plan of a fused step launch (StepPolicy::plan_step, trm_host.hpp) on contexts built by hand: no GPU call.
// Built with the host sanitizers and run by `make -C terrarium.jl_amd/csrc check-preconditions` (cross-compiles; runs without a GPU).
#include "trm_host.hpp"
#include <cassert>

namespace trmh {
int fail(trm_ctx*, int code, const std::string&) { return code; }
template <class NF> const LaunchArgs<NF>& launch_args(trm_ctx*) { static LaunchArgs<NF> a{}; return a; }
}  // namespace trmh
using namespace trmh;

// fp64, Richards, Brooks-Corey with lambda = 0.2 (the compiled hydraulics), 67 columns x 32 levels, no surface energy balance, T / liq
// derived on request and consistent, no boundary kinds set
static trm_ctx base() {
    trm_ctx c;
    std::memset(&c.params, 0, sizeof c.params);
    c.params.flow = TRM_FLOW_RICHARDS;
    c.params.swrc = TRM_SWRC_BROOKS_COREY;
    c.params.unsat_k = TRM_UNSATK_LINEAR;
    c.params.bc_lambda = 0.2;
    c.Nh = 67; c.Nz = 32; c.Nzp = 32;
    c.opt_derive = 1;
    c.closure_consistent = true;
    return c;
}
static StepPlan euler(const trm_ctx& c, bool not_last = false, bool behind_interior = false) { return StepPolicy<double>::plan_step(&c, PROG_EULER, not_last, behind_interior); }
static bool io(const StepPlan& s, int staged, int scalar_in) { return s.staged == staged && s.scalar_in == scalar_in; }

int main() {
    static double x[4];
    {   // the base context: the deriving signature instance, T / liq left unstored
        trm_ctx c = base();
        const StepPlan s = euler(c);
        assert(s.route == ROUTE_COLUMN && s.derive == DERIVE_T_LIQ && s.sig == 0 && io(s, 0, 1) && s.store_closure == 0);
        assert(s.psi_form == PSI_STORED && s.check_entry == 0 && s.derives_unread && s.psi_step && !s.refusal);
        assert(euler(c, true).psi_form == PSI_STORED);      // (psi_consistent is false: the stored pressure head is not a step launch's)
        // interior launches: not the call's last; behind one, the call's last derives the pressure head at entry
        c.psi_consistent = true;
        assert(euler(c, true).psi_form == PSI_INTERIOR && euler(c, true).check_entry == 0 && euler(c, true).store_closure == 0);
        assert(euler(c, true, true).psi_form == PSI_INTERIOR && euler(c, true, true).check_entry == 1);
        const StepPlan last = euler(c, false, true);
        assert(last.psi_form == PSI_LAST && last.check_entry == 1 && !last.refusal);
        assert(euler(c).psi_form == PSI_STORED);
        // the other programs keep the plain form
        for (int prog : {PROG_HEUN, PROG_MULTI}) {
            const StepPlan p = StepPolicy<double>::plan_step(&c, prog, true, false);
            assert(p.route == ROUTE_COLUMN && p.derive == DERIVE_NONE && p.store_closure == 1 && p.psi_form == PSI_STORED && !p.derives_unread && !p.psi_step);
        }
        // ... and a launch behind an interior launch that cannot derive the pressure head is refused
        c.opt_interior = 0;
        const StepPlan r = euler(c, false, true);
        assert(r.refusal && std::string(r.refusal) == "trm_step: the launch behind an interior launch cannot derive the pressure head");
        assert(euler(c, true).psi_form == PSI_STORED && !euler(c, true).refusal);
    }
    {   // something reads T / liq between the launches: stored every step, never interior
        trm_ctx c = base();
        c.psi_consistent = true;
        trm_ctx::Average avg;
        avg.field = TRM_FIELD_TEMPERATURE;
        c.averages.push_back(avg);
        assert(euler(c, true).store_closure == 1 && euler(c, true).psi_form == PSI_STORED && euler(c, true).derive == DERIVE_T_LIQ);
        c.d_tan[0] = x;
        assert(euler(c, true).store_closure == 1 && euler(c, true).psi_form == PSI_STORED);
        c.averages.clear();      // (the tangent state alone)
        assert(euler(c, true).store_closure == 1 && euler(c, true).psi_form == PSI_STORED);
        c.d_tan[0] = nullptr;
        assert(euler(c, true).store_closure == 0 && euler(c, true).psi_form == PSI_INTERIOR);
        c.part = 0;              // one pipeline part
        c.part_n[0] = 30; c.part_n[1] = 37; c.part_lo[1] = 30;
        assert(euler(c, true).route == ROUTE_COLUMN && euler(c, true).store_closure == 1 && euler(c, true).psi_form == PSI_STORED && !euler(c, true).derives_unread);
        c.averages.push_back(avg);
        assert(euler(c, true).store_closure == 1 && euler(c, true).psi_form == PSI_STORED);
    }
    {   // T / liq are not the closure of the stored state: read as stored
        trm_ctx c = base();
        c.closure_consistent = false;
        const StepPlan s = euler(c, true);
        assert(s.route == ROUTE_COLUMN && s.derive == DERIVE_NONE && io(s, 0, 1) && s.store_closure == 1 && s.sig == 0 && !s.derives_unread);
    }
    {   // the LandModel's launch with the surface processes inside
        trm_ctx c = base();
        c.params.seb = 1;
        c.top_valid = true;
        c.d_top3 = x;
        const StepPlan s = euler(c, true);
        assert(s.route == ROUTE_SURFACE_IN_LAUNCH && s.derive == DERIVE_T_LIQ && s.sig == BCSIG_LAND && io(s, 0, 1) && s.store_closure == 0);
        assert(s.psi_form == PSI_STORED && s.derives_unread && !s.psi_step);
        assert(StepPolicy<double>::plan_step(&c, PROG_HEUN, false, false).route == ROUTE_SURFACE_IN_LAUNCH);
        assert(StepPolicy<double>::plan_step(&c, PROG_MULTI, false, false).route == ROUTE_COLUMN);
        c.Nh = 65537;           // (beyond the size where the single launch pays)
        assert(euler(c).route == ROUTE_COLUMN && euler(c).sig == BCSIG_LAND);
        c.Nh = 67;
        c.top_escaped = true;   // (the top-cell arrays are not trusted)
        assert(euler(c).route == ROUTE_COLUMN && euler(c).store_closure == 1);
    }
    {   // fp32, the reference-default hydraulics: the packed step chooses its own instance
        trm_ctx c = base();
        c.precision = TRM_F32;
        c.esize = 4;
        const StepPlan s = StepPolicy<float>::plan_step(&c, PROG_EULER, true, false);
        assert(s.route == ROUTE_PACKED && s.store_closure == 1 && s.psi_form == PSI_STORED && !s.derives_unread);
        c.opt_packed = 0;
        const StepPlan u = StepPolicy<float>::plan_step(&c, PROG_EULER, true, false);
        assert(u.route == ROUTE_COLUMN && u.derive == DERIVE_T_LIQ && u.store_closure == 0 && u.psi_form == PSI_STORED);
    }
    {   // two levels per lane; a Gradient condition on temperature at the top
        trm_ctx c = base();
        c.Nz = 100; c.Nzp = 100;
        assert(euler(c, true).route == ROUTE_LEVELS && euler(c, true).store_closure == 1 && euler(c, true).psi_form == PSI_STORED);
        assert(euler(c, false, true).refusal);
        trm_ctx g = base();
        g.bc_kind[TRM_BCV_TEMPERATURE][TRM_TOP] = TRM_BC_GRADIENT;
        assert(euler(g, true).route == ROUTE_GENERIC && euler(g, true).store_closure == 1 && !euler(g, true).derives_unread);
    }
    {   // an open time average the multi-step program carries itself
        trm_ctx c = base();
        trm_ctx::Average avg;
        avg.field = TRM_FIELD_TEMPERATURE;
        c.averages.push_back(avg);
        assert(StepPolicy<double>::plan_step(&c, PROG_MULTI, false, false).route == ROUTE_ACCUM_IN_LAUNCH);
    }
    // the (staged, scalar_in) combinations that have instances
    int staged = 1, scalar_in = 1;
    Policy<double>::io_paths(false, staged, scalar_in);
    assert(staged == 1 && scalar_in == 0);
    staged = 1; scalar_in = 1;
    Policy<double>::io_paths(true, staged, scalar_in);
    assert(staged == 1 && scalar_in == 1);
    staged = 0; scalar_in = 0;
    Policy<double>::io_paths(true, staged, scalar_in);
    assert(staged == 0 && scalar_in == 1);
    std::puts("step plan preconditions ok");
    return 0;
}
