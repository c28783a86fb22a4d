// Exercises the dispatch from a decided launch to its kernel instance (trm_dispatch.hpp and the trm_launch_column*.inl files on top of it) on
// values and contexts built by hand: no GPU call -- TRM_LAUNCH counts the launches instead of making them, so no kernel is instantiated.
// Built with the host sanitizers and run by `make -C terrarium.jl_amd/csrc check-preconditions` (cross-compiles; runs without a GPU).
static int g_launches = 0;
#define TRM_LAUNCH(c, K, grid, block, ...) \
    do { (void)(c); (void)(grid); (void)(block); ++g_launches; } while (0)
#include "trm_host.hpp"
#include <algorithm>
#include <cassert>
// the launch files under test, with the explicit instantiations the library has of them
#include "trm_launch_column_f64_euler_rich.hip"
#include "trm_launch_column_f64_euler_noflow.hip"
#include "trm_launch_column_f64_heun.hip"
#include "trm_launch_column_f64_multi_rich.hip"
#include "trm_launch_column_f64_multi_noflow.hip"
#include "trm_launch_column_f32_euler.hip"
#include "trm_launch_column_f32_heun.hip"
#include "trm_launch_column_f32_multi.hip"
#include "trm_launch_column_sig_f64_noflow.hip"
#include "trm_launch_column_sig_f64_rich_a.hip"
#include "trm_launch_column_sig_f64_rich_b.hip"
#include "trm_launch_column_sig_f64_rich_c.hip"
#include "trm_launch_column_sig_heun_f64_a.hip"
#include "trm_launch_column_sig_heun_f64_b.hip"
#include "trm_launch_column_sig_heun_f64_c.hip"
#include "trm_launch_column_psi_f64_a.hip"
#include "trm_launch_column_psi_f64_b.hip"
#include "trm_launch_column_psi_f64_c.hip"
#include "trm_launch_column_psi_f64_d.hip"
#include "trm_launch_column_land_bc.hip"
#include "trm_launch_column_land_vg.hip"
#include "trm_launch_packed.hip"
#include <sys/wait.h>
#include <unistd.h>

namespace trmh {
static std::string g_error;
int fail(trm_ctx*, int code, const std::string& msg) { g_error = msg; return code; }
template <class NF> const LaunchArgs<NF>& launch_args(trm_ctx*) { static LaunchArgs<NF> a{}; return a; }
int front_args(trm_ctx*, const char*, FrontArgs& fa) { fa = FrontArgs{}; fa.chain_blocks = 1; return TRM_OK; }
}  // namespace trmh
using namespace trmh;

// ---- the helpers: each listed value reaches the callback once with its constant; an unlisted one reaches nothing --------------------
struct Seen { int calls = 0, a = -99, b = -99; };
template <class D> static Seen one(D&& dispatch, bool expect) {
    Seen s;
    const bool found = dispatch([&](auto k) { ++s.calls; s.a = decltype(k)::value; });
    assert(found == expect && s.calls == (expect ? 1 : 0));
    return s;
}
static void check_helpers() {
    for (int v : {-1, 0, 3, 5, 7, 9}) {
        const bool listed = v == 3 || v == 5 || v == 9;
        const Seen s = one([&](auto f) { return by_value<3, 5, 9>(v, f); }, listed);
        assert(!listed || s.a == v);
    }
    for (int h : {HYD_BC_LINEAR, HYD_VG_N2, HYD_GENERIC}) {
        assert(one([&](auto f) { return by_hyd(h, f); }, true).a == h);
        const Seen s = one([&](auto f) { return by_compiled_hyd(h, f); }, h != HYD_GENERIC);      // (never van Genuchten for the generic one)
        assert(h == HYD_GENERIC || s.a == h);
    }
    one([&](auto f) { return by_hyd(7, f); }, false);
    for (int nz : {1, 30, 32, 33, 40, 64}) assert(one([&](auto f) { return by_lanes(nz, f); }, true).a == (nz > 32 ? 64 : 32));
    for (bool b : {false, true}) assert(one([&](auto f) { return by_bool(b, f); }, true).a == (b ? 1 : 0));
    // what rides along with a derivative launch: each of the five rides reaches its constant once; a value off the list reaches none
    int ride_calls[5] = {};
    for (int r = -1; r <= 5; ++r) {
        const bool listed = r >= RIDE_NONE && r <= RIDE_PARAM_SERIES;
        const Seen s = one([&](auto f) { return by_ride(r, f); }, listed);
        if (listed) { assert(s.a == r); ++ride_calls[s.a]; }
    }
    for (int n : ride_calls) assert(n == 1);
    by_ride(RIDE_PARAM_SERIES, [](auto k) { static_assert(std::is_same<typename decltype(k)::value_type, Ride>::value, "the constant is a Ride"); });
    for (int st : {0, 1, 2})
        for (int sc : {0, 1, 3}) {
            Seen s;
            const bool found = by_io(st, sc, [&](auto ST, auto SC) { ++s.calls; s.a = ST(); s.b = SC(); });
            assert(found == (st || sc) && s.calls == (found ? 1 : 0));
            assert(!found || (s.a == (st != 0) && s.b == (sc != 0)));
        }
    // the signature list against the parent's lists: launch_by_signature's five (two under Richards alone), column_psi_supported's four
    const int all[] = {0, 2, 6, 64, 34}, rich_only[] = {64, 34}, psi[] = {0, 2, 6, 34};
    assert(kSignatureCount == 5);
    for (int sig = -1; sig < 128; ++sig) {
        const bool in_all = std::find(std::begin(all), std::end(all), sig) != std::end(all);
        const bool in_rich = std::find(std::begin(rich_only), std::end(rich_only), sig) != std::end(rich_only);
        const bool in_psi = std::find(std::begin(psi), std::end(psi), sig) != std::end(psi);
        assert(signature_has_instance(sig, true) == in_all && signature_has_instance(sig, false) == (in_all && !in_rich));
        assert(column_psi_supported(sig) == in_psi);
        assert(!in_all || one([&](auto f) { return by_signature<true>(sig, f); }, true).a == sig);
        if (!in_all) one([&](auto f) { return by_signature<true>(sig, f); }, false);
        assert(!(in_all && !in_rich) || one([&](auto f) { return by_signature<false>(sig, f); }, true).a == sig);
        if (!in_all || in_rich) one([&](auto f) { return by_signature<false>(sig, f); }, false);
        assert(!in_psi || one([&](auto f) { return by_psi_signature(sig, f); }, true).a == sig);
        if (!in_psi) one([&](auto f) { return by_psi_signature(sig, f); }, false);
        const bool packed = sig == 64 || sig == 2;      // (trm_launch_packed.hip at the parent: BCSIG_LAND, BCSIG_T_TOP)
        assert(!packed || one([&](auto f) { return by_packed_signature(sig, f); }, true).a == sig);
        if (!packed) one([&](auto f) { return by_packed_signature(sig, f); }, false);
    }
}

// ---- every plan of StepPolicy::plan_step for k_column / k_column_land names a tuple the launchers accept ------------------------------
// the id the parent's launch_column / launch_column_land wrote out by hand per branch, from the plan
template <class NF> static int expected_id(const trm_ctx& c, const StepPlan& s, int prog) {
    using P = Policy<NF>;
    const bool f64 = std::is_same<NF, double>::value, rich = P::richards(&c);
    const int H = P::hyd(&c), LPC = c.Nz > 32 ? 64 : 32;
    const int plain[] = {0, 2, 6}, richards[] = {64, 34};
    auto listed = [&](int sig) { return f64 && (std::find(std::begin(plain), std::end(plain), sig) != std::end(plain) || (rich && std::find(std::begin(richards), std::end(richards), sig) != std::end(richards))); };
    if (prog == PROG_MULTI) return program_id(TRM_PROGRAM_COLUMN_MULTI, H, LPC, DERIVE_NONE, 0, 1, -1) | (c.params.seb ? 1 << 25 : 0) | (c.series.empty() ? 0 : 1 << 26);
    if (prog == PROG_HEUN) {
        if (s.route == ROUTE_SURFACE_IN_LAUNCH) return program_id(TRM_PROGRAM_COLUMN_LAND, H, LPC, DERIVE_NONE, 0, 1, BCSIG_LAND) | (PROG_HEUN << 25);
        const int hsig = (c.opt_bc_signature && H != HYD_GENERIC) ? bc_signature_of(&c) : -1;
        return program_id(TRM_PROGRAM_COLUMN_HEUN, H, LPC, DERIVE_NONE, 0, 1, listed(hsig) ? hsig : -1);
    }
    if (s.route == ROUTE_SURFACE_IN_LAUNCH) return program_id(TRM_PROGRAM_COLUMN_LAND, H, LPC, s.derive, s.staged, s.scalar_in, BCSIG_LAND);
    if (s.psi_form != PSI_STORED) return program_id(TRM_PROGRAM_COLUMN_EULER, H, LPC, DERIVE_T_LIQ, s.staged, s.scalar_in, s.sig);
    if (listed(s.sig)) return s.derive == DERIVE_T_LIQ ? program_id(TRM_PROGRAM_COLUMN_EULER, H, LPC, DERIVE_T_LIQ, s.staged, s.scalar_in, s.sig) : program_id(TRM_PROGRAM_COLUMN_EULER, H, LPC, DERIVE_NONE, 0, 1, s.sig);
    if (s.derive == DERIVE_T_LIQ) return f64 ? program_id(TRM_PROGRAM_COLUMN_EULER, H, LPC, DERIVE_T_LIQ, s.staged, s.scalar_in, -1) : program_id(TRM_PROGRAM_COLUMN_EULER, H, LPC, DERIVE_T_LIQ, 0, 1, -1);
    return program_id(TRM_PROGRAM_COLUMN_EULER, H, LPC, DERIVE_NONE, 0, 1, -1);
}
static long g_plans = 0, g_accepted = 0, g_psi = 0, g_front = 0, g_packed = 0, g_land_pk = 0, g_io[2][2] = {};
template <class NF> static void check_plan(trm_ctx& c, int prog, bool not_last, bool behind) {
    const StepPlan s = StepPolicy<NF>::plan_step(&c, prog, not_last, behind);
    ++g_plans;
    if (s.refusal || (s.route != ROUTE_COLUMN && s.route != ROUTE_SURFACE_IN_LAUNCH && s.route != ROUTE_PACKED)) return;
    g_launches = 0;
    g_error.clear();
    c.last_program = 0;
    int rc = TRM_OK;
    const bool rich = Policy<NF>::richards(&c);
    if (s.route == ROUTE_PACKED) rc = PackedLaunch::step(&c, 60.0, 0);      // (k_step_pk chooses its own instance: it must have one)
    else if (s.route == ROUTE_SURFACE_IN_LAUNCH) {
        if constexpr (std::is_same<NF, float>::value) rc = PackedLaunch::step_land(&c, 60.0, 0);
        else rc = FrontLaunch::run(&c, s, 60.0, 0, prog == PROG_HEUN);
    } else by_value<PROG_EULER, PROG_HEUN, PROG_MULTI>(prog, [&](auto PROG) { by_bool(rich, [&](auto RICH) { rc = ColumnLaunch<NF, RICH(), PROG()>::run(&c, s, 60.0, 0, prog == PROG_MULTI ? 4 : 1); }); });
    if (rc != TRM_OK || g_launches != 1) {
        std::fprintf(stderr, "plan not accepted: rc %d \"%s\" launches %d; f%d prog %d flow %d hyd %d seb %d Nz %d derive %d staged %d scalar_in %d sig %d psi %d\n", rc, g_error.c_str(),
                     g_launches, (int)sizeof(NF) * 8, prog, (int)rich, Policy<NF>::hyd(&c), c.params.seb, c.Nz, s.derive, s.staged, s.scalar_in, s.sig, s.psi_form);
        std::abort();
    }
    if (s.route == ROUTE_PACKED) { ++g_packed; return; }
    if (!(s.route == ROUTE_SURFACE_IN_LAUNCH && std::is_same<NF, float>::value)) assert(c.last_program == expected_id<NF>(c, s, prog));
    ++g_accepted;
    g_psi += s.psi_form != PSI_STORED;
    g_front += s.route == ROUTE_SURFACE_IN_LAUNCH;
    if (prog == PROG_EULER && s.derive == DERIVE_T_LIQ) g_io[s.staged][s.scalar_in] += 1;
}
static void check_plans() {
    static double x[4];
    for (int f32 = 0; f32 < 2; ++f32)
    for (int flow : {TRM_FLOW_RICHARDS, TRM_FLOW_NOFLOW})
    for (int hyd : {HYD_BC_LINEAR, HYD_VG_N2, HYD_GENERIC})
    for (int seb = 0; seb < 2; ++seb)
    for (int nz : {30, 40, 100, 200})
    for (int kinds = 0; kinds < 5; ++kinds)         // no condition; T top; T top + energy flux bottom; T top + infiltration; T bottom (no instance)
    for (int derive : {0, 1, 2})
    for (int consistent = 0; consistent < 2; ++consistent)
    for (int tops = 0; tops < 2; ++tops)             // (the LandModel's top-cell arrays current: the surface processes in the launch)
    for (long nh : {67L, 30000L}) {
        trm_ctx c;
        std::memset(&c.params, 0, sizeof c.params);
        c.precision = f32 ? TRM_F32 : TRM_F64;
        c.esize = f32 ? 4 : 8;
        c.params.flow = flow;
        c.params.seb = seb;
        if (hyd == HYD_VG_N2) { c.params.swrc = TRM_SWRC_VAN_GENUCHTEN; c.params.unsat_k = TRM_UNSATK_VAN_GENUCHTEN; c.params.vg_n = 2.0; }
        else { c.params.swrc = TRM_SWRC_BROOKS_COREY; c.params.unsat_k = TRM_UNSATK_LINEAR; c.params.bc_lambda = hyd == HYD_GENERIC ? 0.3 : 0.2; }
        c.Nh = nh; c.Nz = nz; c.Nzp = nz <= 32 ? 32 : nz <= 64 ? 64 : nz;
        c.opt_derive = derive;
        c.opt_interior = 1;
        c.closure_consistent = consistent != 0;
        c.psi_consistent = consistent != 0;
        if (kinds >= 1 && kinds <= 3) c.bc_kind[TRM_BCV_TEMPERATURE][TRM_TOP] = TRM_BC_VALUE;
        if (kinds == 2) c.bc_kind[TRM_BCV_INTERNAL_ENERGY][0] = TRM_BC_FLUX;
        if (kinds == 3) c.bc_kind[TRM_BCV_SATURATION_WATER_ICE][TRM_TOP] = TRM_BC_FLUX;
        if (kinds == 4) c.bc_kind[TRM_BCV_TEMPERATURE][0] = TRM_BC_VALUE;
        if (tops) { c.top_valid = true; c.d_top3 = x; }
        for (int packed = 0; packed < (f32 ? 2 : 1); ++packed) {
            c.opt_packed = packed;
            // the interleaved fp32 LandModel launch (Ops::interleave_now: a Richards LandModel on the packed path, one level per lane)
            if (f32 && seb && flow == TRM_FLOW_RICHARDS && nz <= 64 && Policy<float>::packed_path(&c)) {
                c.part_n[0] = nh / 2; c.part_n[1] = nh - nh / 2; c.part_lo[1] = nh / 2;
                g_launches = 0;
                const int rc = LandLaunch<float>::run(&c, 0, 1, 60.0, 0, false);
                assert(rc == TRM_OK && g_launches == 1);
                ++g_land_pk;
            }
            for (int prog : {PROG_EULER, PROG_HEUN, PROG_MULTI})
                for (int where = 0; where < (prog == PROG_EULER ? 4 : 1); ++where) {
                    if (f32) check_plan<float>(c, prog, (where & 1) != 0, (where & 2) != 0);
                    else check_plan<double>(c, prog, (where & 1) != 0, (where & 2) != 0);
                }
        }
    }
}

int main() {
    check_helpers();
    // TRM_STAGED_SMALL / TRM_SCALAR_INPUTS are read once per process: one child per forced (staged, scalar_in) pair, and one with neither
    for (int forced = -1; forced < 4; ++forced) {
        std::fflush(nullptr);
        const pid_t pid = fork();
        assert(pid >= 0);
        if (pid == 0) {
            if (forced >= 0) { setenv("TRM_STAGED_SMALL", (forced & 1) ? "1" : "0", 1); setenv("TRM_SCALAR_INPUTS", (forced & 2) ? "1" : "0", 1); }
            else { unsetenv("TRM_STAGED_SMALL"); unsetenv("TRM_SCALAR_INPUTS"); }
            check_plans();
            std::printf("  forced pair %d: %ld plans, %ld launched (%ld on k_column_psi, %ld with the surface processes in the launch); deriving, by (staged, scalar_in): (0, 1) %ld, (1, 0) %ld, (1, 1) %ld\n",
                        forced, g_plans, g_accepted, g_psi, g_front, g_io[0][1], g_io[1][0], g_io[1][1]);
            std::printf("    and %ld on k_step_pk, %ld on k_land_pk\n", g_packed, g_land_pk);
            assert(g_accepted > 1000 && g_psi > 0 && g_front > 0 && g_packed > 0 && g_land_pk > 0 && g_io[0][0] == 0);
            if (forced == 1) assert(g_io[1][0] > 0 && g_io[0][1] == 0);      // (staged, vector loads)
            if (forced == 3) assert(g_io[1][1] > 0 && g_io[1][0] > 0);       // ((1, 1) for the LandModel and the run-time kinds alone)
            std::fflush(nullptr);
            _exit(0);
        }
        int status = 0;
        assert(waitpid(pid, &status, 0) == pid);
        assert(WIFEXITED(status) && WEXITSTATUS(status) == 0);
    }
    std::puts("launch dispatch ok");
    return 0;
}
