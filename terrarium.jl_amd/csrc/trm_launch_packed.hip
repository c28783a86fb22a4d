// trm_launch_packed.hip -- fp32 with two columns per lane and packed math (trm_packed_f32.hpp): the launches of k_step_pk and
// of k_land_pk (the interleaved LandModel launches in fp32).
#include "trm_host.hpp"
#include "trm_packed_f32.hpp"

namespace trmh {

// the workgroups that step `n` columns, two per lane
template <int LPC> static unsigned packed_blocks(long n) {
    const long pairs = (n + 1) / 2;
    const long waves = (pairs + (64 / LPC) - 1) / (64 / LPC);
    return (unsigned)((waves * 64 + TRM_STEP_BLOCK - 1) / TRM_STEP_BLOCK);
}
// (the id reports the run-time `staged` argument; BCSIG: the boundary kinds compiled in, for the signatures that have an instance)
template <bool RICH, int LPC, int H, int DERIVE, int BCSIG = BCSIG_RUNTIME> static int run_packed(trm_ctx* c, double dt, int finalize, int staged) {
    const LaunchArgs<float>& la = launch_args<float>(c);
    TRM_LAUNCH(c, (k_step_pk<RICH, LPC, H, DERIVE, BCSIG>), dim3(packed_blocks<LPC>(ncols(c))), dim3(TRM_STEP_BLOCK), state_view<float>(c), la.p, (float)dt, finalize, write_kf(c, finalize), staged);
    c->last_program = program_id(TRM_PROGRAM_PACKED_F32, H, LPC, DERIVE, staged, 1, BCSIG);
    return TRM_OK;
}
int PackedLaunch::step(trm_ctx* c, double dt, int finalize) {
    using P = Policy<float>;
    int rc = NO_INSTANCE;
    by_bool(P::richards(c), [&](auto RICH) { by_lanes(c->Nz, [&](auto LPC) { by_compiled_hyd(P::hyd(c), [&](auto H) {
        const int derive = P::derive_now<RICH()>(c);
        const int staged = P::staged_now<RICH()>(c, true);
        // (TRM_OPT_BC_SIGNATURE: the liquid fraction alone under Richards has the signature instances)
        if constexpr (RICH()) {
            if (derive == DERIVE_LIQ && c->opt_bc_signature)
                by_packed_signature(bc_signature_of(c), [&](auto SIG) { rc = run_packed<true, LPC(), H(), DERIVE_LIQ, SIG()>(c, dt, finalize, staged); });
        }
        if (rc == NO_INSTANCE)
            by_value<DERIVE_NONE, DERIVE_T_LIQ, DERIVE_LIQ, DERIVE_LIQ_PSI>(derive, [&](auto D) { rc = run_packed<RICH(), LPC(), H(), D()>(c, dt, finalize, staged); });
    }); }); });
    return launched(c, rc, "k_step_pk: no instance for this launch");
}

// k_step_pk_land: the packed LandModel step with the surface processes in the first workgroups of the launch
template <int LPC, int H, int DERIVE> static int run_packed_land(trm_ctx* c, const FrontArgs& fa, double dt, int finalize, int staged) {
    const LaunchArgs<float>& la = launch_args<float>(c);
    TRM_LAUNCH(c, (k_step_pk_land<LPC, H, DERIVE>), dim3((unsigned)fa.chain_blocks + packed_blocks<LPC>(c->Nh)), dim3(TRM_STEP_BLOCK), la.state, la.p, (float)dt, finalize, write_kf(c, finalize), staged, fa);
    c->last_program = program_id(TRM_PROGRAM_PACKED_LAND, H, LPC, DERIVE, staged, 1, BCSIG_LAND);
    return TRM_OK;
}
int PackedLaunch::step_land(trm_ctx* c, double dt, int finalize) {
    using P = Policy<float>;
    FrontArgs fa;
    if (int rc = front_args(c, "k_step_pk_land", fa)) return rc;
    const int derive = P::derive_now<true>(c), staged = P::staged_now<true>(c, true);
    if (derive != DERIVE_NONE && derive != DERIVE_LIQ) return fail(c, TRM_EINVAL, "k_step_pk_land: no instance for this derivation mode");
    int rc = NO_INSTANCE;
    by_lanes(c->Nz, [&](auto LPC) { by_compiled_hyd(P::hyd(c), [&](auto H) { by_value<DERIVE_NONE, DERIVE_LIQ>(derive, [&](auto D) {
        rc = run_packed_land<LPC(), H(), D()>(c, fa, dt, finalize, staged);
    }); }); });
    return launched(c, rc, "k_step_pk_land: no instance for the generic hydraulics");
}

// columns of part `qcol` step; the surface processes of part `qsurf` run beside them for ITS next column step (k_land_pk)
template <int H, int LPC, bool TOP_ARRAYS> static int run_land_pk(trm_ctx* c, int qcol, int qsurf, double dt, int finalize) {
    const LaunchArgs<float>& la = launch_args<float>(c);
    const unsigned sblocks = (unsigned)((c->part_n[qsurf] + TRM_STEP_BLOCK - 1) / TRM_STEP_BLOCK);
    TRM_LAUNCH(c, (k_land_pk<true, LPC, H, TOP_ARRAYS>), dim3(sblocks + packed_blocks<LPC>(c->part_n[qcol])), dim3(TRM_STEP_BLOCK), la.part[qcol], la.p, (float)dt, finalize, write_kf(c, finalize), la.part[qsurf], (int)sblocks);
    c->last_program = program_id(TRM_PROGRAM_LAND_INTERLEAVED, H, LPC, DERIVE_NONE, 0, 1, -1);
    return TRM_OK;
}
template <> int LandLaunch<float>::run(trm_ctx* c, int qcol, int qsurf, double dt, int finalize, bool top_arrays) {
    if (top_arrays && !launch_args<float>(c).part[qsurf].top_T) return fail(c, TRM_EINVAL, "LandModel launch: the top-cell arrays were requested on a context that has none");
    int rc = NO_INSTANCE;
    by_compiled_hyd(Policy<float>::hyd(c), [&](auto H) { by_lanes(c->Nz, [&](auto LPC) { by_bool(top_arrays, [&](auto TOPS) {
        rc = run_land_pk<H(), LPC(), TOPS()>(c, qcol, qsurf, dt, finalize);
    }); }); });
    return launched(c, rc, "k_land_pk: no instance for the generic hydraulics");
}

}  // namespace trmh
