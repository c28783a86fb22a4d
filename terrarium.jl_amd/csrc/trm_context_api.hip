// trm_context_api.hip -- the context of the C ABI of libterrarium_hip.so (include/terrarium_hip.h): its construction and destruction, the
// launch-argument cache, the environment switches, the clock, status and options, saving and restoring the state.  It defines the small host
// pieces every trm_*_api.hip file uses (fail, finish, tick, bc_changed / state_changed, flush_closure, io_buffer, alloc_fields,
// fill_input_row; trm_host.hpp declares them).  trm_save_state / trm_restore_state sit here, not with field I/O: they copy every field
// the context owns and its clock.  Host code alone: no kernel is launched from this file.  gfx950 only; no CPU fallback.
#include "trm_host.hpp"

using namespace trm;
using namespace trmh;

namespace {
thread_local std::string g_create_error;
}  // namespace

namespace trmh {
int fail(trm_ctx* ctx, int code, const std::string& msg) {
    if (ctx) ctx->err = msg;
    else g_create_error = msg;
    return code;
}
}  // namespace trmh

namespace {

// ---- grid: ColumnGrid (column_grid.jl:20-34) + Oceananigans' stretched-coordinate recipe --------------
// thickness[0] is the surface layer.  All derived quantities are formed in NF.
template <class NF> struct HostGrid {
    std::vector<NF> zF, zC, dzc, rdzc, rdzf, dzf, psiz;  // faces 0..Nz ; centres 0..Nz-1
    NF dzf_bot, dzf_top;
    void build(int Nz, const double* thickness) {
        // z_coords = convert.(NF, vcat(-reverse(cumsum(z_thick)), 0))
        std::vector<double> cs(Nz);
        double acc = thickness[0];
        cs[0] = acc;
        for (int n = 1; n < Nz; ++n) { acc = acc + thickness[n]; cs[n] = acc; }
        zF.resize(Nz + 1);
        for (int f = 0; f < Nz; ++f) zF[f] = (NF)(-cs[Nz - 1 - f]);
        zF[Nz] = NF(0);
        // halo faces continue with the boundary cell's spacing (Bounded topology)
        NF Fm1 = zF[0] - (zF[1] - zF[0]);
        NF Fp1 = zF[Nz] + (zF[Nz] - zF[Nz - 1]);
        zC.resize(Nz);
        dzc.resize(Nz);
        rdzc.resize(Nz);
        for (int k = 0; k < Nz; ++k) {
            zC[k] = (zF[k + 1] + zF[k]) / NF(2);
            dzc[k] = zF[k + 1] - zF[k];
            rdzc[k] = NF(1) / dzc[k];
        }
        NF Cm1 = (zF[0] + Fm1) / NF(2);
        NF Cp1 = (Fp1 + zF[Nz]) / NF(2);
        dzf.resize(Nz + 1);
        rdzf.resize(Nz + 1);
        for (int f = 0; f <= Nz; ++f) {
            NF hi = (f < Nz) ? zC[f] : Cp1;
            NF lo = (f > 0) ? zC[f - 1] : Cm1;
            dzf[f] = hi - lo;
            rdzf[f] = NF(1) / dzf[f];
        }
        dzf_bot = dzf[0];
        dzf_top = dzf[Nz];
        // elevation head psi_z = z - z_ref with z_ref the surface face (soil_hydraulic_closures.jl:112-121)
        psiz.resize(Nz);
        for (int k = 0; k < Nz; ++k) psiz[k] = zC[k] - zF[Nz];
    }
};

template <class NF> DevParams<NF> make_dev_params(const trm_params& q) {
    DevParams<NF> p;
    NF rho_soc = (NF)q.rho_soc, rho_org = (NF)q.rho_org, por_m = (NF)q.por_mineral, por_o = (NF)q.por_organic;
    p.org = rho_soc / ((NF(1) - por_o) * rho_org);               // homogeneous_strat.jl:34-44
    p.por = (NF(1) - p.org) * por_m + p.org * por_o;             // homogeneous_strat.jl:51-61
    p.rpor = NF(1) / p.por;
    p.solid_frac = NF(1) - p.por;                                // soil_volume.jl:62
    p.frac_organic = p.solid_frac * p.org;                       // soil_volume.jl:103-107
    p.frac_mineral = p.solid_frac * (NF(1) - p.org);
    p.sk_water = std::sqrt((NF)q.k_water);
    p.sk_ice = std::sqrt((NF)q.k_ice);
    p.sk_air = std::sqrt((NF)q.k_air);
    p.kterm_mineral = std::sqrt((NF)q.k_mineral) * p.frac_mineral;
    p.kterm_organic = std::sqrt((NF)q.k_organic) * p.frac_organic;
    p.c_water = (NF)q.c_water;
    p.c_ice = (NF)q.c_ice;
    p.c_air = (NF)q.c_air;
    p.cterm_mineral = (NF)q.c_mineral * p.frac_mineral;
    p.cterm_organic = (NF)q.c_organic * p.frac_organic;
    p.L = (NF)q.rho_w * (NF)q.Lsl;
    p.K_sat = (NF)q.K_sat;
    p.theta_res = (NF)q.theta_res;
    p.theta_span = p.por - p.theta_res;   // (theta_sat - theta_res) with theta_sat = por at every call site
    p.rtheta_span = NF(1) / p.theta_span;
    p.bc_psi_s = (NF)q.bc_psi_s;
    p.vg_alpha = (NF)q.vg_alpha;
    p.impedance = (NF)q.impedance;
    {   // fully frozen cells: y = -impedance * (1 - 0); Base.:^ takes pow_body(10.0, Int(y)) when y is integer-valued
        const NF y = -p.impedance * (NF(1) - NF(0));
        p.impedance_int = ((NF)(int)y == y && y > NF(-4096) && y < NF(4096)) ? 1 : 0;
        p.I_ice_frozen = p.impedance_int ? pow_int(NF(10), (int)y) : NF(0);
    }
    p.vwc_forcing = (NF)q.vwc_forcing;
    p.neg_inv_alpha = NF(-1) / p.vg_alpha;
    NF lam = (NF)q.bc_lambda, n = (NF)q.vg_n;
    NF m = NF(1) - NF(1) / n;
    p.bc_lambda = make_pow_spec<NF>(lam);
    p.bc_neg_inv_lambda = make_pow_spec<NF>(NF(-1) / lam);
    p.vg_n = make_pow_spec<NF>(n);
    p.vg_neg_m = make_pow_spec<NF>(-m);
    p.vg_neg_inv_m = make_pow_spec<NF>(NF(-1) / m);
    p.vg_inv_n = make_pow_spec<NF>(NF(1) / n);
    p.vgk_e1 = make_pow_spec<NF>(n / (n + NF(1)));
    p.vgk_e2 = make_pow_spec<NF>((n - NF(1)) / n);
    p.albedo = (NF)q.albedo;
    p.emissivity = (NF)q.emissivity;
    p.one_minus_emissivity = NF(1) - p.emissivity;
    p.eps_sigma = p.emissivity * (NF)q.sigma;
    p.sigma = (NF)q.sigma;
    p.prescribed_albedo = q.prescribed_albedo;
    p.kappa_s2 = NF(2) * (NF)q.kappa_s;
    p.rkappa_s2 = NF(1) / p.kappa_s2;
    p.C_h = (NF)q.C_h;
    p.min_windspeed = (NF)q.min_windspeed;
    p.tau_r = (NF)q.tau_r;
    p.rtau_r = NF(1) / p.tau_r;
    p.beta_evap = (NF)q.beta_evap;
    p.field_capacity = (NF)q.field_capacity;
    p.evap_resistance = q.evap_resistance;
    p.Tref = (NF)q.Tref;
    p.eps_mw = (NF)q.eps_mw;
    p.one_minus_eps_mw = NF(1) - p.eps_mw;
    p.ca_rhoa = (NF)q.c_a * (NF)q.rho_a;
    p.Llg_rhoa = (NF)q.Llg * (NF)q.rho_a;
    p.flow = q.flow;
    p.swrc = q.swrc;
    p.unsat_k = q.unsat_k;
    p.seb = q.seb;
    p.halo_policy = q.halo_policy;
    return p;
}

template <class NF> View<NF> make_view(const trm_ctx* c, const FieldSet& s) {
    View<NF> v;
    v.Nh = c->Nh;
    v.Nz = c->Nz;
    v.Nzp = c->Nzp;
    auto F = [&](int id) { return (NF*)s.f[id]; };
    v.U = F(TRM_FIELD_INTERNAL_ENERGY);
    v.sat = F(TRM_FIELD_SATURATION_WATER_ICE);
    v.T = F(TRM_FIELD_TEMPERATURE);
    v.liq = F(TRM_FIELD_LIQUID_WATER_FRACTION);
    v.psi = F(TRM_FIELD_PRESSURE_HEAD);
    v.Kf = F(TRM_FIELD_HYDRAULIC_CONDUCTIVITY);
    v.Kf_top = (NF*)s.kf_top;
    v.top_T = (NF*)c->d_top3;
    v.top_sat = v.top_T ? v.top_T + c->Nh : nullptr;
    v.top_liq = v.top_T ? v.top_T + 2 * c->Nh : nullptr;
    v.G_U = F(TRM_FIELD_TEND_INTERNAL_ENERGY);
    v.G_sat = F(TRM_FIELD_TEND_SATURATION_WATER_ICE);
    v.S = F(TRM_FIELD_SURFACE_EXCESS_WATER);
    v.G_S = F(TRM_FIELD_TEND_SURFACE_EXCESS_WATER);
    v.wt = F(TRM_FIELD_WATER_TABLE);
    v.Ts = F(TRM_FIELD_SKIN_TEMPERATURE);
    v.ghf = F(TRM_FIELD_GROUND_HEAT_FLUX);
    v.swu = F(TRM_FIELD_SURFACE_SHORTWAVE_UP);
    v.lwu = F(TRM_FIELD_SURFACE_LONGWAVE_UP);
    v.rnet = F(TRM_FIELD_SURFACE_NET_RADIATION);
    v.Hs = F(TRM_FIELD_SENSIBLE_HEAT_FLUX);
    v.Hl = F(TRM_FIELD_LATENT_HEAT_FLUX);
    v.evap = F(TRM_FIELD_EVAPORATION_GROUND);
    v.infil = F(TRM_FIELD_INFILTRATION);
    v.runoff = F(TRM_FIELD_SURFACE_RUNOFF);
    v.Tair = F(TRM_FIELD_AIR_TEMPERATURE);
    v.pres = F(TRM_FIELD_AIR_PRESSURE);
    v.wind = F(TRM_FIELD_WINDSPEED);
    v.qair = F(TRM_FIELD_SPECIFIC_HUMIDITY);
    v.rain = F(TRM_FIELD_RAINFALL);
    v.swd = F(TRM_FIELD_SURFACE_SHORTWAVE_DOWN);
    v.lwd = F(TRM_FIELD_SURFACE_LONGWAVE_DOWN);
    v.albedo = F(TRM_FIELD_ALBEDO);
    v.emissivity = F(TRM_FIELD_EMISSIVITY);
    v.zC = (const NF*)c->d_zC;
    v.zF = (const NF*)c->d_zF;
    v.dzc = (const NF*)c->d_dzc;
    v.rdzc = (const NF*)c->d_rdzc;
    v.rdzf = (const NF*)c->d_rdzf;
    v.psiz = (const NF*)c->d_psiz;
    v.lvl = (const NF*)c->d_lvl;
    // (static between the stages unless the caller evaluates a state-dependent forcing at the stage: trm_stage_field_device_ptr)
    v.Fvwc = c->opt_vwc_field ? (const NF*)((&s == &c->stage && c->stage_vwc_own) ? c->stage.f[TRM_FIELD_VWC_FORCING] : c->state.f[TRM_FIELD_VWC_FORCING]) : nullptr;
    BcGeom<NF>& g = v.g;
    g.dzf_bot = (NF)c->dzf_bot;
    g.dzf_top = (NF)c->dzf_top;
    g.hdzf_bot = g.dzf_bot / NF(2);
    g.hdzf_top = g.dzf_top / NF(2);
    g.rhdzf_bot = NF(1) / g.hdzf_bot;
    g.rhdzf_top = NF(1) / g.hdzf_top;
    g.Az = (NF)c->Az;                       // Flat y => Az = dx
    g.V_bot = g.Az * (NF)c->dzc_bot;        // V = Az * dz
    g.V_top = g.Az * (NF)c->dzc_top;
    g.rV_bot = NF(1) / g.V_bot;
    g.rV_top = NF(1) / g.V_top;
    g.zF_top = (NF)c->h_zF[c->Nz];
    g.dzc_top = (NF)c->dzc_top;
    v.status = c->d_status;
    for (int a = 0; a < TRM_BCV_COUNT; ++a)
        for (int b = 0; b < 2; ++b) {
            v.bc.kind[a][b] = c->bc_kind[a][b];
            void* val = (&s == &c->stage && c->bc_value_stage[a][b]) ? c->bc_value_stage[a][b] : c->bc_value[a][b];
            v.bc.value[a][b] = val ? val : c->d_zero;
        }
    fill_small_table(v);
    return v;
}

// The view of columns [lo, lo + n) of `v`: every per-column / per-cell pointer advanced, the per-level tables shared.
// (3-D fields are [Nh][Nzp], 2-D fields and boundary value arrays [Nh]; top_* are three [Nh] rows of one buffer.)
template <class NF> View<NF> sub_view(const View<NF>& v, long lo, long n) {
    View<NF> s = v;
    s.Nh = n;
    const long c3 = lo * v.Nzp;
    auto p3 = [&](NF*& q) { if (q) q += c3; };
    auto p2 = [&](NF*& q) { if (q) q += lo; };
    auto c2 = [&](const NF*& q) { if (q) q += lo; };
    p3(s.U); p3(s.sat); p3(s.T); p3(s.liq); p3(s.psi); p3(s.Kf); p3(s.G_U); p3(s.G_sat);
    if (s.Fvwc) s.Fvwc += c3;
    p2(s.S); p2(s.wt); p2(s.Kf_top); p2(s.G_S);
    p2(s.Ts); p2(s.ghf); p2(s.infil); p2(s.swu); p2(s.lwu); p2(s.rnet); p2(s.Hs); p2(s.Hl); p2(s.evap); p2(s.runoff);
    p2(s.top_T); p2(s.top_sat); p2(s.top_liq);
    c2(s.Tair); c2(s.pres); c2(s.wind); c2(s.qair); c2(s.rain); c2(s.swd); c2(s.lwd); c2(s.albedo); c2(s.emissivity);
    for (int a = 0; a < TRM_BCV_COUNT; ++a)
        for (int b = 0; b < 2; ++b)
            if (s.bc.value[a][b]) s.bc.value[a][b] = (const NF*)s.bc.value[a][b] + lo;
    fill_small_table(s);
    return s;
}

template <class NF> StageView<NF> make_stage_view(const trm_ctx* c) {
    // Heun: the stage's temperature boundary values (a series evaluated at t + dt), else the state's
    StageView<NF> w{};
    auto bc = [&](int side) {
        void* q = c->bc_value_stage[TRM_BCV_TEMPERATURE][side] ? c->bc_value_stage[TRM_BCV_TEMPERATURE][side] : c->bc_value[TRM_BCV_TEMPERATURE][side];
        return (const NF*)(q ? q : c->d_zero);
    };
    w.bcT_bot = bc(0);
    w.bcT_top = bc(1);
    return w;
}

}  // namespace

namespace trmh {
int front_args(trm_ctx* c, const char* kernel, FrontArgs& fa) {
    if (!c->d_top3 || !c->top_valid) return fail(c, TRM_EINVAL, std::string(kernel) + ": the surface workgroups read the top-cell arrays, which are not current");
    const size_t bytes = (size_t)c->Nh * FRONT_GRANULES * sizeof(unsigned long long);
    if (!c->d_gran) {
        TRM_HIP(c, hipMalloc((void**)&c->d_gran, bytes));
        TRM_HIP(c, hipMemsetAsync(c->d_gran, 0, bytes, c->stream));
        c->front_epoch = 0;
    }
    if (++c->front_epoch == 0) {      // (wrapped: stale granules may carry any tag again -- start over)
        TRM_HIP(c, hipMemsetAsync(c->d_gran, 0, bytes, c->stream));
        c->front_epoch = 1;
    }
    fa = FrontArgs{};
    fa.gran = c->d_gran;
    fa.epoch = c->front_epoch;
    fa.tag_bias = c->debug_handoff_tag_bias;
    fa.chain_blocks = (int)((c->Nh + TRM_STEP_BLOCK - 1) / TRM_STEP_BLOCK);
    return TRM_OK;
}
template <class NF> const LaunchArgs<NF>& launch_args(trm_ctx* c) {
    if (!c->args) {
        c->args = new LaunchArgs<NF>();
        c->args_free = [](void* q) { delete (LaunchArgs<NF>*)q; };
    }
    LaunchArgs<NF>* a = (LaunchArgs<NF>*)c->args;
    if (!c->args_valid) {
        a->p = make_dev_params<NF>(c->params);
        a->state = make_view<NF>(c, c->state);
        a->stage = make_view<NF>(c, c->stage);
        for (int q = 0; q < 2; ++q) a->part[q] = sub_view<NF>(a->state, c->part_lo[q], c->part_n[q]);
        a->w = make_stage_view<NF>(c);
        c->args_valid = true;
    }
    return *a;
}
template const LaunchArgs<double>& launch_args<double>(trm_ctx*);
template const LaunchArgs<float>& launch_args<float>(trm_ctx*);

// ---- shared with trm_derivative_api.hip (declared in trm_host.hpp) ------------------------------------------------------------------
// The state has changed behind the derivatives' backs: an open tangent needs a new seed, a tape that holds steps no longer leads to the
// stored state.  bc_changed: a boundary condition has (the backward sweep reads the values the context holds when it runs).
void bc_changed(trm_ctx* c) {
    if (!c->tape_dt.empty() || !c->tape_segs.empty()) c->adj_stale = true;
}
void state_changed(trm_ctx* c) {
    c->tan_stale = true;
    bc_changed(c);
}
// tick! per step: the same sequence of sums as per-step calls (restarts compare the clock bit for bit)
void tick(trm_ctx* c, double dt, int nsteps) {
    for (int j = 0; j < nsteps; ++j) c->time += dt;
    c->iteration += nsteps;
}
// TRM_OPT_DEFER_CLOSURE_STORES: temperature and liquid_water_fraction of the state into their arrays (one small launch on the
// context stream) if the last step launches left them unstored; nothing otherwise.  Every reader and writer of field memory other than
// a deriving per-step launch comes through here first: the ABI entries (TRM_ENTER / TRM_ENTER_HEUN) and Ops::fused_launch.
int flush_closure(trm_ctx* c) {
    if (!c->closure_deferred) return TRM_OK;
    if (int rc = by_precision(c->precision, [&](auto nf) { return MaterializeLaunch<typename decltype(nf)::type>::run(c); })) return rc;
    c->closure_deferred = false;
    c->materializations += 1;
    return TRM_OK;
}
int finish(trm_ctx* c, int rc) {
    if (rc) return rc;
    if (!c->opt_async) TRM_HIP(c, hipStreamSynchronize(c->stream));
    return TRM_OK;
}
int io_buffer(trm_ctx* c, size_t bytes) {
    if (bytes > c->io_cap) {
        if (c->d_io) TRM_HIP(c, hipFree(c->d_io));
        c->d_io = nullptr;
        c->io_cap = 0;
        TRM_HIP(c, hipMalloc(&c->d_io, bytes));
        c->io_cap = bytes;
    }
    return TRM_OK;
}
}  // namespace trmh

namespace {

// The zero fills run on the CONTEXT stream and are waited for.  A plain hipMemset goes to the null stream, which the context's
// non-blocking stream does not synchronise with: under load (two processes time-slicing one device) a fill could land AFTER a
// later upload / copy on the context stream had written the buffer and wipe it -- seen once as a NaN state in a shared-device
// rehearsal of the N > 1 bench.
// Every field starts (field id mod 32) x 16 640 bytes into its own allocation.  hipMalloc hands out identically aligned blocks, so
// column i of every field of the step (nine streams) would sit at the same offset modulo any power of two -- the same HBM
// channel and bank for all of them at the moment a wave touches them.  65 x 256 B moves each field by an odd number of 256-byte
// interleave units: measured -3.7 ... -4.7 % on the HBM-resident fp64 step (8 x N145: 210.7 -> 200.9 us, 218.1 -> 209.9 on another
// box), -3 % at C5, nothing on the cache-resident ones (profiles/r03/exp15*_skew.log).  TRM_FIELD_SKEW (bytes, a multiple of 256)
// overrides it for experiments.
// Environment switches of experiments and tests are validated once; a value outside its range makes trm_create
// fail with a message instead of silently selecting something else.
bool parse_env_int(const char* name, long lo, long hi, long multiple_of, long& out, std::string& err) {
    const char* e = std::getenv(name);
    if (!e) return false;
    char* end = nullptr;
    const long v = std::strtol(e, &end, 10);
    if (end == e || *end != 0 || v < lo || v > hi || (multiple_of > 1 && v % multiple_of != 0)) {
        err = std::string(name) + "=" + e + ": expected an integer in [" + std::to_string(lo) + ", " + std::to_string(hi) + "]" +
              (multiple_of > 1 ? " that is a multiple of " + std::to_string(multiple_of) : std::string());
        return false;
    }
    out = v;
    return true;
}
struct EnvSwitches {
    long field_skew = 16640, derive_default = -1, debug_placement = 0, handoff_tag_bias = 0, defer_closure = -1, interior_steps = -1;
    std::string error;
    EnvSwitches() {
        long v;
        if (parse_env_int("TRM_FIELD_SKEW", 0, 1 << 20, 256, v, error)) field_skew = v;
        if (error.empty() && parse_env_int("TRM_DERIVE_DEFAULT", 0, 5, 1, v, error)) derive_default = v;
        if (error.empty() && parse_env_int("TRM_DEBUG_PLACEMENT", 0, 1, 1, v, error)) debug_placement = v;   // (prints every field's allocation: profiles/tools/placement_probe.sh)
        if (error.empty() && parse_env_int("TRM_DEBUG_HANDOFF_TAG_BIAS", 0, 1, 1, v, error)) handoff_tag_bias = v;      // (tests: FrontArgs::tag_bias)
        if (error.empty() && parse_env_int("TRM_DEFER_CLOSURE_STORES", 0, 1, 1, v, error)) defer_closure = v;      // (child-process A/B)
        if (error.empty() && parse_env_int("TRM_INTERIOR_STEPS", 0, 2, 1, v, error)) interior_steps = v;         // (child-process A/B)
        if (error.empty() && parse_env_int("TRM_STAGED_SMALL", 0, 1, 1, v, error)) { /* read by Policy::staged_now */ }
        if (error.empty() && parse_env_int("TRM_SCALAR_INPUTS", 0, 1, 1, v, error)) { /* read by Policy::scalar_inputs_now */ }
    }
};
const EnvSwitches& env_switches() {
    static const EnvSwitches e;
    return e;
}
size_t field_skew_bytes() { return (size_t)env_switches().field_skew; }
}  // namespace

namespace trmh {
int alloc_fields(trm_ctx* c, FieldSet& s) {
    for (int f = 0; f < TRM_FIELD_COUNT; ++f) {
        if (is_lazy_field(f) && c->veg_mode == TRM_VEGETATION_OFF) continue;
        if (s.f[f]) continue;
        size_t bytes = field_elems(c, f) * c->esize;
        const size_t skew = field_skew_bytes() * (size_t)(f % 32);
        TRM_HIP(c, hipMalloc(&s.raw[f], bytes + skew));
        s.f[f] = (char*)s.raw[f] + skew;
        if (env_switches().debug_placement) std::fprintf(stderr, "trm placement: field %d raw %p bytes %zu skew %zu\n", f, s.raw[f], bytes, skew);
        TRM_HIP(c, hipMemsetAsync(s.f[f], 0, bytes, c->stream));
    }
    if (!s.kf_top) {
        TRM_HIP(c, hipMalloc(&s.kf_top, (size_t)c->Nh * c->esize));
        TRM_HIP(c, hipMemsetAsync(s.kf_top, 0, (size_t)c->Nh * c->esize, c->stream));
    }
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    return TRM_OK;
}
}  // namespace trmh

namespace {

template <class NF> int upload_grid(trm_ctx* c, const double* thickness) {
    HostGrid<NF> g;
    g.build(c->Nz, thickness);
    auto up = [&](void** d, const std::vector<NF>& h) -> int {
        TRM_HIP(c, hipMalloc(d, h.size() * sizeof(NF)));
        TRM_HIP(c, hipMemcpyAsync(*d, h.data(), h.size() * sizeof(NF), hipMemcpyHostToDevice, c->stream));
    TRM_HIP(c, hipStreamSynchronize(c->stream));
        return TRM_OK;
    };
    int rc;
    if ((rc = up(&c->d_zC, g.zC))) return rc;
    if ((rc = up(&c->d_zF, g.zF))) return rc;
    if ((rc = up(&c->d_dzc, g.dzc))) return rc;
    if ((rc = up(&c->d_rdzc, g.rdzc))) return rc;
    if ((rc = up(&c->d_rdzf, g.rdzf))) return rc;
    if ((rc = up(&c->d_psiz, g.psiz))) return rc;
    {   // per-level records for the lane = level kernels
        std::vector<NF> lvl((size_t)c->Nz * 8, NF(0));
        for (int k = 0; k < c->Nz; ++k) {
            NF* q = &lvl[(size_t)k * 8];
            q[0] = g.zC[k]; q[1] = g.psiz[k]; q[2] = g.zF[k]; q[3] = g.dzc[k]; q[4] = g.rdzc[k]; q[5] = g.rdzf[k]; q[6] = g.rdzf[k + 1];
        }
        if ((rc = up(&c->d_lvl, lvl))) return rc;
    }
    c->h_zF.assign(g.zF.begin(), g.zF.end());
    c->h_zC.assign(g.zC.begin(), g.zC.end());
    c->h_dzc.assign(g.dzc.begin(), g.dzc.end());
    c->h_dzf.assign(g.dzf.begin(), g.dzf.end());
    c->dzf_bot = g.dzf_bot;
    c->dzf_top = g.dzf_top;
    c->dzc_bot = g.dzc[0];
    c->dzc_top = g.dzc[c->Nz - 1];
    return TRM_OK;
}

template <class NF> int fill_row(trm_ctx* c, int field, double value) {
    std::vector<NF> h((size_t)c->Nh, (NF)value);
    TRM_HIP(c, hipMemcpyAsync(c->state.f[field], h.data(), h.size() * sizeof(NF), hipMemcpyHostToDevice, c->stream));
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    return TRM_OK;
}

}  // namespace

namespace trmh {
int fill_input_row(trm_ctx* c, int field, double value) {
    return by_precision(c->precision, [&](auto nf) { return fill_row<typename decltype(nf)::type>(c, field, value); });
}
}  // namespace trmh

// ======================================================================================================
// C ABI
// ======================================================================================================
extern "C" {

int trm_abi_version(void) { return TRM_ABI_VERSION; }

int trm_default_params(trm_params* p) {
    if (!p) return TRM_EINVAL;
    std::memset(p, 0, sizeof(*p));
    p->rho_w = 1000.0; p->rho_i = 916.2; p->rho_a = 1.293; p->c_a = 1005.7; p->Lsl = 3.34e5; p->Llg = 2.257e6;
    p->Lsg = 2.834e6; p->g = 9.80665; p->Tref = 273.15; p->sigma = 5.6704e-8; p->kappa_vk = 0.4; p->eps_mw = 0.622;
    p->R_a = 287.058;
    p->k_water = 0.57; p->k_ice = 2.2; p->k_air = 0.025; p->k_mineral = 3.8; p->k_organic = 0.25;
    p->c_water = 4.2e6; p->c_ice = 1.9e6; p->c_air = 0.00125e6; p->c_mineral = 2.0e6; p->c_organic = 2.5e6;
    p->por_mineral = 0.49; p->por_organic = 0.9; p->rho_soc = 0.0; p->rho_org = 1300.0;
    p->K_sat = 1.0e-5; p->theta_res = 0.0; p->bc_psi_s = 0.01; p->bc_lambda = 0.2; p->vg_alpha = 1.0; p->vg_n = 2.0;
    p->impedance = 7.0; p->vwc_forcing = 0.0;
    p->albedo = 0.3; p->emissivity = 0.97; p->kappa_s = 2.0; p->C_h = 1.2e-3; p->min_windspeed = 0.01; p->tau_r = 3600.0;
    p->beta_evap = 1.0;
    p->field_capacity = 0.25;
    p->flow = TRM_FLOW_NOFLOW; p->swrc = TRM_SWRC_BROOKS_COREY; p->unsat_k = TRM_UNSATK_LINEAR; p->seb = 0;
    p->halo_policy = TRM_HALO_REFERENCE_ZERO;
    return TRM_OK;
}

const char* trm_last_error(const trm_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int trm_create(const trm_grid* g, const trm_params* p, trm_ctx** out) {
    if (!g || !p || !out) return fail(nullptr, TRM_EINVAL, "trm_create: null argument");
    if (g->precision != TRM_F64 && g->precision != TRM_F32) return fail(nullptr, TRM_EINVAL, "trm_create: precision");
    if (g->num_layers < 2) return fail(nullptr, TRM_EINVAL, "trm_create: num_layers must be >= 2");
    if (g->num_columns < 1 || !g->thickness) return fail(nullptr, TRM_EINVAL, "trm_create: num_columns / thickness");
    for (int k = 0; k < g->num_layers; ++k)
        if (!(g->thickness[k] > 0)) return fail(nullptr, TRM_EINVAL, "trm_create: layer thickness must be positive");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(nullptr, TRM_EHIP, "trm_create: no HIP device available (this library has no CPU fallback)");
    if (g->device < 0 || g->device >= ndev) return fail(nullptr, TRM_EINVAL, "trm_create: device ordinal out of range");
    {
        long nzp = g->num_layers <= 32 ? 32 : (g->num_layers <= 64 ? 64 : ((g->num_layers + 31) / 32) * 32);
        const double esz = by_precision(g->precision, [](auto nf) { return (double)sizeof(typename decltype(nf)::type); });
        if ((double)g->num_columns * (double)nzp * esz >= 4294967296.0)
            return fail(nullptr, TRM_EINVAL, "trm_create: one field (num_columns * level pitch * word size) must stay below 4 GiB per "
                                             "device (32-bit byte offsets in the step kernel); shard the columns over more contexts");
    }
    if (!env_switches().error.empty()) return fail(nullptr, TRM_EINVAL, "trm_create: " + env_switches().error);
    trm_ctx* c = new trm_ctx();
    c->precision = g->precision;
    c->esize = by_precision(g->precision, [](auto nf) { return (int)sizeof(typename decltype(nf)::type); });
    c->Nh = (long)g->num_columns;
    c->Nz = g->num_layers;
    c->Nzp = c->Nz <= 32 ? 32 : (c->Nz <= 64 ? 64 : ((c->Nz + 31) / 32) * 32);
    c->device = g->device;
    c->params = *p;
    c->Az = g->dx > 0 ? g->dx : 1.0 / (double)c->Nh;
    if (c->precision == TRM_F32) c->Az = (double)(float)c->Az;
    // pipeline parts: two blocks of columns, the seam on a multiple of 64 (whole workgroups of every step kernel)
    c->part_n[0] = std::min<long>(c->Nh, ((c->Nh / 2 + 63) / 64) * 64);
    c->part_lo[1] = c->part_n[0];
    c->part_n[1] = c->Nh - c->part_n[0];
    auto bail = [&](int rc) {
        g_create_error = c->err;
        trm_destroy(c);
        return rc;
    };
    int rc = TRM_OK;
    auto hip = [&](hipError_t e, const char* what) {
        if (e != hipSuccess && rc == TRM_OK) { c->err = std::string(what) + ": " + hipGetErrorString(e); rc = TRM_EHIP; }
    };
    hip(hipSetDevice(c->device), "hipSetDevice");
    hip(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking), "hipStreamCreate");
    c->stream = c->own_stream;
    hip(hipEventCreate(&c->ev0), "hipEventCreate");
    hip(hipEventCreate(&c->ev1), "hipEventCreate");
    hip(hipMalloc((void**)&c->d_status, sizeof(uint32_t)), "hipMalloc(status)");
    hip(hipMalloc(&c->d_zero, (size_t)c->Nh * c->esize), "hipMalloc(zero)");
    if (c->params.seb) hip(hipMalloc(&c->d_top3, 3 * (size_t)c->Nh * c->esize), "hipMalloc(top cells)");
    // (tests: TRM_DERIVE_DEFAULT = 1 makes small grids take the instances with the derivation, where the staged outputs and the
    // input paths are compiled in -- the value a context starts with for TRM_OPT_DERIVE_CLOSURE_FIELDS)
    if (env_switches().derive_default >= 0) c->opt_derive = (int)env_switches().derive_default;
    if (env_switches().defer_closure >= 0) c->opt_defer_closure = (int)env_switches().defer_closure;
    if (env_switches().interior_steps >= 0) c->opt_interior = (int)env_switches().interior_steps;
    c->debug_handoff_tag_bias = (unsigned)env_switches().handoff_tag_bias;
    if (rc == TRM_OK) hip(hipMemsetAsync(c->d_zero, 0, (size_t)c->Nh * c->esize, c->stream), "hipMemset(zero)");
    if (rc) return bail(rc);
    hip(hipMemsetAsync(c->d_status, 0, sizeof(uint32_t), c->stream), "hipMemset(status)");
    hip(hipStreamSynchronize(c->stream), "hipStreamSynchronize");
    if ((rc = alloc_fields(c, c->state))) return bail(rc);
    rc = by_precision(c->precision, [&](auto nf) { return upload_grid<typename decltype(nf)::type>(c, g->thickness); });
    if (rc) return bail(rc);
    // input defaults (prescribed_atmosphere.jl:90-92,148,221-223)
    const struct { int f; double v; } defaults[] = {
        {TRM_FIELD_AIR_TEMPERATURE, 10.0}, {TRM_FIELD_AIR_PRESSURE, 101325.0}, {TRM_FIELD_WINDSPEED, 0.1},
        {TRM_FIELD_SPECIFIC_HUMIDITY, 1.0e-3}, {TRM_FIELD_RAINFALL, 0.0}, {TRM_FIELD_SURFACE_SHORTWAVE_DOWN, 300.0},
        {TRM_FIELD_SURFACE_LONGWAVE_DOWN, 50.0}};
    for (auto& d : defaults) {
        rc = fill_input_row(c, d.f, d.v);
        if (rc) return bail(rc);
    }
    *out = c;
    return TRM_OK;
}

int trm_destroy(trm_ctx* c) {
    if (!c) return TRM_OK;
    (void)hipSetDevice(c->device);
    (void)trm_comm_destroy(c);
    if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
    for (int f = 0; f < TRM_FIELD_COUNT; ++f) {
        if (c->state.f[f]) (void)hipFree(c->state.raw[f]);
        if (c->stage.f[f]) (void)hipFree(c->stage.raw[f]);
        if (c->saved.f[f]) (void)hipFree(c->saved.raw[f]);
    }
    if (c->d_gran) (void)hipFree(c->d_gran);
    if (c->state.kf_top) (void)hipFree(c->state.kf_top);
    if (c->stage.kf_top) (void)hipFree(c->stage.kf_top);
    if (c->saved.kf_top) (void)hipFree(c->saved.kf_top);
    for (int a = 0; a < TRM_BCV_COUNT; ++a)
        for (int b = 0; b < 2; ++b)
        {
            if (c->bc_value[a][b]) (void)hipFree(c->bc_value[a][b]);
            if (c->bc_value_stage[a][b]) (void)hipFree(c->bc_value_stage[a][b]);
        }
    for (auto& sr : c->series)
        if (sr.d_values) (void)hipFree(sr.d_values);
    for (void* q : {c->d_zC, c->d_zF, c->d_dzc, c->d_rdzc, c->d_rdzf, c->d_psiz, c->d_lvl, c->d_rootf, c->d_zero, c->d_top3, (void*)c->d_status, (void*)c->d_reduce, c->d_io, c->d_series_table, c->d_series_rows})
        if (q) (void)hipFree(q);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->copy_stream) { (void)hipStreamSynchronize(c->copy_stream); (void)hipStreamDestroy(c->copy_stream); }
    if (c->copy_done) (void)hipEventDestroy(c->copy_done);
    if (c->copy_order) (void)hipEventDestroy(c->copy_order);
    if (c->h_stage) (void)hipHostFree(c->h_stage);
    for (auto& st : c->row_stage) {
        if (st.pending) (void)hipEventSynchronize(st.done);
        if (st.done) (void)hipEventDestroy(st.done);
        if (st.h) (void)hipHostFree(st.h);
    }
    for (void* q : {(void*)c->d_ring_inv, (void*)c->d_ring_idx, c->d_ring})
        if (q) (void)hipFree(q);
    for (auto& a : c->averages)
        if (a.d_sum) (void)hipFree(a.d_sum);
    for (double* q : c->d_acc_partial)
        if (q) (void)hipFree(q);
    release_tangent(c);
    release_adjoint(c);

    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    if (c->args && c->args_free) c->args_free(c->args);
    delete c;
    return TRM_OK;
}

int trm_field_rows(const trm_ctx* c, int field, int64_t* rows) {
    if (!c || !rows || !valid_field(field)) return TRM_EINVAL;
    *rows = field_rows(c, field);
    return TRM_OK;
}

int trm_get_grid(const trm_ctx* c, double* z_faces, double* z_centers, double* dz_center, double* dz_face) {
    if (!c) return TRM_EINVAL;
    if (z_faces) std::memcpy(z_faces, c->h_zF.data(), sizeof(double) * (c->Nz + 1));
    if (z_centers) std::memcpy(z_centers, c->h_zC.data(), sizeof(double) * c->Nz);
    if (dz_center) std::memcpy(dz_center, c->h_dzc.data(), sizeof(double) * c->Nz);
    if (dz_face) std::memcpy(dz_face, c->h_dzf.data(), sizeof(double) * (c->Nz + 1));
    return TRM_OK;
}

// ---- reset!(state) + reset!(clock) (state_variables.jl:102-120, model_integrator.jl:96-99) -----------------------------------
int trm_reset(trm_ctx* c) {
    TRM_ENTER(c);
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    for (int f = 0; f < TRM_FIELD_COUNT; ++f) {
        // prognostic, auxiliary and tendency fields go to zero; inputs keep their values (they are re-initialised from their
        // sources), and so do the static root fractions and the user's per-cell forcing
        if (!c->state.f[f] || is_input_field(f) || f == TRM_FIELD_ROOT_FRACTION || f == TRM_FIELD_VWC_FORCING) continue;
        TRM_HIP(c, hipMemsetAsync(c->state.f[f], 0, field_elems(c, f) * c->esize, c->stream));
    }
    TRM_HIP(c, hipMemsetAsync(c->state.kf_top, 0, (size_t)c->Nh * c->esize, c->stream));
    if (c->d_top3) TRM_HIP(c, hipMemsetAsync(c->d_top3, 0, 3 * (size_t)c->Nh * c->esize, c->stream));
    TRM_HIP(c, hipMemsetAsync(c->d_status, 0, sizeof(uint32_t), c->stream));
    for (auto& a : c->averages) {   // open accumulators start over; their handles stay
        if (a.field < 0) continue;
        TRM_HIP(c, hipMemsetAsync(a.d_sum, 0, field_elems(c, a.field) * sizeof(double), c->stream));
        a.window = 0.0;
        a.steps = 0;
    }
    c->time = 0.0;
    c->iteration = 0;
    c->top_valid = false;
    c->tend_valid = true;
    c->closure_consistent = false;
    state_changed(c);
    return finish(c, TRM_OK);
}

int trm_save_state(trm_ctx* c) {
    TRM_ENTER_HEUN(c);
    {   // (allocates what is missing: everything the first time, the vegetation fields once they exist)
        int rc = alloc_fields(c, c->saved);
        if (rc) return rc;
        c->has_saved = true;
    }
    for (int f = 0; f < TRM_FIELD_COUNT; ++f)
        if (c->state.f[f] && c->saved.f[f]) TRM_HIP(c, hipMemcpyAsync(c->saved.f[f], c->state.f[f], field_elems(c, f) * c->esize, hipMemcpyDeviceToDevice, c->stream));
    TRM_HIP(c, hipMemcpyAsync(c->saved.kf_top, c->state.kf_top, (size_t)c->Nh * c->esize, hipMemcpyDeviceToDevice, c->stream));
    TRM_HIP(c, hipMemcpyAsync(&c->saved_status, c->d_status, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    c->saved_time = c->time;
    c->saved_iteration = c->iteration;
    c->saved_tend_valid = c->tend_valid;
    c->saved_closure_consistent = c->closure_consistent;
    return TRM_OK;
}
int trm_restore_state(trm_ctx* c) {
    TRM_ENTER_KEEP(c);
    c->heun_pending = false;
    if (!c->has_saved) return fail(c, TRM_EINVAL, "trm_restore_state: nothing was saved");
    c->closure_deferred = false;      // (every field is overwritten below: nothing to materialise)
    for (int f = 0; f < TRM_FIELD_COUNT; ++f)
        if (c->state.f[f] && c->saved.f[f]) TRM_HIP(c, hipMemcpyAsync(c->state.f[f], c->saved.f[f], field_elems(c, f) * c->esize, hipMemcpyDeviceToDevice, c->stream));
    TRM_HIP(c, hipMemcpyAsync(c->state.kf_top, c->saved.kf_top, (size_t)c->Nh * c->esize, hipMemcpyDeviceToDevice, c->stream));
    TRM_HIP(c, hipMemcpyAsync(c->d_status, &c->saved_status, sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    c->time = c->saved_time;
    c->iteration = c->saved_iteration;
    c->tend_valid = c->saved_tend_valid;
    c->closure_consistent = c->saved_closure_consistent;
    c->psi_consistent = false;      // (the restored pressure_head / water_table: whatever the saved state held)
    c->top_valid = false;
    state_changed(c);
    return finish(c, TRM_OK);
}

int trm_clock(const trm_ctx* c, double* time, int64_t* iteration) {
    if (!c) return TRM_EINVAL;
    if (time) *time = c->time;
    if (iteration) *iteration = c->iteration;
    return TRM_OK;
}
int trm_set_clock(trm_ctx* c, double time, int64_t iteration) {
    if (!c) return TRM_EINVAL;
    c->heun_pending = false;
    c->time = time;
    c->iteration = iteration;
    return TRM_OK;
}

int trm_status(trm_ctx* c, uint32_t* flags) {
    TRM_ENTER_KEEP(c);
    if (!flags) return TRM_EINVAL;
    TRM_HIP(c, hipMemcpyAsync(flags, c->d_status, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    return TRM_OK;
}

int trm_set_status(trm_ctx* c, uint32_t flags) {
    TRM_ENTER(c);
    TRM_HIP(c, hipMemcpyAsync(c->d_status, &flags, sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    TRM_HIP(c, hipStreamSynchronize(c->stream));      // (`flags` lives on this call's stack)
    return TRM_OK;
}

int trm_set_option(trm_ctx* c, int option, int value) {
    if (!c) return TRM_EINVAL;
    c->args_valid = false;
    c->heun_pending = false;
    // (an option that changes which program the next step takes: the arrays are made current here, not by whatever runs next)
    if (c->closure_deferred && option != TRM_OPT_ASYNC && option != TRM_OPT_WRITE_KF_EVERY_STEP && option != TRM_OPT_INTERIOR_STEPS && option != TRM_OPT_DERIVATIVE_SERIES &&
        option != TRM_OPT_DERIVATIVE_SERIES_PARAMS && option != TRM_OPT_DERIVATIVE_RICHARDS && option != TRM_OPT_DERIVATIVE_RICHARDS_ADJOINT &&
        !(option == TRM_OPT_DEFER_CLOSURE_STORES && value != 0)) {
        TRM_HIP(c, hipSetDevice(c->device));
        if (int rf = flush_closure(c)) return rf;
    }
    switch (option) {
        case TRM_OPT_ASYNC: c->opt_async = value != 0; return TRM_OK;
        case TRM_OPT_STEP_KERNEL:
            if (value != TRM_KERNEL_FUSED && value != TRM_KERNEL_UNFUSED) break;
            c->opt_kernel = value;
            return TRM_OK;
        case TRM_OPT_WRITE_KF_EVERY_STEP: c->opt_write_kf = value != 0; return TRM_OK;
        case TRM_OPT_VWC_FORCING_FIELD: c->opt_vwc_field = value != 0; return TRM_OK;
        case TRM_OPT_PACKED_F32: c->opt_packed = value != 0; return TRM_OK;
        case TRM_OPT_DERIVE_CLOSURE_FIELDS:
            if (value < 0 || value > 5) break;
            c->opt_derive = value;
            return TRM_OK;
        case TRM_OPT_STEPS_PER_LAUNCH:
            if (value < 0 || value > 100000) break;
            c->opt_steps_per_launch = value;
            return TRM_OK;
        case TRM_OPT_PIPELINE_PARTS:
            if (value < 0 || value > 2) break;
            c->opt_pipeline = value;
            return TRM_OK;
        case TRM_OPT_SINGLE_STEP_PROGRAM:
            if (value < 0 || value > 2) break;
            c->opt_single_step = value;
            return TRM_OK;
        case TRM_OPT_BC_SIGNATURE: c->opt_bc_signature = value != 0; return TRM_OK;
        case TRM_OPT_ZERO_GRADIENT_FAST: c->opt_zero_gradient_fast = value != 0; c->args_valid = false; return TRM_OK;
        case TRM_OPT_SURFACE_IN_LAUNCH:
            if (value < 0 || value > 2) break;
            c->opt_front = value;
            return TRM_OK;
        case TRM_OPT_DEFER_CLOSURE_STORES: c->opt_defer_closure = value != 0; return TRM_OK;
        case TRM_OPT_INTERIOR_STEPS:
            if (value < 0 || value > 2) break;
            c->opt_interior = value;
            return TRM_OK;
        case TRM_OPT_DERIVATIVE_SERIES: c->opt_derivative_series = value != 0; return TRM_OK;
        case TRM_OPT_DERIVATIVE_SERIES_PARAMS: c->opt_derivative_series_params = value != 0; return TRM_OK;
        case TRM_OPT_DERIVATIVE_RICHARDS: c->opt_derivative_richards = value != 0; return TRM_OK;
        case TRM_OPT_DERIVATIVE_RICHARDS_ADJOINT: c->opt_derivative_richards_adjoint = value != 0; return TRM_OK;
        case TRM_OPT_DERIVATIVE_RICHARDS_PARAMS: c->opt_derivative_richards_params = value != 0; return TRM_OK;
        case TRM_OPT_DERIVATIVE_RICHARDS_RECORD: c->opt_derivative_richards_record = value != 0; return TRM_OK;
        default: break;
    }
    return fail(c, TRM_EINVAL, "trm_set_option: unknown option or value");
}
int trm_get_option(const trm_ctx* c, int option, int* value) {
    if (!c || !value) return TRM_EINVAL;
    switch (option) {
        case TRM_OPT_ASYNC: *value = c->opt_async; return TRM_OK;
        case TRM_OPT_STEP_KERNEL: *value = c->opt_kernel; return TRM_OK;
        case TRM_OPT_WRITE_KF_EVERY_STEP: *value = c->opt_write_kf; return TRM_OK;
        case TRM_OPT_VWC_FORCING_FIELD: *value = c->opt_vwc_field; return TRM_OK;
        case TRM_OPT_PACKED_F32: *value = c->opt_packed; return TRM_OK;
        case TRM_OPT_DERIVE_CLOSURE_FIELDS: *value = c->opt_derive; return TRM_OK;
        case TRM_OPT_STEPS_PER_LAUNCH: *value = c->opt_steps_per_launch; return TRM_OK;
        case TRM_OPT_PIPELINE_PARTS: *value = c->opt_pipeline; return TRM_OK;
        case TRM_OPT_SINGLE_STEP_PROGRAM: *value = c->opt_single_step; return TRM_OK;
        case TRM_OPT_BC_SIGNATURE: *value = c->opt_bc_signature; return TRM_OK;
        case TRM_OPT_ZERO_GRADIENT_FAST: *value = c->opt_zero_gradient_fast; return TRM_OK;
        case TRM_OPT_SURFACE_IN_LAUNCH: *value = c->opt_front; return TRM_OK;
        case TRM_OPT_DEFER_CLOSURE_STORES: *value = c->opt_defer_closure; return TRM_OK;
        case TRM_INFO_CLOSURE_STORED: *value = c->closure_deferred ? 0 : 1; return TRM_OK;
        case TRM_INFO_MATERIALIZATIONS: *value = (int)c->materializations; return TRM_OK;
        case TRM_OPT_INTERIOR_STEPS: *value = c->opt_interior; return TRM_OK;
        case TRM_INFO_INTERIOR_LAUNCHES: *value = (int)c->interior_launches; return TRM_OK;
        case TRM_OPT_DERIVATIVE_SERIES: *value = c->opt_derivative_series; return TRM_OK;
        case TRM_OPT_DERIVATIVE_SERIES_PARAMS: *value = c->opt_derivative_series_params; return TRM_OK;
        case TRM_OPT_DERIVATIVE_RICHARDS: *value = c->opt_derivative_richards; return TRM_OK;
        case TRM_OPT_DERIVATIVE_RICHARDS_ADJOINT: *value = c->opt_derivative_richards_adjoint; return TRM_OK;
        case TRM_OPT_DERIVATIVE_RICHARDS_PARAMS: *value = c->opt_derivative_richards_params; return TRM_OK;
        case TRM_OPT_DERIVATIVE_RICHARDS_RECORD: *value = c->opt_derivative_richards_record; return TRM_OK;
        case TRM_INFO_DERIVATIVE_SERIES: *value = c->derivative_series; return TRM_OK;
        case TRM_INFO_LAST_PROGRAM: *value = c->last_program; return TRM_OK;
        case TRM_INFO_GENERIC_BOUNDARY_KERNELS: *value = by_precision(c->precision, [&](auto nf) { return trmh::Policy<typename decltype(nf)::type>::generic_bcs(c); }) ? 1 : 0; return TRM_OK;
        case TRM_INFO_BC_SIGNATURE: *value = trmh::bc_signature_of(c); return TRM_OK;
        case TRM_INFO_TOP_ARRAYS_CURRENT: *value = c->top_valid ? 1 : 0; return TRM_OK;
        case TRM_INFO_CLOSURE_CONSISTENT: *value = (c->closure_consistent && !c->closure_escaped) ? 1 : 0; return TRM_OK;
        default: return TRM_EINVAL;
    }
}

int trm_set_stream(trm_ctx* c, void* hip_stream) {
    TRM_ENTER(c);
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    return TRM_OK;
}
int trm_synchronize(trm_ctx* c) {
    TRM_ENTER_KEEP(c);
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    return TRM_OK;
}

}  // extern "C"
