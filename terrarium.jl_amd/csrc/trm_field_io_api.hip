// trm_field_io_api.hip -- field data in and out of a context: uploads, downloads, rows, device pointers, the constant boundary values and
// forcings, the full ring grid, the per-device reductions.  The only trm_*_api.hip file with kernels of its own: the small data-movement
// kernels (transposition, row staging, ring scatter / gather, reductions) and their launch code.  trm_set_bc sits here, not with the series
// it may replace: it uploads per-column values like trm_set_forcing.  Defines upload_3d / download_3d and upload_field (trm_host.hpp).
#include "trm_host.hpp"
#include "trm_reduce_fold.hpp"

using namespace trm;
using namespace trmh;

namespace {

// ---- reductions ------------------------------------------------------------------------------------
// minimum / maximum as Julia's Base.minimum / maximum (nan_min / nan_max, trm_reduce_fold.hpp): a NaN anywhere gives NaN, the
// minimum of zeros of both signs is -0, their maximum +0
// element (row r, column i) of a field sits at base[r] + i * stride[r]
template <class NF, int OP> __global__ void k_reduce_rows(const NF* f3, const NF* ftop, long Nh, int Nzp, int Nz, int is3d,
                                                          const NF* weight, double* partial) {
    const int row = blockIdx.y;
    const NF* base = is3d ? ((row == Nz && ftop) ? ftop : f3 + row) : f3;
    const long stride = (is3d && !(row == Nz && ftop)) ? Nzp : 1;
    double acc = (OP == TRM_REDUCE_MIN) ? HUGE_VAL : (OP == TRM_REDUCE_MAX ? -HUGE_VAL : 0.0);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < Nh; i += (long)gridDim.x * blockDim.x) {
        double x = (double)base[i * stride];
        if (OP == TRM_REDUCE_SUM) acc += x;
        else if (OP == TRM_REDUCE_VOLUME_INTEGRAL_Z) acc += x * (double)weight[row];
        else if (OP == TRM_REDUCE_MIN) acc = nan_min(acc, x);
        else if (OP == TRM_REDUCE_MAX) acc = nan_max(acc, x);
        else acc += (x != x) ? 1.0 : 0.0;
    }
    __shared__ double sm[4];
    for (int off = 32; off > 0; off >>= 1) {
        double o = __shfl_down(acc, off, 64);
        if (OP == TRM_REDUCE_MIN) acc = nan_min(acc, o);
        else if (OP == TRM_REDUCE_MAX) acc = nan_max(acc, o);
        else acc += o;
    }
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = sm[0];
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) {
            if (OP == TRM_REDUCE_MIN) r = nan_min(r, sm[w]);
            else if (OP == TRM_REDUCE_MAX) r = nan_max(r, sm[w]);
            else r += sm[w];
        }
        partial[(long)row * gridDim.x + blockIdx.x] = r;
    }
}

template <class NF> int reduce_impl(trm_ctx* c, int field, int op, double* out) {
    const long rows = field_rows(c, field);
    const int nblocks = (int)std::min<long>(256, (c->Nh + 255) / 256);
    size_t need = (size_t)rows * nblocks;
    if (need > c->reduce_cap) {
        if (c->d_reduce) TRM_HIP(c, hipFree(c->d_reduce));
        TRM_HIP(c, hipMalloc((void**)&c->d_reduce, need * sizeof(double)));
        c->reduce_cap = need;
    }
    const NF* f = (const NF*)c->state.f[field];
    const NF* ftop = field == TRM_FIELD_HYDRAULIC_CONDUCTIVITY ? (const NF*)c->state.kf_top : nullptr;
    const NF* w = (const NF*)c->d_dzc;
    const int d3 = is_3d(field) ? 1 : 0;
    dim3 grid(nblocks, (unsigned)rows);
#define TRM_REDUCE_LAUNCH(OP) hipLaunchKernelGGL((k_reduce_rows<NF, OP>), grid, dim3(256), 0, c->stream, f, ftop, c->Nh, c->Nzp, c->Nz, d3, w, c->d_reduce)
    switch (op) {
        case TRM_REDUCE_SUM: TRM_REDUCE_LAUNCH(TRM_REDUCE_SUM); break;
        case TRM_REDUCE_MIN: TRM_REDUCE_LAUNCH(TRM_REDUCE_MIN); break;
        case TRM_REDUCE_MAX: TRM_REDUCE_LAUNCH(TRM_REDUCE_MAX); break;
        case TRM_REDUCE_HASNAN: TRM_REDUCE_LAUNCH(TRM_REDUCE_HASNAN); break;
        case TRM_REDUCE_VOLUME_INTEGRAL_Z:
            // (rows alone does not tell: a grid of one layer would give every 2-D field Nz rows)
            if (!(is_3d(field) && rows == c->Nz)) return fail(c, TRM_EINVAL, "VOLUME_INTEGRAL_Z needs a cell-centred 3-D field");
            TRM_REDUCE_LAUNCH(TRM_REDUCE_VOLUME_INTEGRAL_Z);
            break;
        default: return fail(c, TRM_EINVAL, "unknown reduction op");
    }
#undef TRM_REDUCE_LAUNCH
    TRM_HIP(c, hipGetLastError());
    std::vector<double> part(need);
    TRM_HIP(c, hipMemcpyAsync(part.data(), c->d_reduce, need * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    // fixed-order fold of the block partials: deterministic for a given shard size
    double total = 0.0;
    for (long r = 0; r < rows; ++r) {
        double acc = (op == TRM_REDUCE_MIN) ? HUGE_VAL : (op == TRM_REDUCE_MAX ? -HUGE_VAL : 0.0);
        for (int b = 0; b < nblocks; ++b) {
            double x = part[(size_t)r * nblocks + b];
            if (op == TRM_REDUCE_MIN) acc = nan_min(acc, x);
            else if (op == TRM_REDUCE_MAX) acc = nan_max(acc, x);
            else acc += x;
        }
        if (op == TRM_REDUCE_VOLUME_INTEGRAL_Z) total += acc;
        else if (op == TRM_REDUCE_HASNAN) out[r] = acc > 0.0 ? 1.0 : 0.0;
        else out[r] = acc;
    }
    if (op == TRM_REDUCE_VOLUME_INTEGRAL_Z) out[0] = total;
    return TRM_OK;
}

// Host arrays are the reference's interior layout [rows][Nh] (column fastest); the device keeps 3-D fields
// z-fastest [Nh][Nzp].  The transposition runs on the device (32 x 32 tiles through LDS, both sides coalesced): the host
// array crosses PCIe once, as it is, through a staging buffer the context keeps.
template <class NF, bool TO_DEVICE_LAYOUT>
__global__ void __launch_bounds__(256) k_transpose(const NF* __restrict__ src, NF* __restrict__ dst, long Nh, int Nz, int Nzp) {
    __shared__ NF tile[32][33];
    const long i0 = (long)blockIdx.x * 32;
    const int k0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    if (TO_DEVICE_LAYOUT) {   // src [Nz][Nh] -> dst [Nh][Nzp]; levels Nz..Nzp-1 are padding (0)
        for (int r = ty; r < 32; r += 8) {
            const int k = k0 + r;
            const long i = i0 + tx;
            tile[r][tx] = (k < Nz && i < Nh) ? src[(size_t)k * Nh + i] : NF(0);
        }
        __syncthreads();
        for (int r = ty; r < 32; r += 8) {
            const long i = i0 + r;
            const int k = k0 + tx;
            if (i < Nh && k < Nzp) dst[(size_t)i * Nzp + k] = tile[tx][r];
        }
    } else {                  // src [Nh][Nzp] -> dst [Nz][Nh]
        for (int r = ty; r < 32; r += 8) {
            const long i = i0 + r;
            const int k = k0 + tx;
            tile[r][tx] = (i < Nh && k < Nzp) ? src[(size_t)i * Nzp + k] : NF(0);
        }
        __syncthreads();
        for (int r = ty; r < 32; r += 8) {
            const int k = k0 + r;
            const long i = i0 + tx;
            if (k < Nz && i < Nh) dst[(size_t)k * Nh + i] = tile[tx][r];
        }
    }
}

// Rows [row0, row0 + nrows) of a 3-D field in the host layout [nrows][Nh] (32 x 32 tiles through LDS, as k_transpose): the
// output path of a snapshot writer that wants `ground_temperature` -- one row -- does not move the whole field.
template <class NF>
__global__ void __launch_bounds__(256) k_rows_to_host_layout(const NF* __restrict__ src, NF* __restrict__ dst, long Nh, int Nzp, int row0, int nrows) {
    __shared__ NF tile[32][33];
    const long i0 = (long)blockIdx.x * 32;
    const int r0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) {
        const long i = i0 + r;
        const int k = row0 + r0 + tx;
        tile[r][tx] = (i < Nh && r0 + tx < nrows && k < Nzp) ? src[(size_t)i * Nzp + k] : NF(0);
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int q = r0 + r;
        const long i = i0 + tx;
        if (q < nrows && i < Nh) dst[(size_t)q * Nh + i] = tile[tx][r];
    }
}
// RingGrids.Field(field, grid; fill_value) (column_ring_grid.jl:102-115): rows [nrows][Nh] of the columns -> [nrows][P] on the
// full ring grid, `fill` outside the mask.  One thread per grid point: coalesced writes, reads in column order.
template <class NF> __global__ void k_scatter_ring(const NF* __restrict__ rows, NF* __restrict__ out, const int32_t* __restrict__ inv, long P, long Nh, NF fill) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const int32_t col = inv[p];
    const size_t r = blockIdx.y;
    out[r * (size_t)P + p] = col >= 0 ? rows[r * (size_t)Nh + col] : fill;
}
// Oceananigans.Field(ring_field, grid) (column_ring_grid.jl:117-149): the masked points of [nrows][P] in ring order
template <class NF> __global__ void k_gather_ring(const NF* __restrict__ full, NF* __restrict__ rows, const int32_t* __restrict__ idx, long P, long Nh) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Nh) return;
    const size_t r = blockIdx.y;
    rows[r * (size_t)Nh + i] = full[r * (size_t)P + idx[i]];
}
}  // namespace

namespace trmh {
// Host data [Nz][Nh] to / from a 3-D device buffer [Nh][Nzp] through d_io, synchronised.  `top`: the [Nh] buffer of a Face field's top
// face, which travels as row Nz of the host array (null: Nz rows).
template <class NF> int upload_3d(trm_ctx* c, const NF* host, NF* dev, NF* top) {
    const long Nh = c->Nh;
    const size_t bytes = (size_t)(c->Nz + (top ? 1 : 0)) * Nh * sizeof(NF);
    if (int rc = io_buffer(c, bytes)) return rc;
    TRM_HIP(c, hipMemcpyAsync(c->d_io, host, bytes, hipMemcpyHostToDevice, c->stream));
    dim3 grid((unsigned)((Nh + 31) / 32), (unsigned)((c->Nzp + 31) / 32));
    hipLaunchKernelGGL((k_transpose<NF, true>), grid, dim3(256), 0, c->stream, (const NF*)c->d_io, dev, Nh, c->Nz, c->Nzp);
    TRM_HIP(c, hipGetLastError());
    if (top) TRM_HIP(c, hipMemcpyAsync(top, (const NF*)c->d_io + (size_t)c->Nz * Nh, (size_t)Nh * sizeof(NF), hipMemcpyDeviceToDevice, c->stream));
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    return TRM_OK;
}
template <class NF> int download_3d(trm_ctx* c, const NF* dev, NF* host, const NF* top) {
    const long Nh = c->Nh;
    const size_t bytes = (size_t)(c->Nz + (top ? 1 : 0)) * Nh * sizeof(NF);
    if (int rc = io_buffer(c, bytes)) return rc;
    dim3 grid((unsigned)((Nh + 31) / 32), (unsigned)((c->Nzp + 31) / 32));
    hipLaunchKernelGGL((k_transpose<NF, false>), grid, dim3(256), 0, c->stream, dev, (NF*)c->d_io, Nh, c->Nz, c->Nzp);
    TRM_HIP(c, hipGetLastError());
    if (top) TRM_HIP(c, hipMemcpyAsync((NF*)c->d_io + (size_t)c->Nz * Nh, top, (size_t)Nh * sizeof(NF), hipMemcpyDeviceToDevice, c->stream));
    TRM_HIP(c, hipMemcpyAsync(host, c->d_io, bytes, hipMemcpyDeviceToHost, c->stream));
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    return TRM_OK;
}
template int upload_3d<double>(trm_ctx*, const double*, double*, double*);
template int upload_3d<float>(trm_ctx*, const float*, float*, float*);
template int download_3d<double>(trm_ctx*, const double*, double*, const double*);
template int download_3d<float>(trm_ctx*, const float*, float*, const float*);
}  // namespace trmh

namespace {

template <class NF> int upload_impl(trm_ctx* c, int field, const NF* host) {
    if (is_3d(field))   // (Face field: the top face lives in its own [Nh] buffer)
        return upload_3d<NF>(c, host, (NF*)c->state.f[field], field_rows(c, field) == c->Nz + 1 ? (NF*)c->state.kf_top : nullptr);
    TRM_HIP(c, hipMemcpyAsync(c->state.f[field], host, (size_t)c->Nh * sizeof(NF), hipMemcpyHostToDevice, c->stream));
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    return TRM_OK;
}
template <class NF> int download_impl(trm_ctx* c, int field, NF* host) {
    if (is_3d(field))
        return download_3d<NF>(c, (const NF*)c->state.f[field], host, field_rows(c, field) == c->Nz + 1 ? (const NF*)c->state.kf_top : nullptr);
    TRM_HIP(c, hipMemcpyAsync(host, c->state.f[field], (size_t)c->Nh * sizeof(NF), hipMemcpyDeviceToHost, c->stream));
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    return TRM_OK;
}

// rows [row0, row0 + nrows) of a field into the staging buffer d_io as [nrows][Nh] (on the context stream, not synchronised)
template <class NF> int stage_rows(trm_ctx* c, int field, int row0, int nrows) {
    const long Nh = c->Nh;
    int rc = io_buffer(c, (size_t)nrows * Nh * sizeof(NF));
    if (rc) return rc;
    NF* io = (NF*)c->d_io;
    if (!is_3d(field)) {
        TRM_HIP(c, hipMemcpyAsync(io, c->state.f[field], (size_t)Nh * sizeof(NF), hipMemcpyDeviceToDevice, c->stream));
        return TRM_OK;
    }
    const int cell_rows = std::min(nrows, c->Nz - row0);     // (the Face field's top face lives in its own [Nh] buffer)
    if (cell_rows > 0) {
        dim3 grid((unsigned)((Nh + 31) / 32), (unsigned)((cell_rows + 31) / 32));
        hipLaunchKernelGGL((k_rows_to_host_layout<NF>), grid, dim3(256), 0, c->stream, (const NF*)c->state.f[field], io, Nh, c->Nzp, row0, cell_rows);
        TRM_HIP(c, hipGetLastError());
    }
    if (row0 + nrows == c->Nz + 1)
        TRM_HIP(c, hipMemcpyAsync(io + (size_t)(c->Nz - row0) * Nh, c->state.kf_top, (size_t)Nh * sizeof(NF), hipMemcpyDeviceToDevice, c->stream));
    return TRM_OK;
}
int ring_buffer(trm_ctx* c, size_t bytes) {
    if (bytes > c->ring_cap) {
        if (c->d_ring) TRM_HIP(c, hipFree(c->d_ring));
        c->d_ring = nullptr;
        c->ring_cap = 0;
        TRM_HIP(c, hipMalloc(&c->d_ring, bytes));
        c->ring_cap = bytes;
    }
    return TRM_OK;
}
template <class NF> int scatter_ring_impl(trm_ctx* c, int field, int row0, int nrows, double fill, void* out, bool out_is_device) {
    int rc = stage_rows<NF>(c, field, row0, nrows);
    if (rc) return rc;
    NF* dst = (NF*)out;
    if (!out_is_device) {
        if ((rc = ring_buffer(c, (size_t)nrows * c->ring_points * sizeof(NF)))) return rc;
        dst = (NF*)c->d_ring;
    }
    dim3 grid((unsigned)((c->ring_points + 255) / 256), (unsigned)nrows);
    hipLaunchKernelGGL((k_scatter_ring<NF>), grid, dim3(256), 0, c->stream, (const NF*)c->d_io, dst, c->d_ring_inv, c->ring_points, c->Nh, (NF)fill);
    TRM_HIP(c, hipGetLastError());
    if (!out_is_device) TRM_HIP(c, hipMemcpyAsync(out, dst, (size_t)nrows * c->ring_points * sizeof(NF), hipMemcpyDeviceToHost, c->stream));
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    return TRM_OK;
}
// full-grid host (or device) array [rows][P] -> the field: gather on the device, then the usual layout change
template <class NF> int gather_ring_impl(trm_ctx* c, int field, const void* full, bool full_is_device) {
    const long Nh = c->Nh, rows = field_rows(c, field), P = c->ring_points;
    const NF* src = (const NF*)full;
    int rc;
    if (!full_is_device) {
        if ((rc = ring_buffer(c, (size_t)rows * P * sizeof(NF)))) return rc;
        TRM_HIP(c, hipMemcpyAsync(c->d_ring, full, (size_t)rows * P * sizeof(NF), hipMemcpyHostToDevice, c->stream));
        src = (const NF*)c->d_ring;
    }
    if ((rc = io_buffer(c, (size_t)rows * Nh * sizeof(NF)))) return rc;
    NF* io = (NF*)c->d_io;
    dim3 grid((unsigned)((Nh + 255) / 256), (unsigned)rows);
    hipLaunchKernelGGL((k_gather_ring<NF>), grid, dim3(256), 0, c->stream, src, is_3d(field) ? io : (NF*)c->state.f[field], c->d_ring_idx, P, Nh);
    TRM_HIP(c, hipGetLastError());
    if (is_3d(field)) {
        dim3 tg((unsigned)((Nh + 31) / 32), (unsigned)((c->Nzp + 31) / 32));
        hipLaunchKernelGGL((k_transpose<NF, true>), tg, dim3(256), 0, c->stream, (const NF*)io, (NF*)c->state.f[field], Nh, c->Nz, c->Nzp);
        TRM_HIP(c, hipGetLastError());
        if (rows == c->Nz + 1)
            TRM_HIP(c, hipMemcpyAsync(c->state.kf_top, io + (size_t)c->Nz * Nh, (size_t)Nh * sizeof(NF), hipMemcpyDeviceToDevice, c->stream));
    }
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    return TRM_OK;
}

}  // namespace

namespace trmh {
int upload_field(trm_ctx* c, int field, const void* host) {
    return by_precision(c->precision, [&](auto nf) { using NF = typename decltype(nf)::type; return upload_impl<NF>(c, field, (const NF*)host); });
}
}  // namespace trmh

extern "C" {

int trm_upload(trm_ctx* c, int field, const void* host) {
    if (!c || !host || !valid_field(field)) return fail(c, TRM_EINVAL, "trm_upload: bad argument");
    if (!c->state.f[field]) return fail(c, TRM_EINVAL, "trm_upload: the field exists only after trm_set_vegetation");
    if (field == TRM_FIELD_ROOT_FRACTION)
        return fail(c, TRM_EINVAL, "trm_upload: root_fraction is a static function of the root distribution parameters "
                                   "(root_distribution.jl:45-63): set them with trm_set_vegetation");
    TRM_HIP(c, hipSetDevice(c->device));
    c->heun_pending = false;
    if (int rf = flush_closure(c)) return rf;      // (an upload of T alone must find liq current, and the reverse)
    int rc = upload_field(c, field, host);
    if (field <= TRM_FIELD_PRESSURE_HEAD || field == TRM_FIELD_WATER_TABLE) c->closure_consistent = false;   // (U, sat, T, liq, psi, water table)
    if (field == TRM_FIELD_INTERNAL_ENERGY || field == TRM_FIELD_SATURATION_WATER_ICE) state_changed(c);
    if (!rc && field == TRM_FIELD_VWC_FORCING) {
        c->opt_vwc_field = 1;
        c->args_valid = false;
    }
    c->top_valid = false;
    if (!rc && (field == TRM_FIELD_TEND_INTERNAL_ENERGY || field == TRM_FIELD_TEND_SATURATION_WATER_ICE || field == TRM_FIELD_TEND_SURFACE_EXCESS_WATER))
        c->tend_valid = true;   // (a caller that sets one tendency field owns all of them)
    return rc;
}

static bool is_tendency(int f) {
    return f == TRM_FIELD_TEND_INTERNAL_ENERGY || f == TRM_FIELD_TEND_SATURATION_WATER_ICE || f == TRM_FIELD_TEND_SURFACE_EXCESS_WATER;
}
static const char* kStaleTendencies =
    "the tendency fields are not materialised by a fused step that does not finalize (finalize = 0): call trm_step / "
    "trm_step_heun with finalize = 1, or trm_update_state(ctx, 1), before reading them";

int trm_download(trm_ctx* c, int field, void* host) {
    if (!c || !host || !valid_field(field)) return fail(c, TRM_EINVAL, "trm_download: bad argument");
    if (is_tendency(field) && !c->tend_valid) return fail(c, TRM_ESTALE, kStaleTendencies);
    if (!c->state.f[field]) return fail(c, TRM_EINVAL, "trm_download: the field exists only after trm_set_vegetation");
    TRM_HIP(c, hipSetDevice(c->device));
    if (int rf = flush_closure(c)) return rf;
    return by_precision(c->precision, [&](auto nf) { using NF = typename decltype(nf)::type; return download_impl<NF>(c, field, (NF*)host); });
}

int trm_field_device_ptr(trm_ctx* c, int field, void** dev, int64_t* pitch_elems) {
    if (!c || !dev || !valid_field(field)) return fail(c, TRM_EINVAL, "trm_field_device_ptr: bad argument");
    if (!c->state.f[field]) return fail(c, TRM_EINVAL, "trm_field_device_ptr: the field exists only after trm_set_vegetation");
    if (is_tendency(field) && !c->tend_valid) return fail(c, TRM_ESTALE, kStaleTendencies);
    if (c->closure_deferred) {      // (the caller reads the arrays behind the library's back from now on; closure_escaped below ends deferral)
        TRM_HIP(c, hipSetDevice(c->device));
        if (int rf = flush_closure(c)) return rf;
    }
    *dev = c->state.f[field];
    if (pitch_elems) *pitch_elems = is_3d(field) ? c->Nzp : 1;
    // the caller may write the state behind the library's back from now on: stop trusting the top-cell copies
    if (field == TRM_FIELD_TEMPERATURE || field == TRM_FIELD_SATURATION_WATER_ICE || field == TRM_FIELD_LIQUID_WATER_FRACTION)
        c->top_escaped = true;
    if (field <= TRM_FIELD_PRESSURE_HEAD || field == TRM_FIELD_WATER_TABLE) c->closure_escaped = true;   // U, sat, T, liq, psi, the water table may change behind the library's back
    c->top_valid = false;
    return TRM_OK;
}

int trm_bc_device_ptr(trm_ctx* c, int var, int side, void** dev) {
    if (!c || !dev || var < 0 || var >= TRM_BCV_COUNT || (side != TRM_TOP && side != TRM_BOTTOM)) return fail(c, TRM_EINVAL, "trm_bc_device_ptr: bad argument");
    if (c->bc_kind[var][side] == TRM_BC_NOFLUX || !c->bc_value[var][side]) return fail(c, TRM_EINVAL, "trm_bc_device_ptr: the condition carries no values (set it with trm_set_bc first)");
    for (const auto& sr : c->series)
        if (sr.is_bc && sr.var == var && sr.side == side) return fail(c, TRM_EINVAL, "trm_bc_device_ptr: the boundary values are evaluated from a time series every step");
    *dev = c->bc_value[var][side];
    c->bc_zero_gradient[var][side] = false;      // (the caller may write the buffer from now on)
    return TRM_OK;
}

int trm_set_bc(trm_ctx* c, int var, int side, int kind, const void* values, double scalar) {
    if (!c || var < 0 || var >= TRM_BCV_COUNT || (side != TRM_TOP && side != TRM_BOTTOM) || kind < 0 || kind > TRM_BC_GRADIENT)
        return fail(c, TRM_EINVAL, "trm_set_bc: bad argument");
    TRM_HIP(c, hipSetDevice(c->device));
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    if (int rs = sync_copies(c)) return rs;
    // a constant replaces an earlier time series of the same boundary value (which would otherwise overwrite it at the next step)
    for (size_t n = 0; n < c->series.size(); ++n) {
        auto& o = c->series[n];
        if (o.is_bc && o.var == var && o.side == side) {
            if (o.d_values) (void)hipFree(o.d_values);
            c->series.erase(c->series.begin() + (long)n);
            break;
        }
    }
    c->bc_kind[var][side] = kind;
    c->bc_zero_gradient[var][side] = false;
    c->args_valid = false;
    c->heun_pending = false;
    bc_changed(c);
    if (kind == TRM_BC_NOFLUX) return TRM_OK;
    size_t bytes = (size_t)c->Nh * c->esize;
    if (!c->bc_value[var][side]) TRM_HIP(c, hipMalloc(&c->bc_value[var][side], bytes));
    std::vector<unsigned char> h(bytes, 0);
    if (values) {
        std::memcpy(h.data(), values, (size_t)c->Nh * c->esize);
    } else if (c->precision == TRM_F64) {
        double* d = (double*)h.data();
        for (long i = 0; i < c->Nh; ++i) d[i] = scalar;
    } else {
        float* d = (float*)h.data();
        for (long i = 0; i < c->Nh; ++i) d[i] = (float)scalar;
    }
    TRM_HIP(c, hipMemcpyAsync(c->bc_value[var][side], h.data(), bytes, hipMemcpyHostToDevice, c->stream));
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    if (kind == TRM_BC_GRADIENT) {   // every value +0 (all bits clear): see trm_ctx::bc_zero_gradient
        bool zero = true;
        for (size_t n = 0; n < bytes && zero; ++n) zero = h[n] == 0;
        c->bc_zero_gradient[var][side] = zero;
    }
    return TRM_OK;
}

int trm_set_forcing(trm_ctx* c, int input_field, const void* per_column) {
    if (!c || !is_input_field(input_field))
        return fail(c, TRM_EINVAL, "trm_set_forcing: not an input field");
    return trm_upload(c, input_field, per_column);
}

int trm_set_forcing_device(trm_ctx* c, int input_field, const void* dev_per_column) {
    TRM_ENTER(c);
    if (!is_input_field(input_field) || !dev_per_column) return fail(c, TRM_EINVAL, "trm_set_forcing_device: not an input field / null pointer");
    if (!c->state.f[input_field]) return fail(c, TRM_EINVAL, "trm_set_forcing_device: the field exists only after trm_set_vegetation");
    for (const auto& sr : c->series)
        if (!sr.is_bc && sr.field == input_field) return fail(c, TRM_EINVAL, "trm_set_forcing_device: the input is evaluated from a time series every step (trm_clear_series / trm_set_forcing first)");
    // stream-ordered: behind the steps already enqueued, in front of the next one; the host does not wait
    TRM_HIP(c, hipMemcpyAsync(c->state.f[input_field], dev_per_column, (size_t)c->Nh * c->esize, hipMemcpyDeviceToDevice, c->stream));
    return TRM_OK;
}

// ---- output: rows of a field, and the full ring grid (column_ring_grid.jl:102-149) -----------------------------------------
int trm_download_rows(trm_ctx* c, int field, int row0, int nrows, void* host) {
    TRM_ENTER_HEUN(c);
    if (!host || !valid_field(field) || !c->state.f[field]) return fail(c, TRM_EINVAL, "trm_download_rows: bad argument");
    if (row0 < 0 || nrows < 1 || row0 + nrows > field_rows(c, field)) return fail(c, TRM_EINVAL, "trm_download_rows: rows out of range");
    if (is_tendency(field) && !c->tend_valid) return fail(c, TRM_ESTALE, kStaleTendencies);
    int rc = by_precision(c->precision, [&](auto nf) { return stage_rows<typename decltype(nf)::type>(c, field, row0, nrows); });
    if (rc) return rc;
    TRM_HIP(c, hipMemcpyAsync(host, c->d_io, (size_t)nrows * c->Nh * c->esize, hipMemcpyDeviceToHost, c->stream));
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    return TRM_OK;
}

int trm_set_ring_grid(trm_ctx* c, int64_t num_points, const int64_t* mask_index) {
    TRM_ENTER_HEUN(c);
    if (num_points < c->Nh || num_points >= ((int64_t)1 << 31) || !mask_index) return fail(c, TRM_EINVAL, "trm_set_ring_grid: bad argument");
    std::vector<int32_t> inv((size_t)num_points, -1), idx((size_t)c->Nh);
    for (long i = 0; i < c->Nh; ++i) {
        const int64_t p = mask_index[i];
        if (p < 0 || p >= num_points || inv[(size_t)p] >= 0 || (i > 0 && p <= mask_index[i - 1]))
            return fail(c, TRM_EINVAL, "trm_set_ring_grid: mask_index must be strictly increasing grid point indices, one per column");
        inv[(size_t)p] = (int32_t)i;
        idx[(size_t)i] = (int32_t)p;
    }
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    for (void* q : {(void*)c->d_ring_inv, (void*)c->d_ring_idx})
        if (q) (void)hipFree(q);
    c->d_ring_inv = c->d_ring_idx = nullptr;
    TRM_HIP(c, hipMalloc((void**)&c->d_ring_inv, inv.size() * sizeof(int32_t)));
    TRM_HIP(c, hipMalloc((void**)&c->d_ring_idx, idx.size() * sizeof(int32_t)));
    TRM_HIP(c, hipMemcpyAsync(c->d_ring_inv, inv.data(), inv.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    TRM_HIP(c, hipMemcpyAsync(c->d_ring_idx, idx.data(), idx.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    c->ring_points = (long)num_points;
    return TRM_OK;
}

static int ring_args_ok(trm_ctx* c, int field, int row0, int nrows, const void* buf, const char* who) {
    if (!c->ring_points) return fail(c, TRM_EINVAL, std::string(who) + ": call trm_set_ring_grid first");
    if (!buf || !valid_field(field) || !c->state.f[field]) return fail(c, TRM_EINVAL, std::string(who) + ": bad argument");
    if (row0 < 0 || nrows < 1 || row0 + nrows > field_rows(c, field)) return fail(c, TRM_EINVAL, std::string(who) + ": rows out of range");
    if (is_tendency(field) && !c->tend_valid) return fail(c, TRM_ESTALE, kStaleTendencies);
    return TRM_OK;
}
int trm_download_ring(trm_ctx* c, int field, int row0, int nrows, double fill, void* host) {
    TRM_ENTER_HEUN(c);
    if (int rc = ring_args_ok(c, field, row0, nrows, host, "trm_download_ring")) return rc;
    return by_precision(c->precision, [&](auto nf) { return scatter_ring_impl<typename decltype(nf)::type>(c, field, row0, nrows, fill, host, false); });
}
int trm_scatter_ring_device(trm_ctx* c, int field, int row0, int nrows, double fill, void* dev_out) {
    TRM_ENTER_HEUN(c);
    if (int rc = ring_args_ok(c, field, row0, nrows, dev_out, "trm_scatter_ring_device")) return rc;
    return by_precision(c->precision, [&](auto nf) { return scatter_ring_impl<typename decltype(nf)::type>(c, field, row0, nrows, fill, dev_out, true); });
}
static int gather_ring(trm_ctx* c, int field, const void* full, bool device, const char* who) {
    if (int rc = ring_args_ok(c, field, 0, (int)field_rows(c, field), full, who)) return rc;
    if (field == TRM_FIELD_ROOT_FRACTION) return fail(c, TRM_EINVAL, std::string(who) + ": root_fraction is derived from the root distribution parameters");
    int rc = by_precision(c->precision, [&](auto nf) { return gather_ring_impl<typename decltype(nf)::type>(c, field, full, device); });
    if (field <= TRM_FIELD_PRESSURE_HEAD || field == TRM_FIELD_WATER_TABLE) c->closure_consistent = false;
    if (field == TRM_FIELD_INTERNAL_ENERGY || field == TRM_FIELD_SATURATION_WATER_ICE) state_changed(c);
    if (!rc && field == TRM_FIELD_VWC_FORCING) { c->opt_vwc_field = 1; c->args_valid = false; }
    c->top_valid = false;
    if (!rc && is_tendency(field)) c->tend_valid = true;
    return rc;
}
int trm_upload_ring(trm_ctx* c, int field, const void* host_full) {
    TRM_ENTER(c);
    return gather_ring(c, field, host_full, false, "trm_upload_ring");
}
int trm_gather_ring_device(trm_ctx* c, int field, const void* dev_full) {
    TRM_ENTER(c);
    return gather_ring(c, field, dev_full, true, "trm_gather_ring_device");
}

int trm_reduce(trm_ctx* c, int field, int op, double* out) {
    if (!c) return TRM_EINVAL;
    if (!out || !valid_field(field)) return fail(c, TRM_EINVAL, "trm_reduce: bad argument");
    // (before the device is touched: k_reduce_rows would read through the null base of a field that was never allocated)
    if (!c->state.f[field]) return fail(c, TRM_EINVAL, "trm_reduce: the field exists only after trm_set_vegetation");
    TRM_ENTER_HEUN(c);
    if (is_tendency(field) && !c->tend_valid) return fail(c, TRM_ESTALE, kStaleTendencies);
    return by_precision(c->precision, [&](auto nf) { return reduce_impl<typename decltype(nf)::type>(c, field, op, out); });
}

}  // extern "C"
