// trm_series_api.hip -- the time series of forcings and boundary values a context holds: the bookkeeping of their records, the windowed
// ring (append / window / trim), and the time indexing every evaluator of a series uses (series_time_indices: trm_launch_unfused.hip calls
// it).  Host code alone.  sync_copies sits here, not with field I/O (trm_set_bc calls it too): it waits for the copies of
// trm_series_append and resets the series' pending marks.
#include "trm_host.hpp"

using namespace trm;
using namespace trmh;

namespace trmh {
// Time interpolation indices of a series at time t -- Oceananigans' FieldTimeSeries indexing (Linear / Clamp /
// Cyclical), restated; that package is not part of the reference tree (parity unpinned).
// Returns 0-based nodes n1, n2 and the fraction f: value = v[n2] * f + v[n1] * (1 - f); n1 == n2 means "copy".
void series_time_indices(const std::vector<double>& times, int indexing, double t, int& n1, int& n2, double& f, double& g) {
    const int nt = (int)times.size();
    n1 = n2 = 0;
    f = g = 0.0;
    if (nt == 1) return;
    if (indexing == TRM_TIME_RASTER) {
        // update_from_raster! (TerrariumRastersExt.jl:96-121): searchsorted brackets t; on a node or beyond either end the
        // node's values are taken as they are (flat extrapolation), in between x1 + eps * (x2 - x1) / dt
        const int right = (int)(std::lower_bound(times.begin(), times.end(), t) - times.begin());       // first(indexes) - 1
        const int left = (int)(std::upper_bound(times.begin(), times.end(), t) - times.begin()) - 1;    // last(indexes) - 1
        if (left >= 0 && right <= nt - 1) {
            n1 = left;
            n2 = right;
            g = times[right] - times[left];
            f = t - times[left];
            if (!(g > 0)) n1 = n2 = right;   // (on a node)
        } else {
            n1 = n2 = std::min(right, nt - 1);
        }
        return;
    }
    auto find = [&](double tq) {
        // binary search for the bracketing interval; an interior node hit returns (n, n); outside the range the
        // first / last interval is returned (linear extrapolation)
        int low = 0, high = nt - 1;
        while (low + 1 < high) {
            int mid = (low + high) / 2;
            if (times[mid] == tq) { n1 = n2 = mid; f = 0.0; return; }
            if (times[mid] < tq) low = mid; else high = mid;
        }
        n1 = low;
        n2 = high;
        f = (1.0 / (times[n2] - times[n1])) * (tq - times[n1]);
    };
    if (indexing == TRM_TIME_CYCLICAL) {
        const double t1 = times[0], tN = times[nt - 1];
        const double period = (tN - t1) + (tN - times[nt - 2]);
        double tau = std::fmod(t - t1, period);
        if (tau < 0) tau += period;
        const double tm = tau + t1;
        if (tm > tN) {   // between the last node and the first node of the next cycle
            n1 = nt - 1;
            n2 = 0;
            f = (1.0 / (period - (tN - t1))) * (tm - tN);
            return;
        }
        find(tm);
        return;
    }
    find(t);
    if (indexing == TRM_TIME_CLAMP) {
        if (t >= times[nt - 1]) { n1 = n2 = nt - 1; f = 0.0; }
        else if (t <= times[0]) { n1 = n2 = 0; f = 0.0; }
    }
}
// every H2D copy of trm_series_append has finished (before a series buffer is freed or reallocated)
int sync_copies(trm_ctx* c) {
    if (c->copy_stream && c->copy_pending) TRM_HIP(c, hipStreamSynchronize(c->copy_stream));
    c->copy_pending = false;
    for (auto& o : c->series) o.pending_from = -1;
    return TRM_OK;
}
}  // namespace trmh

extern "C" {

namespace {
int add_series(trm_ctx* c, trm_ctx::Series&& sr, int nt, const double* times, const void* values, const char* who) {
    if (nt < 1 || !times || !values) return fail(c, TRM_EINVAL, std::string(who) + ": nt >= 1, times and values are required");
    for (int n = 1; n < nt; ++n)
        if (!(times[n] > times[n - 1])) return fail(c, TRM_EINVAL, std::string(who) + ": times must be strictly increasing");
    if (sr.indexing < TRM_TIME_LINEAR || sr.indexing > TRM_TIME_RASTER) return fail(c, TRM_EINVAL, std::string(who) + ": bad time_indexing");
    TRM_HIP(c, hipSetDevice(c->device));
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    if (int rs = sync_copies(c)) return rs;
    // replace an earlier series with the same target
    for (size_t n = 0; n < c->series.size(); ++n) {
        auto& o = c->series[n];
        if (o.is_bc == sr.is_bc && (sr.is_bc ? (o.var == sr.var && o.side == sr.side) : o.field == sr.field)) {
            if (o.d_values) (void)hipFree(o.d_values);
            c->series.erase(c->series.begin() + (long)n);
            break;
        }
    }
    sr.times.assign(times, times + nt);
    sr.cap = nt;
    sr.head = 0;
    size_t bytes = (size_t)nt * (size_t)c->Nh * c->esize;
    TRM_HIP(c, hipMalloc(&sr.d_values, bytes));
    TRM_HIP(c, hipMemcpyAsync(sr.d_values, values, bytes, hipMemcpyHostToDevice, c->stream));
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    c->series.push_back(std::move(sr));
    return TRM_OK;
}
}  // namespace

int trm_set_forcing_series(trm_ctx* c, int input_field, int nt, const double* times, const void* values, int time_indexing) {
    if (!c || !is_input_field(input_field))
        return fail(c, TRM_EINVAL, "trm_set_forcing_series: not an input field");
    trm_ctx::Series sr;
    sr.is_bc = false;
    sr.field = input_field;
    sr.indexing = time_indexing;
    return add_series(c, std::move(sr), nt, times, values, "trm_set_forcing_series");
}

int trm_set_bc_series(trm_ctx* c, int var, int side, int kind, int nt, const double* times, const void* values, int time_indexing) {
    if (!c || var < 0 || var >= TRM_BCV_COUNT || (side != TRM_TOP && side != TRM_BOTTOM) || kind <= TRM_BC_NOFLUX || kind > TRM_BC_GRADIENT)
        return fail(c, TRM_EINVAL, "trm_set_bc_series: bad argument");
    trm_ctx::Series sr;
    sr.is_bc = true;
    sr.var = var;
    sr.side = side;
    sr.indexing = time_indexing;
    int rc = add_series(c, std::move(sr), nt, times, values, "trm_set_bc_series");
    if (rc) return rc;
    c->bc_kind[var][side] = kind;
    c->bc_zero_gradient[var][side] = false;      // (the values come from the series from now on)
    c->args_valid = false;
    bc_changed(c);
    if (!c->bc_value[var][side]) {
        TRM_HIP(c, hipMalloc(&c->bc_value[var][side], (size_t)c->Nh * c->esize));
        TRM_HIP(c, hipMemsetAsync(c->bc_value[var][side], 0, (size_t)c->Nh * c->esize, c->stream));
        TRM_HIP(c, hipStreamSynchronize(c->stream));
    }
    return TRM_OK;
}

int trm_clear_series(trm_ctx* c) {
    if (!c) return TRM_EINVAL;
    TRM_HIP(c, hipSetDevice(c->device));
    TRM_HIP(c, hipStreamSynchronize(c->stream));
    if (int rs = sync_copies(c)) return rs;
    for (auto& sr : c->series)
        if (sr.d_values) (void)hipFree(sr.d_values);
    c->series.clear();
    bc_changed(c);
    return TRM_OK;
}

// ---- windowed time series ("device-side double-buffered forcing slabs") -------------------------------------
namespace {
trm_ctx::Series* find_series(trm_ctx* c, int is_bc, int id, int side) {
    for (auto& sr : c->series)
        if (sr.is_bc == (is_bc != 0) && (is_bc ? (sr.var == id && sr.side == side) : sr.field == id)) return &sr;
    return nullptr;
}
}  // namespace

int trm_series_append(trm_ctx* c, int is_bc, int id, int side, int nt, const double* times, const void* values) {
    TRM_ENTER(c);
    trm_ctx::Series* sr = find_series(c, is_bc, id, side);
    if (!sr) return fail(c, TRM_EINVAL, "trm_series_append: no such series (create it with trm_set_forcing_series / trm_set_bc_series first)");
    if (nt < 1 || !times || !values) return fail(c, TRM_EINVAL, "trm_series_append: nt >= 1, times and values are required");
    if (sr->indexing == TRM_TIME_CYCLICAL) return fail(c, TRM_EINVAL, "trm_series_append: a cyclical series is periodic over its whole record and cannot be windowed");
    if (!(times[0] > sr->times.back())) return fail(c, TRM_EINVAL, "trm_series_append: times must continue the series (strictly increasing)");
    for (int n = 1; n < nt; ++n)
        if (!(times[n] > times[n - 1])) return fail(c, TRM_EINVAL, "trm_series_append: times must be strictly increasing");
    const size_t row = (size_t)c->Nh * c->esize;
    const long held = (long)sr->times.size();
    if (!c->copy_stream) {
        TRM_HIP(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
        TRM_HIP(c, hipEventCreateWithFlags(&c->copy_done, hipEventDisableTiming));
    }
    if (held + nt > sr->cap) {
        // no free slots left (nothing was trimmed): the ring grows; the levels held are laid out from slot 0 again
        TRM_HIP(c, hipStreamSynchronize(c->stream));
        if (int rs = sync_copies(c)) return rs;
        const long cap = held + nt;
        void* grown = nullptr;
        TRM_HIP(c, hipMalloc(&grown, (size_t)cap * row));
        for (long n = 0; n < held; ++n)
            TRM_HIP(c, hipMemcpyAsync((char*)grown + (size_t)n * row, (char*)sr->d_values + sr->slot((int)n) * row, row, hipMemcpyDeviceToDevice, c->stream));
        TRM_HIP(c, hipStreamSynchronize(c->stream));
        TRM_HIP(c, hipFree(sr->d_values));
        sr->d_values = grown;
        sr->cap = cap;
        sr->head = 0;
    }
    // host -> pinned staging (the caller's array is borrowed for the duration of the call only) -> device, on the side stream:
    // the copy runs under whatever the context stream is executing; the next step that evaluates the series waits for it
    if (c->copy_pending) TRM_HIP(c, hipEventSynchronize(c->copy_done));   // the staging buffer is free again
    if ((size_t)nt * row > c->h_stage_cap) {
        if (c->h_stage) TRM_HIP(c, hipHostFree(c->h_stage));
        c->h_stage = nullptr;
        c->h_stage_cap = 0;
        TRM_HIP(c, hipHostMalloc(&c->h_stage, (size_t)nt * row, hipHostMallocDefault));
        c->h_stage_cap = (size_t)nt * row;
    }
    std::memcpy(c->h_stage, values, (size_t)nt * row);
    // the slots written are free ones: never used, or released by trm_series_trim_before -- whose event marks the context
    // stream's work that may still have been reading them; steps enqueued after the trim cannot see them
    if (c->order_recorded) TRM_HIP(c, hipStreamWaitEvent(c->copy_stream, c->copy_order, 0));
    for (int n = 0; n < nt; ++n)
        TRM_HIP(c, hipMemcpyAsync((char*)sr->d_values + sr->slot((int)held + n) * row, (char*)c->h_stage + (size_t)n * row, row, hipMemcpyHostToDevice, c->copy_stream));
    TRM_HIP(c, hipEventRecord(c->copy_done, c->copy_stream));
    c->copy_pending = true;
    if (sr->pending_from < 0) sr->pending_from = held;
    sr->windowed = true;
    sr->times.insert(sr->times.end(), times, times + nt);
    bc_changed(c);     // (a taped step's rows name the levels the series held when it was recorded)
    return TRM_OK;
}

int trm_series_window(trm_ctx* c, int is_bc, int id, int side, int levels) {
    TRM_ENTER(c);
    trm_ctx::Series* sr = find_series(c, is_bc, id, side);
    if (!sr) return fail(c, TRM_EINVAL, "trm_series_window: no such series (create it with trm_set_forcing_series / trm_set_bc_series first)");
    if (sr->indexing == TRM_TIME_CYCLICAL) return fail(c, TRM_EINVAL, "trm_series_window: a cyclical series is periodic over its whole record and cannot be windowed");
    if (levels < 0) return fail(c, TRM_EINVAL, "trm_series_window: levels < 0");
    sr->windowed = true;
    bc_changed(c);
    const long held = (long)sr->times.size();
    if (levels > sr->cap) {      // reserve: the levels held are laid out from slot 0 of the larger ring
        const size_t row = (size_t)c->Nh * c->esize;
        TRM_HIP(c, hipStreamSynchronize(c->stream));
        if (int rs = sync_copies(c)) return rs;
        void* grown = nullptr;
        TRM_HIP(c, hipMalloc(&grown, (size_t)levels * row));
        for (long n = 0; n < held; ++n)
            TRM_HIP(c, hipMemcpyAsync((char*)grown + (size_t)n * row, (char*)sr->d_values + sr->slot((int)n) * row, row, hipMemcpyDeviceToDevice, c->stream));
        TRM_HIP(c, hipStreamSynchronize(c->stream));
        TRM_HIP(c, hipFree(sr->d_values));
        sr->d_values = grown;
        sr->cap = levels;
        sr->head = 0;
    }
    return TRM_OK;
}

int trm_series_trim_before(trm_ctx* c, double t) {
    if (!c) return TRM_EINVAL;
    bool released = false;
    for (auto& sr : c->series) {
        // only series that stream through a window (levels have been appended): a fully resident series that merely lives in
        // the same context keeps its whole record, whatever the clock does later
        if (sr.indexing == TRM_TIME_CYCLICAL || !sr.windowed) continue;
        // keep the node at or before t (the lower bracket of every later evaluation) and at least two levels
        long drop = 0;
        while ((long)sr.times.size() - drop > 2 && sr.times[(size_t)drop + 1] <= t) ++drop;
        if (drop > 0) {
            sr.times.erase(sr.times.begin(), sr.times.begin() + drop);
            sr.head = (sr.head + drop) % sr.cap;
            if (sr.pending_from >= 0) sr.pending_from = std::max<long>(0, sr.pending_from - drop);
            sr.trimmed = true;
            sr.trimmed_before = sr.times.front();
            released = true;
        }
    }
    if (released) {
        bc_changed(c);
        if (hipSetDevice(c->device) != hipSuccess) return fail(c, TRM_EHIP, "trm_series_trim_before: hipSetDevice");
        if (!c->copy_order) TRM_HIP(c, hipEventCreateWithFlags(&c->copy_order, hipEventDisableTiming));
        TRM_HIP(c, hipEventRecord(c->copy_order, c->stream));
        c->order_recorded = true;
    }
    return TRM_OK;
}

int trm_series_info(const trm_ctx* c, int is_bc, int id, int side, int64_t* levels_held, int64_t* capacity, double* t_first, double* t_last) {
    if (!c) return TRM_EINVAL;
    const trm_ctx::Series* sr = find_series(const_cast<trm_ctx*>(c), is_bc, id, side);
    if (!sr) return TRM_EINVAL;
    if (levels_held) *levels_held = (int64_t)sr->times.size();
    if (capacity) *capacity = sr->cap;
    if (t_first) *t_first = sr->times.front();
    if (t_last) *t_last = sr->times.back();
    return TRM_OK;
}

}  // extern "C"
