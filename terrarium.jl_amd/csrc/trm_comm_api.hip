// trm_comm_api.hip -- the communicators of the C ABI: the RCCL loader (opened on first use; the only file that includes <dlfcn.h>), the
// global reductions and status of one context, and their grouped forms over n contexts driven by one host thread (trm_*_all, but the two
// that step: trm_step_api.hip).  check_ctx_list is defined here, with the other callers of a context list.  Host code alone.
#include "trm_host.hpp"
#include "trm_reduce_fold.hpp"

#include <dlfcn.h>

using namespace trm;
using namespace trmh;

namespace {

// ---- RCCL, opened on first use ------------------------------------------------------------------------
struct Rccl {
    void* handle = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    std::string error;
};
Rccl* rccl() {
    static Rccl r;
    if (r.handle || !r.error.empty()) return &r;
    // TRM_RCCL_LIBRARY (tests): the collective library to open instead -- tests/fake_rccl.c, a stand-in that implements the seven
    // entry points through host memory for n communicators in ONE process, so that the grouped call sequences below run with
    // n > 1 on a one-GPU box (with torch in the process its own librccl.so is already mapped: dlsym on OUR handle still
    // resolves to the library named here)
    if (const char* over = std::getenv("TRM_RCCL_LIBRARY")) {
        r.handle = dlopen(over, RTLD_NOW | RTLD_LOCAL);
    } else {
        for (const char* name : {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"}) {
            r.handle = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (r.handle) break;
        }
    }
    if (!r.handle) {
        r.error = std::string("librccl.so could not be loaded: ") + dlerror();
        return &r;
    }
    auto sym = [&](const char* n) { void* p = dlsym(r.handle, n); if (!p && r.error.empty()) r.error = std::string("librccl.so lacks ") + n; return p; };
    r.GetUniqueId = (decltype(r.GetUniqueId))sym("ncclGetUniqueId");
    r.CommInitRank = (decltype(r.CommInitRank))sym("ncclCommInitRank");
    r.CommDestroy = (decltype(r.CommDestroy))sym("ncclCommDestroy");
    r.GroupStart = (decltype(r.GroupStart))sym("ncclGroupStart");
    r.GroupEnd = (decltype(r.GroupEnd))sym("ncclGroupEnd");
    r.AllReduce = (decltype(r.AllReduce))sym("ncclAllReduce");
    r.GetErrorString = (decltype(r.GetErrorString))sym("ncclGetErrorString");
    return &r;
}
#define TRM_NCCL(ctx, call)                                                                                   \
    do {                                                                                                      \
        ncclResult_t e__ = (call);                                                                            \
        if (e__ != ncclSuccess) return fail(ctx, TRM_ECOMM, std::string(#call) + ": " + rccl()->GetErrorString(e__)); \
    } while (0)

// one all-reduce of `n` doubles over the context's communicator, on the side stream, after the context stream's work
int comm_allreduce(trm_ctx* c, double* host, int n, ncclRedOp_t op) {
    if (!c->comm) return fail(c, TRM_EINVAL, "no communicator: call trm_comm_init first");
    TRM_HIP(c, hipMemcpyAsync(c->d_comm, host, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->comm_stream));
    TRM_NCCL(c, rccl()->AllReduce(c->d_comm, c->d_comm + n, (size_t)n, ncclDouble, op, c->comm, c->comm_stream));
    TRM_HIP(c, hipMemcpyAsync(host, c->d_comm + n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->comm_stream));
    TRM_HIP(c, hipStreamSynchronize(c->comm_stream));
    return TRM_OK;
}

}  // namespace

namespace trmh {
int check_ctx_list(trm_ctx** ctxs, int n, const char* who) {
    if (!ctxs || n < 1) return fail(nullptr, TRM_EINVAL, std::string(who) + ": need at least one context");
    for (int i = 0; i < n; ++i)
        if (!ctxs[i]) return fail(nullptr, TRM_EINVAL, std::string(who) + ": null context in the list");
    for (int i = 1; i < n; ++i)
        if (ctxs[i]->Nz != ctxs[0]->Nz) return fail(ctxs[0], TRM_EINVAL, std::string(who) + ": the contexts are shards of one grid: same number of levels expected");
    // (a caller that holds only the list reads the first non-empty message: none may be left over from an earlier call)
    for (int i = 0; i < n; ++i) ctxs[i]->err.clear();
    return TRM_OK;
}
}  // namespace trmh

extern "C" {

// ---- multi-device diagnostics --------------------------------------------------------
int trm_comm_unique_id(void* id128) {
    if (!id128) return TRM_EINVAL;
    Rccl* r = rccl();
    if (!r->error.empty()) return fail(nullptr, TRM_ECOMM, r->error);
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    ncclUniqueId id;
    ncclResult_t e = r->GetUniqueId(&id);
    if (e != ncclSuccess) return fail(nullptr, TRM_ECOMM, std::string("ncclGetUniqueId: ") + r->GetErrorString(e));
    std::memcpy(id128, &id, sizeof(id));
    return TRM_OK;
}

namespace {
// communicators of one ncclUniqueId form one group: the grouped calls of trm_*_all refuse a list that mixes groups (RCCL would
// wait in ncclGroupEnd for ranks nobody posts)
uint64_t unique_id_hash(const ncclUniqueId& id) {
    uint64_t h = 1469598103934665603ull;
    for (size_t n = 0; n < sizeof(id); ++n) h = (h ^ (unsigned char)id.internal[n]) * 1099511628211ull;
    return h ? h : 1;
}
// the side stream and the send | receive buffer of a context's collectives
int comm_buffers(trm_ctx* c) {
    TRM_HIP(c, hipSetDevice(c->device));
    TRM_HIP(c, hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking));
    TRM_HIP(c, hipMalloc((void**)&c->d_comm, (size_t)(4 * (c->Nz + 1) + 16) * sizeof(double)));
    return TRM_OK;
}
}  // namespace

int trm_comm_init(trm_ctx* c, int rank, int world, const void* id128) {
    TRM_ENTER_HEUN(c);
    if (!id128 || world < 1 || rank < 0 || rank >= world) return fail(c, TRM_EINVAL, "trm_comm_init: bad argument");
    if (c->comm) return fail(c, TRM_EINVAL, "trm_comm_init: the context already has a communicator");
    Rccl* r = rccl();
    if (!r->error.empty()) return fail(c, TRM_ECOMM, r->error);
    ncclUniqueId id;
    std::memcpy(&id, id128, sizeof(id));
    TRM_NCCL(c, r->CommInitRank(&c->comm, world, id, rank));
    c->comm_rank = rank;
    c->comm_world = world;
    c->comm_group = unique_id_hash(id);
    if (int rc = comm_buffers(c)) {
        (void)trm_comm_destroy(c);
        return rc;
    }
    return TRM_OK;
}

int trm_comm_destroy(trm_ctx* c) {
    if (!c || !c->comm) return TRM_OK;
    (void)hipSetDevice(c->device);
    if (c->comm_stream) (void)hipStreamSynchronize(c->comm_stream);
    (void)rccl()->CommDestroy(c->comm);
    c->comm = nullptr;
    if (c->comm_stream) (void)hipStreamDestroy(c->comm_stream);
    c->comm_stream = nullptr;
    if (c->d_comm) (void)hipFree(c->d_comm);
    c->d_comm = nullptr;
    c->comm_world = 1;
    c->comm_rank = 0;
    c->comm_group = 0;
    return TRM_OK;
}

int trm_comm_info(const trm_ctx* c, int* rank, int* world) {
    if (!c) return TRM_EINVAL;
    if (rank) *rank = c->comm_rank;
    if (world) *world = c->comm ? c->comm_world : 0;
    return TRM_OK;
}

namespace {
// What travels for one reduction: the local per-row results, for MIN / MAX next to a NaN flag that travels with the same
// operator -- a NaN on any rank must reach every rank (Base.minimum / maximum), which RCCL's min / max do not promise.
int reduce_rows(const trm_ctx* c, int field, int op) { return op == TRM_REDUCE_VOLUME_INTEGRAL_Z ? 1 : (int)field_rows(c, field); }
int pack_reduce(int op, int rows, const double* local, std::vector<double>& buf) {
    if (op == TRM_REDUCE_MIN || op == TRM_REDUCE_MAX) {
        const double sentinel = op == TRM_REDUCE_MIN ? HUGE_VAL : -HUGE_VAL, yes = op == TRM_REDUCE_MIN ? -1.0 : 1.0;
        buf.assign((size_t)2 * rows, 0.0);
        for (int r = 0; r < rows; ++r) {
            const bool nan = local[r] != local[r];
            buf[r] = nan ? sentinel : local[r];
            buf[rows + r] = nan ? yes : 0.0;
        }
        return 2 * rows;
    }
    buf.assign(local, local + rows);
    return rows;
}
ncclRedOp_t reduce_operator(int op) { return op == TRM_REDUCE_MIN ? ncclMin : ((op == TRM_REDUCE_MAX || op == TRM_REDUCE_HASNAN) ? ncclMax : ncclSum); }
void unpack_reduce(int op, int rows, const std::vector<double>& buf, double* out) {
    if (op == TRM_REDUCE_MIN || op == TRM_REDUCE_MAX) {
        for (int r = 0; r < rows; ++r) out[r] = buf[rows + r] != 0.0 ? std::nan("") : buf[r];
        return;
    }
    for (int r = 0; r < rows; ++r) out[r] = buf[r];
}
// the all-reduce of the packed form on the HOST, ranks folded in order (one process: no wire needed); the folds of trm_reduce, so that
// the sign of a zero minimum / maximum does not depend on which shard held it
void fold_packed(int op, int n, std::vector<double>& acc, const std::vector<double>& x) {
    for (int j = 0; j < n; ++j) {
        if (op == TRM_REDUCE_MIN) acc[j] = nan_min(acc[j], x[j]);
        else if (op == TRM_REDUCE_MAX || op == TRM_REDUCE_HASNAN) acc[j] = nan_max(acc[j], x[j]);
        else acc[j] += x[j];
    }
}
// 1: every context holds rank i of n of ONE communicator group (the grouped all-reduce applies); 0: none has a communicator (host
// fold); -1: anything else -- communicators of different groups, a subset of a group, ranks out of order: refused, because the
// grouped call would post an incomplete set of ranks and RCCL would wait for the others forever
int comm_state(trm_ctx** ctxs, int n) {
    int with = 0;
    for (int i = 0; i < n; ++i) with += ctxs[i]->comm != nullptr;
    if (with == 0) return 0;
    if (with != n) return -1;
    for (int i = 0; i < n; ++i)
        if (ctxs[i]->comm_world != n || ctxs[i]->comm_rank != i || ctxs[i]->comm_group != ctxs[0]->comm_group) return -1;
    return 1;
}
const char* kMixedCommunicators = ": the contexts hold communicators that do not form ONE group in rank order (all of trm_comm_init_all's "
                                  "contexts, in its order) -- a grouped collective over them would wait for ranks nobody posts";
// n all-reduces of `count` doubles, one per context, issued from ONE thread inside a group (RCCL would otherwise block in the
// first one waiting for ranks this thread has not reached yet)
int grouped_allreduce(trm_ctx** ctxs, int n, std::vector<std::vector<double>>& bufs, int count, ncclRedOp_t op) {
    Rccl* r = rccl();
    for (int i = 0; i < n; ++i) {
        trm_ctx* c = ctxs[i];
        TRM_HIP(c, hipSetDevice(c->device));
        TRM_HIP(c, hipMemcpyAsync(c->d_comm, bufs[i].data(), (size_t)count * sizeof(double), hipMemcpyHostToDevice, c->comm_stream));
    }
    TRM_NCCL(ctxs[0], r->GroupStart());
    for (int i = 0; i < n; ++i) {
        trm_ctx* c = ctxs[i];
        const ncclResult_t e = r->AllReduce(c->d_comm, c->d_comm + count, (size_t)count, ncclDouble, op, c->comm, c->comm_stream);
        if (e != ncclSuccess) {
            (void)r->GroupEnd();
            return fail(c, TRM_ECOMM, std::string("ncclAllReduce: ") + r->GetErrorString(e));
        }
    }
    TRM_NCCL(ctxs[0], r->GroupEnd());
    for (int i = 0; i < n; ++i) {
        trm_ctx* c = ctxs[i];
        TRM_HIP(c, hipSetDevice(c->device));
        TRM_HIP(c, hipMemcpyAsync(bufs[i].data(), c->d_comm + count, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, c->comm_stream));
        TRM_HIP(c, hipStreamSynchronize(c->comm_stream));
    }
    return TRM_OK;
}
}  // namespace

int trm_reduce_global(trm_ctx* c, int field, int op, double* out) {
    int rc = trm_reduce(c, field, op, out);     // this device's columns (synchronous)
    if (rc) return rc;
    if (!c->comm) return fail(c, TRM_EINVAL, "trm_reduce_global: call trm_comm_init first");
    const int rows = reduce_rows(c, field, op);
    std::vector<double> buf;
    const int count = pack_reduce(op, rows, out, buf);
    rc = comm_allreduce(c, buf.data(), count, reduce_operator(op));
    if (rc) return rc;
    unpack_reduce(op, rows, buf, out);
    return TRM_OK;
}

int trm_status_global(trm_ctx* c, uint32_t* flags) {
    uint32_t local = 0;
    int rc = trm_status(c, &local);
    if (rc) return rc;
    if (!flags) return TRM_EINVAL;
    if (!c->comm) return fail(c, TRM_EINVAL, "trm_status_global: call trm_comm_init first");
    double bits[8];
    for (int b = 0; b < 8; ++b) bits[b] = (double)((local >> b) & 1u);
    rc = comm_allreduce(c, bits, 8, ncclMax);    // OR of the flag bits
    if (rc) return rc;
    *flags = 0;
    for (int b = 0; b < 8; ++b) *flags |= bits[b] != 0.0 ? (1u << b) : 0u;
    return TRM_OK;
}

// ---- one host thread, n contexts ("1 process x 8 HIP devices") ---------------------------------------------
int trm_comm_init_all(trm_ctx** ctxs, int n) {
    if (int rc = check_ctx_list(ctxs, n, "trm_comm_init_all")) return rc;
    for (int i = 0; i < n; ++i) {
        if (ctxs[i]->comm) return fail(ctxs[i], TRM_EINVAL, "trm_comm_init_all: the context already has a communicator");
        for (int j = 0; j < i; ++j)
            if (ctxs[j]->device == ctxs[i]->device && !std::getenv("TRM_RCCL_ALLOW_SHARED_DEVICE"))      // (tests: with tests/fake_rccl.c)
                return fail(ctxs[i], TRM_EINVAL, "trm_comm_init_all: two contexts on one device (RCCL takes one rank per device; without communicators "
                                                 "trm_reduce_global_all / trm_status_global_all combine the shards on the host)");
    }
    Rccl* r = rccl();
    if (!r->error.empty()) return fail(ctxs[0], TRM_ECOMM, r->error);
    ncclUniqueId id;
    TRM_NCCL(ctxs[0], r->GetUniqueId(&id));
    TRM_NCCL(ctxs[0], r->GroupStart());
    for (int i = 0; i < n; ++i) {
        trm_ctx* c = ctxs[i];
        ncclResult_t e = ncclSuccess;
        if (hipSetDevice(c->device) != hipSuccess) e = ncclUnhandledCudaError;
        if (e == ncclSuccess) e = r->CommInitRank(&c->comm, n, id, i);
        if (e != ncclSuccess) {
            (void)r->GroupEnd();
            // (the communicators handed out so far were never completed by a ncclGroupEnd that succeeded: nothing to destroy)
            for (int j = 0; j <= i; ++j) ctxs[j]->comm = nullptr;
            return fail(c, TRM_ECOMM, std::string("ncclCommInitRank (grouped): ") + r->GetErrorString(e));
        }
    }
    {
        const ncclResult_t e = r->GroupEnd();
        if (e != ncclSuccess) {
            for (int j = 0; j < n; ++j) ctxs[j]->comm = nullptr;
            return fail(ctxs[0], TRM_ECOMM, std::string("ncclGroupEnd: ") + r->GetErrorString(e));
        }
    }
    for (int i = 0; i < n; ++i) {
        trm_ctx* c = ctxs[i];
        c->comm_rank = i;
        c->comm_world = n;
        c->comm_group = unique_id_hash(id);
    }
    for (int i = 0; i < n; ++i) {
        trm_ctx* c = ctxs[i];
        if (int rc = comm_buffers(c)) {
            // a context without its stream / buffer must not keep a communicator (the grouped all-reduce would write through a
            // null pointer): the whole group goes, the failing context's message is the one reported
            const std::string msg = c->err;
            for (int j = 0; j < n; ++j) (void)trm_comm_destroy(ctxs[j]);
            return fail(ctxs[0], rc, "trm_comm_init_all: context " + std::to_string(i) + ": " + msg);
        }
    }
    return TRM_OK;
}

int trm_synchronize_all(trm_ctx** ctxs, int n) {
    if (int rc = check_ctx_list(ctxs, n, "trm_synchronize_all")) return rc;
    int rc = TRM_OK;
    for (int i = 0; i < n; ++i) {
        const int rs = trm_synchronize(ctxs[i]);
        if (!rc) rc = rs;
    }
    return rc;
}

int trm_reduce_global_all(trm_ctx** ctxs, int n, int field, int op, double* out) {
    if (int rc = check_ctx_list(ctxs, n, "trm_reduce_global_all")) return rc;
    if (!out || !valid_field(field)) return fail(ctxs[0], TRM_EINVAL, "trm_reduce_global_all: bad argument");
    const int rows = reduce_rows(ctxs[0], field, op);
    std::vector<std::vector<double>> bufs((size_t)n);
    std::vector<double> local((size_t)field_rows(ctxs[0], field) + 1);
    int count = 0;
    for (int i = 0; i < n; ++i) {
        int rc = trm_reduce(ctxs[i], field, op, local.data());       // this device's columns
        if (rc) return rc;
        count = pack_reduce(op, rows, local.data(), bufs[(size_t)i]);
    }
    const int cs = comm_state(ctxs, n);
    if (cs < 0) return fail(ctxs[0], TRM_EINVAL, std::string("trm_reduce_global_all") + kMixedCommunicators);
    if (n > 1 && cs == 1) {
        if (int rc = grouped_allreduce(ctxs, n, bufs, count, reduce_operator(op))) return rc;
    } else {
        for (int i = 1; i < n; ++i) fold_packed(op, count, bufs[0], bufs[(size_t)i]);
    }
    unpack_reduce(op, rows, bufs[0], out);
    return TRM_OK;
}

int trm_status_global_all(trm_ctx** ctxs, int n, uint32_t* flags) {
    if (int rc = check_ctx_list(ctxs, n, "trm_status_global_all")) return rc;
    if (!flags) return TRM_EINVAL;
    std::vector<std::vector<double>> bufs((size_t)n, std::vector<double>(8));
    for (int i = 0; i < n; ++i) {
        uint32_t local = 0;
        int rc = trm_status(ctxs[i], &local);
        if (rc) return rc;
        for (int b = 0; b < 8; ++b) bufs[(size_t)i][(size_t)b] = (double)((local >> b) & 1u);
    }
    const int cs = comm_state(ctxs, n);
    if (cs < 0) return fail(ctxs[0], TRM_EINVAL, std::string("trm_status_global_all") + kMixedCommunicators);
    if (n > 1 && cs == 1) {
        if (int rc = grouped_allreduce(ctxs, n, bufs, 8, ncclMax)) return rc;
    } else {
        for (int i = 1; i < n; ++i) fold_packed(TRM_REDUCE_MAX, 8, bufs[0], bufs[(size_t)i]);
    }
    *flags = 0;
    for (int b = 0; b < 8; ++b) *flags |= bufs[0][(size_t)b] != 0.0 ? (1u << b) : 0u;
    return TRM_OK;
}

}  // extern "C"
