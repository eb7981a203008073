// dist.cpp — the multi-GPU exchange (flo_dist_*), written directly against RCCL.
#include <rccl/rccl.h>

#include <cstring>

#include "batch_internal.hpp"
#include "container_kernels.hpp"
#include "dist_engine.hpp"

static const int kDefaultReservedCus = 8;

// One process per GPU. Clips shard across ranks with no data-path collective during the encode; the one
// exchange step per batch is a variable-size gather of every rank's finished .flo files to the root, written directly
// against RCCL: ncclAllGather of one u64 per rank (the packed size), then grouped ncclSend / ncclRecv - on the fully
// connected xGMI node every peer has its own link to the root, so the seven transfers run in parallel where a ring
// collective would be bound by one link. Everything runs on a side stream of its own and is double-buffered: the
// transfer of step k overlaps the encode of step k + 1. No host synchronisation sits on that path: the sizes of step k
// travel to pinned host memory asynchronously and are only read when step k + 1 is submitted (by then they have long
// arrived), which is when the transfers of step k are posted; flo_dist_gather_flush posts and awaits the last ones.
// The ordering logic (slot parity, deferred posting, buffer growth) is the DistEngine template of dist_engine.hpp; here it
// is bound to HIP streams and RCCL. tests/native/dist_engine_test.cpp runs the same template over sockets with several
// ranks on the CPU.
#define NCCLRC(ctx, expr)                                                                               \
    do {                                                                                                \
        ncclResult_t r_ = (expr);                                                                       \
        if (r_ != ncclSuccess) return fail(ctx, FLO_ERR_DEVICE, std::string(#expr) + ": " + ncclGetErrorString(r_)); \
    } while (0)

struct RcclBackend {
    struct Buffer {
        uint8_t *p = nullptr;
        size_t cap = 0;
    };
    flo_ctx *ctx = nullptr;
    ncclComm_t comm = nullptr;
    int world = 1;
    hipStream_t cs = nullptr;                 // communication stream
    uint64_t *d_sizes[2] = {nullptr, nullptr};   // [world] device
    uint64_t *h_sizes[2] = {nullptr, nullptr};   // [world] pinned host
    uint64_t *h_mine[2] = {nullptr, nullptr};    // pinned host: this rank's packed size
    uint64_t *d_mine[2] = {nullptr, nullptr};
    hipEvent_t ev_packed[2] = {nullptr, nullptr}, ev_sizes[2] = {nullptr, nullptr}, ev_moved[2] = {nullptr, nullptr};
    std::vector<uint64_t> pack_off;           // scratch: per-clip offsets of the last pack

    // (re)allocate a device buffer to hold `need` bytes; growing waits for the work that may still use the old one
    int reserve(Buffer &b, size_t need) {
        if (b.cap >= need) return FLO_OK;
        flo_ctx *c = ctx;
        HIPCHK(c, hipStreamSynchronize(cs));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (b.p) HIPCHK(c, hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
        const size_t want = need + need / 4 + 4096;
        hipError_t e = hipMalloc(&b.p, want);
        if (e != hipSuccess) return fail(c, FLO_ERR_NOMEM, std::string("gather buffer: ") + hipGetErrorString(e));
        b.cap = want;
        return FLO_OK;
    }
    int payload_bytes(flo_batch *b, uint64_t *need) {
        const uint8_t *base;
        const uint64_t *offs, *sizes;
        int rc = flo_batch_device_files(b, &base, &offs, &sizes);
        if (rc != FLO_OK) return rc;
        *need = packed_offsets(sizes, b->n_clips, nullptr);
        return FLO_OK;
    }
    int pack(flo_batch *b, Buffer &dst, uint64_t *bytes) {
        pack_off.resize(b->n_clips + 1);
        int rc = flo_batch_pack_files(b, dst.p, dst.cap, pack_off.data());
        if (rc != FLO_OK) return rc;
        *bytes = pack_off[b->n_clips];
        return FLO_OK;
    }
    int wait_moved_before_pack(int s) {
        HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ev_moved[s], 0));
        return FLO_OK;
    }
    int mark_packed(int s) {
        HIPCHK(ctx, hipEventRecord(ev_packed[s], ctx->stream));
        return FLO_OK;
    }
    int sizes_exchange(int s, uint64_t mine) {
        flo_ctx *c = ctx;
        *h_mine[s] = mine;
        HIPCHK(c, hipMemcpyAsync(d_mine[s], h_mine[s], 8, hipMemcpyHostToDevice, cs));
        NCCLRC(c, ncclAllGather(d_mine[s], d_sizes[s], 1, ncclUint64, comm, cs));
        HIPCHK(c, hipMemcpyAsync(h_sizes[s], d_sizes[s], (size_t)world * 8, hipMemcpyDeviceToHost, cs));
        HIPCHK(c, hipEventRecord(ev_sizes[s], cs));
        return FLO_OK;
    }
    int sizes_wait(int s, const uint64_t **sizes) {
        HIPCHK(ctx, hipEventSynchronize(ev_sizes[s]));
        *sizes = h_sizes[s];
        return FLO_OK;
    }
    int comm_waits_for_pack(int s) {
        HIPCHK(ctx, hipStreamWaitEvent(cs, ev_packed[s], 0));
        return FLO_OK;
    }
    int copy_own(Buffer &dst, size_t off, Buffer &src, size_t n) {
        HIPCHK(ctx, hipMemcpyAsync(dst.p + off, src.p, n, hipMemcpyDeviceToDevice, cs));
        return FLO_OK;
    }
    int group_begin() {
        NCCLRC(ctx, ncclGroupStart());
        return FLO_OK;
    }
    int recv(Buffer &dst, size_t off, size_t n, int peer) {
        NCCLRC(ctx, ncclRecv(dst.p + off, n, ncclUint8, peer, comm, cs));
        return FLO_OK;
    }
    int send(Buffer &src, size_t n, int peer) {
        NCCLRC(ctx, ncclSend(src.p, n, ncclUint8, peer, comm, cs));
        return FLO_OK;
    }
    int group_end() {
        NCCLRC(ctx, ncclGroupEnd());
        return FLO_OK;
    }
    int mark_moved(int s) {
        HIPCHK(ctx, hipEventRecord(ev_moved[s], cs));
        return FLO_OK;
    }
    int drain() {
        HIPCHK(ctx, hipStreamSynchronize(cs));
        return FLO_OK;
    }
};

// Second exchange mode (flo_dist_table_*): the files stay where they were made, one ncclAllGather tells every rank where
// each file of every rank lies (offset in its owner's device buffer), how long it is and the CRC32 of its DATA chunk.
struct TableSlot {
    uint64_t *h_mine = nullptr, *d_mine = nullptr, *d_all = nullptr, *h_all = nullptr;   // pinned / device rows
    size_t words = 0;                 // capacity of one row, in u64
    hipEvent_t done = nullptr;
    bool used = false;
};
struct flo_dist {
    flo_ctx *ctx = nullptr;
    RcclBackend be;
    flo::DistEngine<RcclBackend> eng;
    TableSlot tab[2];
    uint64_t tab_steps = 0;
    size_t tab_max = 0;               // max_clips of the last submit
    bool defaulted_reserve = false;   // flo_dist_create set the context's CU reservation (and flo_dist_destroy takes it back)
};

extern "C" int flo_dist_unique_id(uint8_t *id) {
    if (!id) return FLO_ERR_ARG;
    static_assert(FLO_DIST_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "unique id size");
    ncclUniqueId u;
    ncclResult_t r = ncclGetUniqueId(&u);
    if (r != ncclSuccess) {
        g_create_err = std::string("ncclGetUniqueId: ") + ncclGetErrorString(r);
        return FLO_ERR_DEVICE;
    }
    memcpy(id, u.internal, NCCL_UNIQUE_ID_BYTES);
    return FLO_OK;
}

extern "C" void flo_dist_destroy(flo_dist *d) {
    if (!d) return;
    RcclBackend &be = d->be;
    hipSetDevice(d->ctx->device);
    if (be.cs) hipStreamSynchronize(be.cs);
    for (int s = 0; s < 2; s++) {
        if (d->eng.send[s].p) hipFree(d->eng.send[s].p);
        if (d->eng.recv[s].p) hipFree(d->eng.recv[s].p);
        if (be.d_sizes[s]) hipFree(be.d_sizes[s]);
        if (be.d_mine[s]) hipFree(be.d_mine[s]);
        if (be.h_sizes[s]) hipHostFree(be.h_sizes[s]);
        if (be.h_mine[s]) hipHostFree(be.h_mine[s]);
        if (be.ev_packed[s]) hipEventDestroy(be.ev_packed[s]);
        if (be.ev_sizes[s]) hipEventDestroy(be.ev_sizes[s]);
        if (be.ev_moved[s]) hipEventDestroy(be.ev_moved[s]);
    }
    for (auto &t : d->tab) {
        if (t.h_mine) hipHostFree(t.h_mine);
        if (t.h_all) hipHostFree(t.h_all);
        if (t.d_mine) hipFree(t.d_mine);
        if (t.d_all) hipFree(t.d_all);
        if (t.done) hipEventDestroy(t.done);
    }
    if (be.comm) ncclCommDestroy(be.comm);
    if (be.cs) hipStreamDestroy(be.cs);
    if (d->defaulted_reserve) d->ctx->reserve_cus = -1;   // later single-GPU encodes on this context get every CU back
    delete d;
}

extern "C" int flo_dist_create(flo_ctx *c, const uint8_t *id, int rank, int world, int root, flo_dist **out) {
    if (!c || !id || !out || world < 1 || rank < 0 || rank >= world || root < 0 || root >= world) return FLO_ERR_ARG;
    *out = nullptr;
    HIPCHK(c, hipSetDevice(c->device));
    flo_dist *d = new flo_dist();
    d->ctx = c;
    RcclBackend &be = d->be;
    be.ctx = c;
    be.world = world;
    d->eng.init(&be, rank, world, root);
    auto bail = [&](int rc) {
        flo_dist_destroy(d);
        return rc;
    };
    if (hipStreamCreateWithFlags(&be.cs, hipStreamNonBlocking) != hipSuccess) return bail(fail(c, FLO_ERR_DEVICE, "hipStreamCreate (communication stream)"));
    ncclUniqueId u;
    memcpy(u.internal, id, NCCL_UNIQUE_ID_BYTES);
    ncclResult_t r = ncclCommInitRank(&be.comm, world, u, rank);
    if (r != ncclSuccess) return bail(fail(c, FLO_ERR_DEVICE, std::string("ncclCommInitRank: ") + ncclGetErrorString(r)));
    for (int s = 0; s < 2; s++) {
        if (hipMalloc(&be.d_sizes[s], (size_t)world * 8) != hipSuccess || hipMalloc(&be.d_mine[s], 8) != hipSuccess ||
            hipHostMalloc(&be.h_sizes[s], (size_t)world * 8) != hipSuccess || hipHostMalloc(&be.h_mine[s], 8) != hipSuccess ||
            hipEventCreateWithFlags(&be.ev_packed[s], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&be.ev_sizes[s], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&be.ev_moved[s], hipEventDisableTiming) != hipSuccess)
            return bail(fail(c, FLO_ERR_NOMEM, "flo_dist_create: buffers"));
    }
    // RCCL's send / receive are kernels: with more than one rank the persistent chain kernel leaves a few compute units
    // free for them, or the transfer of step k could not start before the encode of step k + 1 has ended
    // (flo_ctx_reserve_cus; an explicit setting or FLO_RESERVE_CUS wins)
    if (world > 1 && c->reserve_cus < 0) {
        c->reserve_cus = kDefaultReservedCus;
        d->defaulted_reserve = true;
    }
    *out = d;
    return FLO_OK;
}

extern "C" int flo_dist_table_submit(flo_dist *d, flo_batch *b, size_t max_clips) {
    if (!d || !b) return FLO_ERR_ARG;
    flo_ctx *c = d->ctx;
    if (b->ctx != c) return fail(c, FLO_ERR_ARG, "batch and communicator belong to different contexts");
    if (!b->synced) return fail(c, FLO_ERR_STATE, "call flo_batch_encode + flo_batch_sync first");
    if (b->n_clips > max_clips) return fail(c, FLO_ERR_ARG, "flo_dist_table_submit: max_clips is smaller than this rank's clip count");
    HIPCHK(c, hipSetDevice(c->device));
    RcclBackend &be = d->be;
    TableSlot &t = d->tab[d->tab_steps & 1];
    const size_t words = 1 + 3 * max_clips;
    if (t.used) HIPCHK(c, hipEventSynchronize(t.done));   // this slot's previous round trip (two steps ago): long over
    if (t.words < words) {
        if (t.h_mine) hipHostFree(t.h_mine);
        if (t.h_all) hipHostFree(t.h_all);
        if (t.d_mine) hipFree(t.d_mine);
        if (t.d_all) hipFree(t.d_all);
        t.h_mine = t.h_all = t.d_mine = t.d_all = nullptr;
        t.words = 0;
        if (hipHostMalloc(&t.h_mine, words * 8) != hipSuccess || hipHostMalloc(&t.h_all, words * 8 * (size_t)be.world) != hipSuccess ||
            hipMalloc(&t.d_mine, words * 8) != hipSuccess || hipMalloc(&t.d_all, words * 8 * (size_t)be.world) != hipSuccess)
            return fail(c, FLO_ERR_NOMEM, "flo_dist_table_submit: buffers");
        if (!t.done && hipEventCreateWithFlags(&t.done, hipEventDisableTiming) != hipSuccess) return fail(c, FLO_ERR_NOMEM, "flo_dist_table_submit: event");
        t.words = words;
    }
    const uint8_t *base;
    const uint64_t *offs, *sizes;
    int rc = flo_batch_device_files(b, &base, &offs, &sizes);
    if (rc != FLO_OK) return rc;
    memset(t.h_mine, 0, words * 8);
    t.h_mine[0] = b->n_clips;
    for (size_t i = 0; i < b->n_clips; i++) {
        t.h_mine[1 + i] = sizes[i];
        t.h_mine[1 + max_clips + i] = offs[i];
    }
    HIPCHK(c, hipMemcpyAsync(t.d_mine, t.h_mine, words * 8, hipMemcpyHostToDevice, be.cs));
    // (the batch is synced: its files, CRC fields included, are complete; nothing on the encode stream to wait for)
    if (flo::launch_table_crcs(base, (unsigned long long *)t.d_mine, b->n_clips, max_clips, be.cs) != 0)
        return fail(c, FLO_ERR_DEVICE, "flo_dist_table_submit: table kernel");
    NCCLRC(c, ncclAllGather(t.d_mine, t.d_all, words, ncclUint64, be.comm, be.cs));
    HIPCHK(c, hipMemcpyAsync(t.h_all, t.d_all, words * 8 * (size_t)be.world, hipMemcpyDeviceToHost, be.cs));
    HIPCHK(c, hipEventRecord(t.done, be.cs));
    t.used = true;
    d->tab_max = max_clips;
    d->tab_steps++;
    return FLO_OK;
}

extern "C" int flo_dist_table_flush(flo_dist *d) {
    if (!d) return FLO_ERR_ARG;
    HIPCHK(d->ctx, hipSetDevice(d->ctx->device));
    for (auto &t : d->tab)
        if (t.used) HIPCHK(d->ctx, hipEventSynchronize(t.done));
    return FLO_OK;
}

extern "C" int flo_dist_table_result(flo_dist *d, const uint64_t **rows, size_t *row_words, size_t *max_clips) {
    if (!d) return FLO_ERR_ARG;
    if (!d->tab_steps) return fail(d->ctx, FLO_ERR_STATE, "no table has been submitted yet");
    const TableSlot &t = d->tab[(d->tab_steps - 1) & 1];
    HIPCHK(d->ctx, hipEventSynchronize(t.done));
    if (rows) *rows = t.h_all;
    if (row_words) *row_words = 1 + 3 * d->tab_max;
    if (max_clips) *max_clips = d->tab_max;
    return FLO_OK;
}

extern "C" int flo_dist_gather_submit(flo_dist *d, flo_batch *b) {
    if (!d || !b) return FLO_ERR_ARG;
    flo_ctx *c = d->ctx;
    if (b->ctx != c) return fail(c, FLO_ERR_ARG, "batch and communicator belong to different contexts");
    if (!b->synced) return fail(c, FLO_ERR_STATE, "call flo_batch_encode + flo_batch_sync first");
    HIPCHK(c, hipSetDevice(c->device));
    return d->eng.submit(b);
}

extern "C" int flo_dist_gather_flush(flo_dist *d) {
    if (!d) return FLO_ERR_ARG;
    HIPCHK(d->ctx, hipSetDevice(d->ctx->device));
    return d->eng.flush();
}

extern "C" int flo_dist_gather_result(flo_dist *d, const uint8_t **base, const uint64_t **rank_offsets,
                                      const uint64_t **rank_sizes) {
    if (!d) return FLO_ERR_ARG;
    if (d->eng.rank != d->eng.root) return fail(d->ctx, FLO_ERR_STATE, "only the root holds the gathered files");
    if (d->eng.res_slot < 0) return fail(d->ctx, FLO_ERR_STATE, "nothing has been gathered yet");
    if (base) *base = d->eng.recv[d->eng.res_slot].p;
    if (rank_offsets) *rank_offsets = d->eng.res_off.data();
    if (rank_sizes) *rank_sizes = d->eng.res_size.data();
    return FLO_OK;
}

extern "C" void *flo_dist_stream(flo_dist *d) { return d ? (void *)d->be.cs : nullptr; }
