// context.cpp — the context of libflo_hip.so's C ABI (include/flo_hip.h): creation, error text, profiling hooks, the
// constant tables of a sample rate, the staging ring. Host code only.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ctx_internal.hpp"

thread_local std::string g_create_err;

int fail(flo_ctx *c, int code, const std::string &msg) {
    if (c) c->err = msg;
    return code;
}

int fetch_file(flo_ctx *c, const uint8_t *d_file, size_t n, const uint8_t *meta, size_t meta_len, int bit_depth, const char *what,
               uint8_t **out, size_t *out_len) {
    uint8_t *f = (uint8_t *)malloc(n + meta_len ? n + meta_len : 1);
    if (!f) return fail(c, FLO_ERR_NOMEM, "malloc failed");
    hipError_t e = hipMemcpy(f, d_file, n, hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        free(f);
        return fail(c, FLO_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
    }
    attach_meta(f, n, meta, meta_len);
    if (bit_depth >= 0) set_bit_depth(f, (uint8_t)bit_depth);
    *out = f;
    *out_len = n + meta_len;
    return FLO_OK;
}

extern "C" const char *flo_last_create_error(void) { return g_create_err.c_str(); }
extern "C" const char *flo_last_error(const flo_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }
extern "C" void flo_free(void *p) { free(p); }

extern "C" int flo_ctx_create(int device, flo_ctx **out) {
    if (!out) return FLO_ERR_ARG;
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) {
        g_create_err = std::string("no HIP device available: ") + (e != hipSuccess ? hipGetErrorString(e) : "count = 0") +
                       " (libflo_hip has no CPU fallback)";
        return FLO_ERR_DEVICE;
    }
    if (device < 0 || device >= n) {
        g_create_err = "device index out of range";
        return FLO_ERR_ARG;
    }
    flo_ctx *c = new flo_ctx();
    c->device = device;
    int prev_dev = -1;
    hipGetDevice(&prev_dev);   // the calling thread's current device is left as it was found
    auto restore = [&] {
        if (prev_dev >= 0 && prev_dev != device) hipSetDevice(prev_dev);
    };
    if ((e = hipSetDevice(device)) != hipSuccess || (e = hipGetDeviceProperties(&c->prop, device)) != hipSuccess ||
        (e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) {
        g_create_err = std::string("device init failed: ") + hipGetErrorString(e);
        delete c;
        restore();
        return FLO_ERR_DEVICE;
    }
    if (std::string(c->prop.gcnArchName).find("gfx950") == std::string::npos) {
        g_create_err = std::string("device is ") + c->prop.gcnArchName + ", this library carries gfx950 code only";
        hipStreamDestroy(c->stream);
        delete c;
        restore();
        return FLO_ERR_DEVICE;
    }
    {
        std::string serr;
        c->stager = stager_create(serr);   // light: pinned buffers and copy threads appear when first needed
    }
    if (const char *e2 = getenv("FLO_RESERVE_CUS")) {   // compute units left to other kernels (RCCL's, at N > 1)
        const int v = atoi(e2);
        if (v >= 0 && v < c->prop.multiProcessorCount) c->reserve_cus = v;
    }
    restore();
    *out = c;
    return FLO_OK;
}

extern "C" void flo_ctx_destroy(flo_ctx *c) {
    if (!c) return;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    sdec_work_free(c);
    lstream_work_free(c);
    for (auto *t : c->tables) {
        if (t->blob) hipFree(t->blob);
        delete t;
    }
    for (auto &r : c->prof) {
        hipEventDestroy(r.a);
        hipEventDestroy(r.b);
    }
    hipStreamDestroy(c->stream);
    if (c->stager) stager_destroy(c->stager);
    if (c->up_stream) hipStreamDestroy(c->up_stream);
    if (c->down_stream) hipStreamDestroy(c->down_stream);
    if (c->an_side.fork) hipEventDestroy(c->an_side.fork);
    for (int i = 0; i < 3; i++) {
        if (c->an_side.join[i]) hipEventDestroy(c->an_side.join[i]);
        if (c->an_side.st[i]) hipStreamDestroy(c->an_side.st[i]);
    }
    delete c;
}

extern "C" int flo_ctx_device_info(const flo_ctx *c, char *name, size_t cap, int *cus, uint64_t *hbm) {
    if (!c) return FLO_ERR_ARG;
    if (name && cap) snprintf(name, cap, "%s (%s)", c->prop.name, c->prop.gcnArchName);
    if (cus) *cus = c->prop.multiProcessorCount;
    if (hbm) *hbm = (uint64_t)c->prop.totalGlobalMem;
    return FLO_OK;
}
extern "C" void *flo_ctx_stream(flo_ctx *c) { return c ? (void *)c->stream : nullptr; }
extern "C" int flo_ctx_force_path(flo_ctx *c, int which) {
    if (!c || which < 0 || which > 5) return FLO_ERR_ARG;
    c->force_path = which;
    return FLO_OK;
}

// ---- profiling hooks -----------------------------------------------------------------------------------
extern "C" int flo_ctx_profile_enable(flo_ctx *c, int on) {
    if (!c) return FLO_ERR_ARG;
    c->profile = on != 0;
    return FLO_OK;
}
extern "C" int flo_ctx_profile_reset(flo_ctx *c) {
    if (!c) return FLO_ERR_ARG;
    for (auto &r : c->prof) {
        hipEventDestroy(r.a);
        hipEventDestroy(r.b);
    }
    c->prof.clear();
    c->prof_sum.clear();
    return FLO_OK;
}
// Fold every finished bracket into the per-kernel sums and destroy its events (a long profiled run keeps at most the
// launches since the last drain alive).
int profile_drain(flo_ctx *c, bool wait) {
    size_t keep = 0;
    for (size_t i = 0; i < c->prof.size(); i++) {
        ProfRec &r = c->prof[i];
        if (!wait && hipEventQuery(r.b) != hipSuccess) {
            if (keep != i) c->prof[keep] = r;   // not finished yet: stays queued
            keep++;
            continue;
        }
        float ms = 0;
        HIPCHK(c, hipEventSynchronize(r.b));
        HIPCHK(c, hipEventElapsedTime(&ms, r.a, r.b));
        ProfSum &ps = c->prof_sum[r.name];
        ps.ms += ms;
        ps.n++;
        hipEventDestroy(r.a);
        hipEventDestroy(r.b);
    }
    c->prof.resize(keep);
    return FLO_OK;
}
extern "C" int flo_ctx_profile_query(flo_ctx *c, const char *kernel, double *total_ms, uint64_t *launches) {
    if (!c || !kernel) return FLO_ERR_ARG;
    int rc = profile_drain(c, true);
    if (rc != FLO_OK) return rc;
    auto it = c->prof_sum.find(kernel);
    if (total_ms) *total_ms = it == c->prof_sum.end() ? 0.0 : it->second.ms;
    if (launches) *launches = it == c->prof_sum.end() ? 0 : it->second.n;
    return FLO_OK;
}

// ---- constant tables -----------------------------------------------------------------------------------
int get_tables(flo_ctx *c, uint32_t sr, float quality, TableSet **out) {
    float q = quality < 0.f ? 0.f : (quality > 1.f ? 1.f : quality);
    if (quality != quality) q = 0.f;  // NaN clamps to NaN in Rust; the threshold formula then yields NaN -> treat as 0
    for (auto *t : c->tables)
        if (t->host.sample_rate == sr && t->host.quality == q) {
            *out = t;
            return FLO_OK;
        }
    TableSet *t = new TableSet();
    build_lossy_tables(sr, q, t->host);
    const LossyTablesHost &h = t->host;
    struct Part {
        const void *src;
        size_t bytes;
        size_t off;
    };
    std::vector<Part> parts;
    size_t total = 0;
    auto add = [&](const void *p, size_t b) {
        total = (total + 255) & ~(size_t)255;
        parts.push_back({p, b, total});
        total += b;
        return parts.size() - 1;
    };
    size_t i_ext = add(h.pack_ext.data(), h.pack_ext.size() * 4);
    size_t i_pack = add(h.pack.data(), h.pack.size() * 4), i_athdb = add(h.ath_db.data(), h.ath_db.size() * 4),
           i_band = add(h.band.data(), h.band.size()), i_bc = add(h.band_count.data(), h.band_count.size() * 4),
           i_s10 = add(h.s10d.data(), h.s10d.size() * 4), i_lb = add(h.lane_bnd.data(), h.lane_bnd.size() * 4),
           i_ls = add(h.lane_slot0.data(), h.lane_slot0.size() * 4), i_bs = add(h.band_slot0.data(), h.band_slot0.size() * 4),
           i_win = add(h.window.data(), h.window.size() * 4), i_masks = add(&h.masks, sizeof(StatMasks));
    hipError_t e = hipMalloc(&t->blob, total);
    if (e != hipSuccess) {
        delete t;
        return fail(c, FLO_ERR_NOMEM, std::string("hipMalloc tables: ") + hipGetErrorString(e));
    }
    std::vector<uint8_t> stage(total, 0);
    for (auto &p : parts) memcpy(stage.data() + p.off, p.src, p.bytes);
    e = hipMemcpy(t->blob, stage.data(), total, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        hipFree(t->blob);
        delete t;
        return fail(c, FLO_ERR_DEVICE, std::string("hipMemcpy tables: ") + hipGetErrorString(e));
    }
    auto P = [&](size_t i) { return (const char *)t->blob + parts[i].off; };
    t->dev.pack = (const float4 *)P(i_pack);
    t->dev.pack_g = t->dev.pack;
    t->dev.pack_ext = (const float4 *)P(i_ext);
    t->dev.ath_db = (const float *)P(i_athdb);
    t->dev.band = (const uint8_t *)P(i_band);
    t->dev.band_count = (const float *)P(i_bc);
    t->dev.s10d = (const float *)P(i_s10);
    t->dev.lane_bnd = (const uint32_t *)P(i_lb);
    t->dev.lane_slot0 = (const uint32_t *)P(i_ls);
    t->dev.band_slot0 = (const uint32_t *)P(i_bs);
    t->dev_window = (const float *)P(i_win);
    t->dev_masks = (const StatMasks *)P(i_masks);
    t->dev.max_band_slots = h.max_band_slots;
    t->dev.dirty = h.dirty;
    t->dev.smr_thr = h.smr_threshold;
    t->dev.q_transparent = h.q_transparent;
    if (h.n_slots > kSlotCap || h.max_band_slots > 64 || !h.masks_ok) {   // (cannot happen: 64 lanes + 24 band edges, 64 lanes per band)
        hipFree(t->blob);
        delete t;
        return fail(c, FLO_ERR_ARG, "band segment table exceeds capacity");
    }
    c->tables.push_back(t);
    *out = t;
    return FLO_OK;
}

int ctx_stager(flo_ctx *c) {
    if (c->stager && c->up_stream) return FLO_OK;
    if (c->stager) {
        HIPCHK(c, hipStreamCreateWithFlags(&c->up_stream, hipStreamNonBlocking));
        HIPCHK(c, hipStreamCreateWithFlags(&c->down_stream, hipStreamNonBlocking));
        return FLO_OK;
    }
    std::string err;
    c->stager = stager_create(err);
    if (!c->stager) return fail(c, FLO_ERR_NOMEM, err);
    HIPCHK(c, hipStreamCreateWithFlags(&c->up_stream, hipStreamNonBlocking));
    HIPCHK(c, hipStreamCreateWithFlags(&c->down_stream, hipStreamNonBlocking));
    return FLO_OK;
}

extern "C" int flo_ctx_reserve_cus(flo_ctx *c, int n) {
    if (!c || n < 0 || n >= c->prop.multiProcessorCount) return FLO_ERR_ARG;
    c->reserve_cus = n;
    return FLO_OK;
}
extern "C" int flo_ctx_upload_path(flo_ctx *c, char *name, size_t cap, double *direct_gbs, double *ring_gbs) {
    if (!c) return FLO_ERR_ARG;
    int rc = ctx_stager(c);
    if (rc != FLO_OK) return rc;
    const char *n = stager_upload_choice(c->stager, direct_gbs, ring_gbs);
    if (name && cap) snprintf(name, cap, "%s", n);
    return FLO_OK;
}
extern "C" int flo_ctx_reserved_cus(flo_ctx *c) { return c ? (c->reserve_cus > 0 ? c->reserve_cus : 0) : -1; }
