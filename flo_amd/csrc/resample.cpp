// resample.cpp — sample-rate conversion on the device (flo_resample_filter, flo_resample_out_frames, flo_batch_resample,
// flo_resample): a resident batch at one rate becomes a resident batch at another, every clip in one launch. Host code
// only: the filter, the index arithmetic and the geometry are resample_plan.cpp, the kernel is resample_kernels.hip.
#include <cstdlib>
#include <cstring>

#include "batch_internal.hpp"
#include "devmem.hpp"
#include "resample_kernels.hpp"
#include "resample_plan.hpp"

static void put_err(char *err, size_t cap, const std::string &m) {
    if (err && cap) {
        strncpy(err, m.c_str(), cap - 1);
        err[cap - 1] = 0;
    }
}

extern "C" int flo_resample_filter(uint32_t in_rate, uint32_t out_rate, flo_resample_info *info, float **table, char *err, size_t err_cap) {
    if (table) *table = nullptr;
    ResamplePlan p;
    std::string m;
    if (!resample_plan(in_rate, out_rate, p, m)) {
        put_err(err, err_cap, m);
        return FLO_ERR_ARG;
    }
    if (info) *info = flo_resample_info{p.L, p.M, p.taps, p.tile_outputs};
    if (table) {
        const std::vector<float> h = resample_table(p);
        float *t = (float *)malloc(h.size() * sizeof(float));
        if (!t) {
            put_err(err, err_cap, "out of memory");
            return FLO_ERR_NOMEM;
        }
        memcpy(t, h.data(), h.size() * sizeof(float));
        *table = t;
    }
    return FLO_OK;
}

extern "C" int flo_resample_out_frames(uint32_t in_rate, uint32_t out_rate, uint64_t in_frames, uint64_t *out_frames) {
    ResamplePlan p;
    std::string m;
    if (!out_frames || !resample_plan(in_rate, out_rate, p, m)) return FLO_ERR_ARG;
    return resample_out_frames(p, in_frames, *out_frames) ? FLO_OK : FLO_ERR_ARG;
}

// Enqueue the conversion of n clips on the ctx stream: clip i's n_in[i] frames at d_src + src_off[i] become n_out[i] frames
// at d_dst + dst_off[i] (offsets in floats, even for stereo). The table and the work list go up through *pin into *d_aux;
// both belong to the caller, who keeps them until the stream has run the launch.
static int resample_enqueue(flo_ctx *c, const ResamplePlan &P, uint8_t ch, size_t n, const float *d_src, float *d_dst,
                            const std::vector<uint64_t> &src_off, const std::vector<uint64_t> &n_in, const std::vector<uint64_t> &dst_off,
                            const std::vector<uint64_t> &n_out, void **d_aux, void **pin) {
    std::vector<uint32_t> pre;
    if (!resample_tiles(P, n_out.data(), n, pre) || n > 0x7FFFFFFFull) return fail(c, FLO_ERR_ARG, "too many tiles for one resample launch");
    const uint32_t n_tiles = pre[n];
    if (!n_tiles) return FLO_OK;
    const std::vector<float> h = resample_table(P);
    // table | src_off | n_in | dst_off | n_out | pre
    const size_t table_bytes = (h.size() * 4 + 15) & ~(size_t)15, list_bytes = 4 * n * 8, bytes = table_bytes + list_bytes + (n + 1) * 4;
    std::string perr;
    uint8_t *host = (uint8_t *)stager_pinned_get(c->stager, bytes, perr);
    if (!host) return fail(c, FLO_ERR_NOMEM, perr);
    *pin = host;
    memcpy(host, h.data(), h.size() * 4);
    uint64_t *lists = (uint64_t *)(host + table_bytes);
    memcpy(lists, src_off.data(), n * 8);
    memcpy(lists + n, n_in.data(), n * 8);
    memcpy(lists + 2 * n, dst_off.data(), n * 8);
    memcpy(lists + 3 * n, n_out.data(), n * 8);
    memcpy(host + table_bytes + list_bytes, pre.data(), (n + 1) * 4);
    uint8_t *dev = nullptr;
    hipError_t e = pool_alloc(&dev, bytes);
    if (e != hipSuccess) return fail(c, e == hipErrorOutOfMemory ? FLO_ERR_NOMEM : FLO_ERR_DEVICE, std::string("resample work list: ") + hipGetErrorString(e));
    *d_aux = dev;
    HIPCHK(c, hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, c->stream));
    ResampleArgs A;
    A.src = d_src;
    A.dst = d_dst;
    A.table = (const float *)dev;
    const unsigned long long *dl = (const unsigned long long *)(dev + table_bytes);
    A.src_off = dl;
    A.n_in = dl + n;
    A.dst_off = dl + 2 * n;
    A.n_out = dl + 3 * n;
    A.pre = (const unsigned int *)(dev + table_bytes + list_bytes);
    A.n_clips = (unsigned)n;
    A.channels = ch;
    A.L = P.L;
    A.M = P.M;
    A.taps = P.taps;
    A.slots = P.slots;
    A.lanes_per_phase = P.lanes_per_phase;
    A.phases_per_wave = P.phases_per_wave;
    A.chunks = P.chunks;
    A.units = P.units;
    A.shift = P.shift;
    A.span = P.span;
    A.lds_elems = P.lds_elems;
    return timed_launch(c, "resample", [&] { return launch_resample(A, n_tiles, resample_lds_bytes(P, ch), c->stream); });
}

extern "C" int flo_batch_resample(flo_batch *src, uint32_t out_rate, flo_batch **out) {
    if (!src || !out) return FLO_ERR_ARG;
    *out = nullptr;
    flo_ctx *c = src->ctx;
    ResamplePlan P;
    std::string m;
    if (!resample_plan(src->sr, out_rate, P, m)) return fail(c, FLO_ERR_ARG, "flo_batch_resample: " + m);
    const size_t n = src->n_clips;
    const uint8_t ch = src->ch;
    std::vector<uint64_t> n_in(n), n_out(n);
    std::vector<size_t> n_il(n);
    for (size_t i = 0; i < n; i++) {
        n_in[i] = src->n_il[i] / ch;   // whole sample-frames: a kept partial frame (flo_batch::tail) is not carried over
        if (!resample_out_frames(P, n_in[i], n_out[i]) || n_out[i] > (uint64_t)(SIZE_MAX / 8) / ch)
            return fail(c, FLO_ERR_ARG, "flo_batch_resample: a clip too long for this rate pair");
        n_il[i] = (size_t)(n_out[i] * ch);
    }
    flo_batch *b = nullptr;
    int rc = flo_batch_create(c, src->mode, n, n_il.data(), out_rate, ch, src->qol, &b);
    if (rc != FLO_OK) return rc;
    b->bit_depth = src->bit_depth;
    b->exact = src->exact;
    auto leave = [&](int code) {
        if (code != FLO_OK) flo_batch_destroy(b);   // (waits for the stream first)
        else *out = b;
        return code;
    };
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return leave(fail(c, FLO_ERR_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e)));
    if (P.identity()) {   // equal rates: not filtered, a copy bit for bit
        for (size_t i = 0; i < n; i++) {
            if (!n_il[i]) continue;
            e = hipMemcpyAsync(b->d_pcm + b->clip_off[i], src->d_pcm + src->clip_off[i], n_il[i] * sizeof(float), hipMemcpyDeviceToDevice, c->stream);
            if (e != hipSuccess) return leave(fail(c, FLO_ERR_DEVICE, std::string("hipMemcpyAsync: ") + hipGetErrorString(e)));
        }
    } else {
        rc = resample_enqueue(c, P, ch, n, src->d_pcm, b->d_pcm, src->clip_off, n_in, b->clip_off, n_out, &b->d_resample, &b->pin_resample);
        if (rc != FLO_OK) return leave(rc);
    }
    b->pcm_written = true;
    return leave(FLO_OK);
}

extern "C" int flo_resample(flo_ctx *c, const float *pcm, size_t n_interleaved, uint32_t in_rate, uint32_t out_rate, uint8_t channels,
                            float **out, size_t *n_out_interleaved) {
    if (!c || !out || !n_out_interleaved || (!pcm && n_interleaved)) return FLO_ERR_ARG;
    *out = nullptr;
    *n_out_interleaved = 0;
    if (channels < 1 || channels > 8) return fail(c, FLO_ERR_ARG, "flo_resample: 1 to 8 channels");
    ResamplePlan P;
    std::string m;
    if (!resample_plan(in_rate, out_rate, P, m)) return fail(c, FLO_ERR_ARG, "flo_resample: " + m);
    const uint64_t n_in = n_interleaved / channels;
    uint64_t n_out = 0;
    if (!resample_out_frames(P, n_in, n_out) || n_out > (uint64_t)(SIZE_MAX / 8) / channels) return fail(c, FLO_ERR_ARG, "flo_resample: a clip too long for this rate pair");
    const size_t in_floats = (size_t)n_in * channels, out_floats = (size_t)n_out * channels;
    float *res = (float *)malloc(out_floats ? out_floats * sizeof(float) : 1);
    if (!res) return fail(c, FLO_ERR_NOMEM, "out of memory");
    auto leave = [&](int code) {
        if (code != FLO_OK) free(res);
        else *out = res, *n_out_interleaved = out_floats;
        return code;
    };
    if (!out_floats) return leave(FLO_OK);
    if (P.identity()) {
        memcpy(res, pcm, out_floats * sizeof(float));
        return leave(FLO_OK);
    }
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return leave(fail(c, FLO_ERR_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e)));
    DevBuf<float> d_in, d_out;
    DevMem aux;
    void *pin = nullptr;
    int rc;
    {
        QuiesceOnExit idle(c);
        if (!d_in.alloc(in_floats + 4) || !d_out.alloc(out_floats + 4)) return leave(fail(c, FLO_ERR_NOMEM, "flo_resample: device memory"));
        e = hipMemcpyAsync(d_in.p, pcm, in_floats * sizeof(float), hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) return leave(fail(c, FLO_ERR_DEVICE, std::string("hipMemcpyAsync: ") + hipGetErrorString(e)));
        rc = resample_enqueue(c, P, channels, 1, d_in.p, d_out.p, {0}, {n_in}, {0}, {n_out}, &aux.p, &pin);
        if (rc == FLO_OK) {
            e = hipMemcpyAsync(res, d_out.p, out_floats * sizeof(float), hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) rc = fail(c, FLO_ERR_DEVICE, std::string("flo_resample: ") + hipGetErrorString(e));
        }
    }
    if (pin) stager_pinned_put(c->stager, pin);
    return leave(rc);
}
