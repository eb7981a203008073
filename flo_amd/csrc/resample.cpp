// resample.cpp — sample-rate conversion on the device (flo_resample_filter, flo_resample_out_frames, flo_batch_resample,
// flo_resample): a resident batch at one rate becomes a resident batch at another, every clip in one launch. Host code
// only: the filter, the index arithmetic and the geometry are resample_plan.cpp, the kernel is resample_kernels.hip.
#include <cstdlib>
#include <cstring>

#include "batch_internal.hpp"
#include "clip_tiles.hpp"
#include "devmem.hpp"
#include "resample_kernels.hpp"
#include "resample_plan.hpp"

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
// at d_dst + dst_off[i] (offsets in floats, even for stereo). The table and the work list go up through `pin` into `d_aux`
// (work_block_get); both belong to the caller, who keeps them until the stream has run the launch.
static int resample_enqueue(flo_ctx *c, const ResamplePlan &P, uint8_t ch, size_t n, const float *d_src, float *d_dst,
                            const std::vector<uint64_t> &src_off, const std::vector<uint64_t> &n_in, const std::vector<uint64_t> &dst_off,
                            const std::vector<uint64_t> &n_out, void *&d_aux, void *&pin) {
    std::vector<uint32_t> pre;
    if (!clip_tiles(n_out.data(), n, P.tile_outputs, pre)) return fail(c, FLO_ERR_ARG, "too many tiles for one resample launch");
    const uint32_t n_tiles = pre[n];
    if (!n_tiles) return FLO_OK;
    const std::vector<float> h = resample_table(P);
    BlockLayout B;   // table | src_off | n_in | dst_off | n_out | pre
    const size_t o_table = B.take(h.size() * 4), o_src = B.take(n * 8), o_in = B.take(n * 8), o_dst = B.take(n * 8), o_out = B.take(n * 8),
                 o_pre = B.take((n + 1) * 4);
    const size_t bytes = B.bytes;
    int rc = work_block_get(c, bytes, "resample work list", pin, d_aux);
    if (rc != FLO_OK) return rc;
    void *const host = pin, *const dev = d_aux;
    memcpy(B.at<float>(host, o_table), h.data(), h.size() * 4);
    memcpy(B.at<uint64_t>(host, o_src), src_off.data(), n * 8);
    memcpy(B.at<uint64_t>(host, o_in), n_in.data(), n * 8);
    memcpy(B.at<uint64_t>(host, o_dst), dst_off.data(), n * 8);
    memcpy(B.at<uint64_t>(host, o_out), n_out.data(), n * 8);
    memcpy(B.at<uint32_t>(host, o_pre), pre.data(), (n + 1) * 4);
    HIPCHK(c, hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, c->stream));
    ResampleArgs A;
    A.src = d_src;
    A.dst = d_dst;
    A.table = B.at<const float>(dev, o_table);
    A.src_off = B.at<const unsigned long long>(dev, o_src);
    A.n_in = B.at<const unsigned long long>(dev, o_in);
    A.dst_off = B.at<const unsigned long long>(dev, o_dst);
    A.n_out = B.at<const unsigned long long>(dev, o_out);
    A.pre = B.at<const unsigned int>(dev, o_pre);
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
    const std::vector<uint64_t> n_in = batch_whole_frames(src);
    std::vector<uint64_t> n_out(n);
    std::vector<size_t> n_il(n);
    for (size_t i = 0; i < n; i++) {
        if (!resample_out_frames(P, n_in[i], n_out[i]) || n_out[i] > (uint64_t)(SIZE_MAX / 8) / ch)
            return fail(c, FLO_ERR_ARG, "flo_batch_resample: a clip too long for this rate pair");
        n_il[i] = (size_t)(n_out[i] * ch);
    }
    BatchHold made;
    int rc = batch_derive(src, n, n_il.data(), out_rate, ch, &made.b);
    if (rc != FLO_OK) return rc;
    flo_batch *b = made.b;
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return fail(c, FLO_ERR_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));
    if (P.identity()) {   // equal rates: not filtered, a copy bit for bit
        for (size_t i = 0; i < n; i++) {
            if (!n_il[i]) continue;
            e = hipMemcpyAsync(b->d_pcm + b->clip_off[i], src->d_pcm + src->clip_off[i], n_il[i] * sizeof(float), hipMemcpyDeviceToDevice, c->stream);
            if (e != hipSuccess) return fail(c, FLO_ERR_DEVICE, std::string("hipMemcpyAsync: ") + hipGetErrorString(e));
        }
    } else {
        rc = resample_enqueue(c, P, ch, n, src->d_pcm, b->d_pcm, src->clip_off, n_in, b->clip_off, n_out, b->d_work, b->pin_work);
        if (rc != FLO_OK) return rc;
    }
    b->pcm_written = true;
    *out = made.release();
    return FLO_OK;
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
        rc = resample_enqueue(c, P, channels, 1, d_in.p, d_out.p, {0}, {n_in}, {0}, {n_out}, aux.p, pin);
        if (rc == FLO_OK) {
            e = hipMemcpyAsync(res, d_out.p, out_floats * sizeof(float), hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) rc = fail(c, FLO_ERR_DEVICE, std::string("flo_resample: ") + hipGetErrorString(e));
        }
    }
    if (pin) stager_pinned_put(c->stager, pin);
    return leave(rc);
}
