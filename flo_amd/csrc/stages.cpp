// stages.cpp — the stage entry points (flo_mdct_forward, flo_lossy_analyze / quantize / pack_frames / quantize_smr, flo_sparse_pack):
// single stages of the lossy encoder on host buffers, for tests against the reference's stages.
#include <cstring>

#include "batch_internal.hpp"
#include "devmem.hpp"
#include "lossy_kernels.hpp"

extern "C" int flo_mdct_forward(flo_ctx *c, const float *frames, size_t n_frames, float *coeffs) {
    if (!c || (n_frames && (!frames || !coeffs))) return FLO_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (!n_frames) return FLO_OK;
    TableSet *ts;
    int rc = get_tables(c, 44100, 0.55f, &ts);
    if (rc != FLO_OK) return rc;
    DevBuf<float> d_in, d_out;
    QuiesceOnExit quiesce(c);
    if (!d_in.alloc(n_frames * 2048) || !d_out.alloc(n_frames * 1024)) return fail(c, FLO_ERR_DEVICE, "flo_mdct_forward: device buffers");
    hipError_t e = hipMemcpyAsync(d_in.p, frames, n_frames * 2048 * sizeof(float), hipMemcpyHostToDevice, c->stream);
    int lrc = 0;
    if (e == hipSuccess) e = stream_delay(c->stream);   // (these launches bypass timed_launch)
    if (e == hipSuccess) lrc = launch_mdct_only(ts->dev, d_in.p, n_frames, d_out.p, c->stream);
    if (e == hipSuccess && lrc == 0)
        e = hipMemcpyAsync(coeffs, d_out.p, n_frames * 1024 * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    hipError_t e2 = hipStreamSynchronize(c->stream);
    if (e != hipSuccess || e2 != hipSuccess || lrc != 0)
        return fail(c, FLO_ERR_DEVICE, std::string("flo_mdct_forward: ") + hipGetErrorString(e != hipSuccess ? e : e2));
    return FLO_OK;
}

static int analyze_common(flo_ctx *c, const float *pcm, size_t n, const float *in_coeffs, size_t in_hops, uint32_t sr,
                          uint8_t ch, float quality, int exact, float *coeffs, int16_t *q, uint16_t *sfw, size_t *num_hops,
                          uint8_t *data = nullptr, size_t data_cap = 0, size_t *data_len = nullptr, uint32_t *frame_sizes = nullptr) {
    flo_batch *b = nullptr;
    size_t n_il = in_coeffs ? (in_hops ? (in_hops - 1) * 1024 * ch : 0) : n;
    if (in_coeffs && in_hops == 0) return FLO_OK;
    int rc = flo_batch_create(c, FLO_MODE_LOSSY, 1, &n_il, sr, ch, quality, &b);
    if (rc != FLO_OK) return rc;
    const size_t hops = b->hops[0];
    if (num_hops) *num_hops = hops;
    DevBuf<float> d_in;   // (released behind every done(): the batch's destruction has waited for the stream)
    auto done = [&](int code) {
        flo_batch_destroy(b);
        return code;
    };
    const size_t per = hops * ch;
    if (pool_alloc(&b->d_dbg_coeffs, per * 1024 * 4 + 16) != hipSuccess || pool_alloc(&b->d_dbg_q, per * 1024 * 2 + 16) != hipSuccess ||
        pool_alloc(&b->d_dbg_sfw, per * 25 * 2 + 16) != hipSuccess)
        return done(fail(c, FLO_ERR_NOMEM, "hipMalloc analysis buffers"));
    if (in_coeffs) {
        if (!d_in.alloc(per * 1024)) return done(fail(c, FLO_ERR_NOMEM, "hipMalloc"));
        if (hipMemcpy(d_in.p, in_coeffs, per * 1024 * 4, hipMemcpyHostToDevice) != hipSuccess)
            return done(fail(c, FLO_ERR_DEVICE, "hipMemcpy"));
        b->d_in_coeffs = d_in.p;
        b->exact = exact ? 1 : 0;
    } else {
        rc = flo_batch_upload(b, 0, pcm);
        if (rc != FLO_OK) return done(rc);
    }
    rc = flo_batch_encode(b, 0);   // the plan's analysis default: the forced form, else 1
    if (rc == FLO_OK) rc = flo_batch_sync(b);
    if (rc != FLO_OK) return done(rc);
    hipError_t e = hipSuccess;
    if (coeffs && !in_coeffs) e = hipMemcpy(coeffs, b->d_dbg_coeffs, per * 1024 * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && q) e = hipMemcpy(q, b->d_dbg_q, per * 1024 * 2, hipMemcpyDeviceToHost);
    if (e == hipSuccess && sfw) e = hipMemcpy(sfw, b->d_dbg_sfw, per * 25 * 2, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return done(fail(c, FLO_ERR_DEVICE, std::string("analysis D2H: ") + hipGetErrorString(e)));
    if (data_len) {   // the clip's DATA chunk and frame sizes, read out of its finished file (header 70 bytes, TOC, DATA)
        uint8_t *file = nullptr;
        size_t len = 0;
        rc = flo_batch_fetch(b, 0, nullptr, 0, &file, &len);
        if (rc != FLO_OK) return done(rc);
        uint32_t n_toc = 0;
        uint64_t toc_size = 0, data_size = 0;
        bool ok = len >= kFileHeaderBytes;
        if (ok) {
            memcpy(&toc_size, file + 38, 8);
            memcpy(&data_size, file + 46, 8);
            memcpy(&n_toc, file + 70, 4);
            ok = n_toc == hops && toc_size == 4 + kTocEntryBytes * hops && 70 + toc_size + data_size <= len;
        }
        if (ok && data_size > data_cap) {
            flo_free(file);
            return done(fail(c, FLO_ERR_ARG, "output buffer too small"));
        }
        if (ok) {
            for (size_t h = 0; frame_sizes && h < hops; h++) memcpy(&frame_sizes[h], file + head_bytes(h) + 12, 4);
            if (data_size) memcpy(data, file + 70 + toc_size, data_size);
            *data_len = data_size;
        }
        flo_free(file);
        if (!ok) return done(fail(c, FLO_ERR_DEVICE, "flo_lossy_pack_frames: the finished file does not parse"));
    }
    return done(FLO_OK);
}

extern "C" int flo_lossy_analyze(flo_ctx *c, const float *pcm, size_t n, uint32_t sr, uint8_t ch, float quality,
                                 float *coeffs, int16_t *q, uint16_t *sfw, size_t *num_hops) {
    if (!c || (n && !pcm)) return FLO_ERR_ARG;
    return analyze_common(c, pcm, n, nullptr, 0, sr, ch, quality, 0, coeffs, q, sfw, num_hops);
}
extern "C" int flo_lossy_quantize(flo_ctx *c, const float *coeffs, size_t num_hops, uint32_t sr, uint8_t ch,
                                  float quality, int exact, int16_t *q, uint16_t *sfw) {
    if (!c || (num_hops && !coeffs)) return FLO_ERR_ARG;
    return analyze_common(c, nullptr, 0, coeffs, num_hops, sr, ch, quality, exact, nullptr, q, sfw, nullptr);
}

extern "C" int flo_lossy_pack_frames(flo_ctx *c, const float *coeffs, size_t num_hops, uint32_t sr, uint8_t ch, float quality,
                                     int16_t *q, uint16_t *sfw, uint8_t *data, size_t data_cap, size_t *data_len, uint32_t *frame_sizes) {
    if (!c || !data_len || (num_hops && (!coeffs || !data || !frame_sizes))) return FLO_ERR_ARG;
    *data_len = 0;
    return analyze_common(c, nullptr, 0, coeffs, num_hops, sr, ch, quality, 0, nullptr, q, sfw, nullptr, data, data_cap, data_len, frame_sizes);
}

extern "C" int flo_lossy_quantize_smr(flo_ctx *c, const float *coeffs, const float *smr, size_t n_vec, uint32_t sr, float quality,
                                      int16_t *q, float *scale_factors) {
    if (!c || (n_vec && (!coeffs || !scale_factors || (smr && !q)))) return FLO_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (!n_vec) return FLO_OK;
    TableSet *ts;
    int rc = get_tables(c, sr, quality, &ts);
    if (rc != FLO_OK) return rc;
    DevBuf<float> d_c, d_smr, d_sf;   // (d_smr, d_q: only with an SMR, null otherwise)
    DevBuf<short> d_q;
    QuiesceOnExit quiesce(c);
    if (!d_c.alloc(n_vec * 1024) || !d_sf.alloc(n_vec * 25) || (smr && (!d_smr.alloc(n_vec * 1024) || !d_q.alloc(n_vec * 1024))))
        return fail(c, FLO_ERR_DEVICE, "flo_lossy_quantize_smr: device buffers");
    hipError_t e = hipMemcpyAsync(d_c.p, coeffs, n_vec * 4096, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && smr) e = hipMemcpyAsync(d_smr.p, smr, n_vec * 4096, hipMemcpyHostToDevice, c->stream);
    int lrc = 0;
    if (e == hipSuccess) e = stream_delay(c->stream);
    if (e == hipSuccess) lrc = launch_quantise_smr(ts->dev, d_c.p, d_smr.p, n_vec, d_q.p, d_sf.p, c->stream);
    if (e == hipSuccess && lrc == 0) e = hipMemcpyAsync(scale_factors, d_sf.p, n_vec * 100, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && lrc == 0 && smr) e = hipMemcpyAsync(q, d_q.p, n_vec * 2048, hipMemcpyDeviceToHost, c->stream);
    hipError_t e2 = hipStreamSynchronize(c->stream);
    if (e != hipSuccess || e2 != hipSuccess || lrc != 0)
        return fail(c, FLO_ERR_DEVICE, std::string("flo_lossy_quantize_smr: ") + hipGetErrorString(e != hipSuccess ? e : e2));
    return FLO_OK;
}

extern "C" int flo_sparse_pack(flo_ctx *c, const int16_t *q, size_t n_vec, int form, uint8_t *out, size_t out_cap,
                               uint32_t *out_off) {
    if (!c || (n_vec && (!q || !out || !out_off)) || form < 0 || form > 2) return FLO_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (out_off) out_off[0] = 0;
    if (!n_vec) return FLO_OK;
    std::vector<uint8_t> slots(n_vec * 2080);   // (in front of the guard: the copies into them have ended when they go)
    std::vector<uint32_t> sizes(n_vec);
    DevBuf<short> d_q;
    DevBuf<uint8_t> d_slots;
    DevBuf<uint32_t> d_sizes;
    QuiesceOnExit quiesce(c);
    if (!d_q.alloc(n_vec * 1024) || !d_slots.alloc(n_vec * 2080) || !d_sizes.alloc(n_vec)) return fail(c, FLO_ERR_DEVICE, "flo_sparse_pack failed");
    hipError_t e = hipMemcpyAsync(d_q.p, q, n_vec * 2048, hipMemcpyHostToDevice, c->stream);
    int lrc = 0;
    if (e == hipSuccess) e = stream_delay(c->stream);
    if (e == hipSuccess) lrc = launch_sparse_only(d_q.p, n_vec, d_slots.p, d_sizes.p, form, c->stream);
    if (e == hipSuccess && lrc == 0) e = hipMemcpyAsync(slots.data(), d_slots.p, slots.size(), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && lrc == 0) e = hipMemcpyAsync(sizes.data(), d_sizes.p, n_vec * 4, hipMemcpyDeviceToHost, c->stream);
    hipError_t e2 = hipStreamSynchronize(c->stream);
    if (e != hipSuccess || e2 != hipSuccess || lrc != 0) return fail(c, FLO_ERR_DEVICE, "flo_sparse_pack failed");
    size_t pos = 0;
    for (size_t i = 0; i < n_vec; i++) {
        if (pos + sizes[i] > out_cap) return fail(c, FLO_ERR_ARG, "output buffer too small");
        memcpy(out + pos, slots.data() + i * 2080, sizes[i]);
        pos += sizes[i];
        out_off[i + 1] = (uint32_t)pos;
    }
    return FLO_OK;
}
