// convolve.cpp — FIR filtering and convolution on the device (flo_batch_convolve, flo_convolve): the clips of a resident
// batch filtered by clips of another resident batch into the clips of a new one, every output clip in one launch.
// Host code only: the checks, the taps of a job and the geometry are conv_plan.cpp, the kernel conv_kernels.hip, the
// filter design fir_design.cpp.
#include <cstdlib>
#include <cstring>
#include <memory>

#include "batch_internal.hpp"
#include "clip_tiles.hpp"
#include "conv_kernels.hpp"
#include "conv_plan.hpp"

static ConvSource conv_source(const flo_batch *b, const std::vector<uint64_t> &frames) {
    ConvSource s;
    if (!b) return s;
    s.present = true;
    s.ctx = b->ctx;
    s.rate = b->sr;
    s.channels = b->ch;
    s.n_clips = b->n_clips;
    s.clip_frames = frames.data();
    return s;
}

extern "C" int flo_batch_convolve(flo_batch *src, flo_batch *irs, size_t n_out, const flo_conv_job *jobs, flo_batch **out) {
    if (!out) return FLO_ERR_ARG;
    *out = nullptr;
    flo_ctx *c = src ? src->ctx : irs ? irs->ctx : nullptr;   // the first batch there is carries the message
    if (!c) return FLO_ERR_ARG;
    const std::vector<uint64_t> n_src = src ? batch_whole_frames(src) : std::vector<uint64_t>(),
                                n_ir = irs ? batch_whole_frames(irs) : std::vector<uint64_t>();
    std::vector<uint32_t> K, pre;
    std::string m;
    if (!conv_check(conv_source(src, n_src), conv_source(irs, n_ir), n_out, jobs, K, pre, m)) return fail(c, FLO_ERR_ARG, "flo_batch_convolve: " + m);
    if (n_out && !src->pcm_written) return batch_no_pcm(src, "flo_batch_convolve");
    if (n_out && !irs->pcm_written) return batch_no_pcm(irs, "flo_batch_convolve");
    const uint8_t ch = src->ch;
    std::vector<size_t> n_il(n_out);
    for (size_t k = 0; k < n_out; k++) n_il[k] = (size_t)(jobs[k].frames * ch);
    BatchHold made;
    int rc = batch_derive(src, n_out, n_il.data(), src->sr, ch, &made.b);
    if (rc != FLO_OK) return rc;
    flo_batch *b = made.b;
    if (n_out && pre[n_out]) {
        hipError_t e = hipSetDevice(c->device);
        if (e != hipSuccess) return fail(c, FLO_ERR_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));
        // jobs | pre: up through pinned memory into a pool block, both the new batch's until it goes. Every byte the kernel
        // reads is written here first (the unused words of a job included)
        BlockLayout B;
        const size_t o_jobs = B.take(n_out * sizeof(ConvJob)), o_pre = B.take((n_out + 1) * 4);
        rc = work_block_get(c, B.bytes, "flo_batch_convolve: work list", b->pin_work, b->d_work);
        if (rc != FLO_OK) return rc;
        void *const host = b->pin_work, *const dev = b->d_work;
        ConvJob *hj = B.at<ConvJob>(host, o_jobs);
        for (size_t k = 0; k < n_out; k++) {
            const flo_conv_job &g = jobs[k];
            ConvJob j{};
            j.src = src->d_pcm + src->clip_off[g.clip];
            // (ir_start at or beyond P: K is 0 and the pointer is never read; it stays inside the clip all the same)
            j.ir = irs->d_pcm + irs->clip_off[g.ir] + (g.ir_start < n_ir[g.ir] ? g.ir_start : 0) * irs->ch;
            j.n_src = n_src[g.clip];
            j.skip = conv_skip(g.skip, j.n_src, K[k]);
            j.frames = g.frames;
            j.dst_off = b->clip_off[k];
            j.taps = K[k];
            j.ir_channels = irs->ch;
            hj[k] = j;
        }
        memcpy(B.at<uint32_t>(host, o_pre), pre.data(), (n_out + 1) * 4);
        e = hipMemcpyAsync(dev, host, B.bytes, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) return fail(c, FLO_ERR_DEVICE, std::string("hipMemcpyAsync: ") + hipGetErrorString(e));
        ConvArgs A;
        A.dst = b->d_pcm;
        A.jobs = B.at<const ConvJob>(dev, o_jobs);
        A.pre = B.at<const unsigned int>(dev, o_pre);
        A.n_out = (unsigned)n_out;
        A.channels = ch;
        rc = timed_launch(c, "convolve", [&] { return launch_convolve(A, pre[n_out], irs->ch, c->stream); });
        if (rc != FLO_OK) return rc;
    }
    b->pcm_written = true;
    *out = made.release();
    return FLO_OK;
}

int conv_one_clip(flo_ctx *c, const std::string &who, const std::string &batch_who, ConvBatchOp op, const float *pcm, size_t n_interleaved,
                  const float *ir, size_t ir_interleaved, uint32_t sample_rate, uint8_t channels, uint8_t ir_channels, const flo_conv_job *job,
                  float **out, size_t *n_out) {
    if (!c || !out || !n_out || (n_interleaved && !pcm) || (ir_interleaved && !ir)) return FLO_ERR_ARG;
    *out = nullptr;
    *n_out = 0;
    if (channels < 1) return fail(c, FLO_ERR_ARG, who + ": channels must be at least 1");
    if (ir_channels < 1) return fail(c, FLO_ERR_ARG, who + ": ir_channels must be at least 1");
    if (!sample_rate) return fail(c, FLO_ERR_ARG, who + ": sample_rate must be non-zero");
    if (!job) return fail(c, FLO_ERR_ARG, who + ": job is NULL");
    if (job->clip != 0) return fail(c, FLO_ERR_ARG, who + ": clip " + std::to_string(job->clip) + " is not 0: there is one clip");
    if (job->ir != 0) return fail(c, FLO_ERR_ARG, who + ": ir " + std::to_string(job->ir) + " is not 0: there is one response");
    const size_t len = n_interleaved / channels * channels, ir_len = ir_interleaved / ir_channels * ir_channels;
    std::unique_ptr<float, decltype(&free)> res(nullptr, free);   // (freed behind the batches, whose destruction waits for the stream)
    BatchHold a, h, b;                                            // (b goes first)
    int rc = flo_batch_create(c, FLO_MODE_LOSSLESS, 1, &len, sample_rate, channels, 0, &a.b);
    if (rc != FLO_OK) return rc;
    rc = flo_batch_create(c, FLO_MODE_LOSSLESS, 1, &ir_len, sample_rate, ir_channels, 0, &h.b);
    if (rc != FLO_OK) return rc;
    rc = batch_upload_all(a.b, &pcm);
    if (rc != FLO_OK) return rc;
    rc = batch_upload_all(h.b, &ir);
    if (rc != FLO_OK) return rc;
    rc = op(a.b, h.b, 1, job, &b.b);
    if (rc != FLO_OK) {
        const std::string msg = c->err, from = batch_who + ": ";   // "flo_batch_convolve: ..." reads "flo_convolve: ..." here
        if (msg.compare(0, from.size(), from) == 0) fail(c, rc, who + ": " + msg.substr(from.size()));
        return rc;
    }
    const size_t floats = b.b->n_il[0];
    res.reset((float *)malloc(floats ? floats * sizeof(float) : 1));
    if (!res) return fail(c, FLO_ERR_NOMEM, "out of memory");
    if (floats) {
        hipError_t e = hipMemcpyAsync(res.get(), b.b->d_pcm + b.b->clip_off[0], floats * sizeof(float), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return fail(c, FLO_ERR_DEVICE, who + ": " + hipGetErrorString(e));
    }
    *out = res.release();
    *n_out = floats;
    return FLO_OK;
}

extern "C" int flo_convolve(flo_ctx *c, const float *pcm, size_t n_interleaved, const float *ir, size_t ir_interleaved, uint32_t sample_rate,
                            uint8_t channels, uint8_t ir_channels, const flo_conv_job *job, float **out, size_t *n_out) {
    return conv_one_clip(c, "flo_convolve", "flo_batch_convolve", flo_batch_convolve, pcm, n_interleaved, ir, ir_interleaved, sample_rate, channels,
                         ir_channels, job, out, n_out);
}
