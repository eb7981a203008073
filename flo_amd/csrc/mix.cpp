// mix.cpp — mixing and concatenation on the device (flo_batch_mix, flo_mix): parts of the clips of several resident batches
// are summed into the clips of a new resident batch, every output clip in one launch.
// Host code only: the checks, the prefixes and the class of a part on a tile are mix_plan.cpp, the kernel mix_kernels.hip.
#include <cstdlib>
#include <cstring>
#include <memory>

#include "batch_internal.hpp"
#include "clip_tiles.hpp"
#include "mix_kernels.hpp"
#include "mix_plan.hpp"

extern "C" int flo_batch_mix(flo_batch *const *srcs, size_t n_srcs, size_t n_out, const uint64_t *out_frames, size_t n_parts,
                             const flo_mix_part *parts, flo_batch **out) {
    if (!out) return FLO_ERR_ARG;
    *out = nullptr;
    flo_ctx *c = nullptr;   // the first source there is carries the message
    for (size_t i = 0; srcs && i < n_srcs && !c; i++)
        if (srcs[i]) c = srcs[i]->ctx;
    if (!c) return FLO_ERR_ARG;
    std::vector<std::vector<uint64_t>> frames(n_srcs);
    std::vector<MixSource> S(n_srcs);
    for (size_t i = 0; i < n_srcs; i++) {
        const flo_batch *s = srcs[i];
        if (!s) continue;
        frames[i] = batch_whole_frames(s);
        S[i].present = true;
        S[i].ctx = s->ctx;
        S[i].rate = s->sr;
        S[i].channels = s->ch;
        S[i].n_clips = s->n_clips;
        S[i].clip_frames = frames[i].data();
    }
    std::vector<uint32_t> ppre, pre;
    std::string m;
    if (!mix_check(S.data(), n_srcs, n_out, out_frames, n_parts, parts, ppre, pre, m)) return fail(c, FLO_ERR_ARG, "flo_batch_mix: " + m);
    for (size_t i = 0; i < n_parts; i++)
        if (!srcs[parts[i].batch]->pcm_written) return batch_no_pcm(srcs[parts[i].batch], "flo_batch_mix");
    const flo_batch *first = srcs[0];
    const uint8_t ch = first->ch;
    std::vector<size_t> n_il(n_out);
    for (size_t k = 0; k < n_out; k++) n_il[k] = (size_t)(out_frames[k] * ch);
    BatchHold made;
    int rc = batch_derive(first, n_out, n_il.data(), first->sr, ch, &made.b);
    if (rc != FLO_OK) return rc;
    flo_batch *b = made.b;
    if (n_out && pre[n_out]) {
        hipError_t e = hipSetDevice(c->device);
        if (e != hipSuccess) return fail(c, FLO_ERR_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));
        // parts | clips | ppre | pre: up through pinned memory into a pool block, both the new batch's until it goes. Every
        // byte the kernel reads is written here first (the unused words of a part included)
        BlockLayout B;
        const size_t o_parts = B.take(n_parts * sizeof(MixPart)), o_clips = B.take(n_out * sizeof(MixClip)), o_ppre = B.take((n_out + 1) * 4),
                     o_pre = B.take((n_out + 1) * 4);
        rc = work_block_get(c, B.bytes, "flo_batch_mix: work list", b->pin_work, b->d_work);
        if (rc != FLO_OK) return rc;
        void *const host = b->pin_work, *const dev = b->d_work;
        MixPart *hp = B.at<MixPart>(host, o_parts);
        for (size_t i = 0; i < n_parts; i++) {
            const flo_mix_part &g = parts[i];
            const flo_batch *s = srcs[g.batch];
            MixPart p{};
            p.src = s->d_pcm + s->clip_off[g.clip];
            p.n_src = frames[g.batch][g.clip];
            p.start = g.start;
            p.frames = g.frames;
            p.at = g.at;
            p.fade_in = g.fade_in;
            p.fade_out = g.fade_out;
            p.gain = g.gain;
            hp[i] = p;
        }
        MixClip *hc = B.at<MixClip>(host, o_clips);
        for (size_t k = 0; k < n_out; k++) hc[k] = MixClip{b->clip_off[k], out_frames[k]};
        memcpy(B.at<uint32_t>(host, o_ppre), ppre.data(), (n_out + 1) * 4);
        memcpy(B.at<uint32_t>(host, o_pre), pre.data(), (n_out + 1) * 4);
        e = hipMemcpyAsync(dev, host, B.bytes, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) return fail(c, FLO_ERR_DEVICE, std::string("hipMemcpyAsync: ") + hipGetErrorString(e));
        MixArgs A;
        A.dst = b->d_pcm;
        A.parts = B.at<const MixPart>(dev, o_parts);
        A.clips = B.at<const MixClip>(dev, o_clips);
        A.ppre = B.at<const unsigned int>(dev, o_ppre);
        A.pre = B.at<const unsigned int>(dev, o_pre);
        A.n_out = (unsigned)n_out;
        A.channels = ch;
        rc = timed_launch(c, "mix", [&] { return launch_mix(A, pre[n_out], c->stream); });
        if (rc != FLO_OK) return rc;
    }
    b->pcm_written = true;
    *out = made.release();
    return FLO_OK;
}

extern "C" int flo_mix(flo_ctx *c, size_t n_clips, const float *const *pcm, const size_t *n_interleaved, uint32_t sample_rate,
                       uint8_t channels, size_t n_parts, const flo_mix_part *parts, uint64_t out_frames, float **out, size_t *n_out) {
    if (!c || !out || !n_out || (n_clips && (!pcm || !n_interleaved))) return FLO_ERR_ARG;
    *out = nullptr;
    *n_out = 0;
    for (size_t i = 0; i < n_clips; i++)
        if (n_interleaved[i] && !pcm[i]) return FLO_ERR_ARG;
    if (channels < 1) return fail(c, FLO_ERR_ARG, "flo_mix: channels must be at least 1");
    if (!sample_rate) return fail(c, FLO_ERR_ARG, "flo_mix: sample_rate must be non-zero");
    if (n_parts && !parts) return fail(c, FLO_ERR_ARG, "flo_mix: parts is NULL");
    for (size_t i = 0; i < n_parts; i++) {
        if (parts[i].batch != 0) return fail(c, FLO_ERR_ARG, "flo_mix: batch " + std::to_string(parts[i].batch) + " of part " + std::to_string(i) + " is not 0: the clips are one source");
        if (parts[i].out != 0) return fail(c, FLO_ERR_ARG, "flo_mix: out " + std::to_string(parts[i].out) + " of part " + std::to_string(i) + " is not 0: there is one output");
    }
    std::vector<size_t> lens(n_clips);
    for (size_t i = 0; i < n_clips; i++) lens[i] = n_interleaved[i] / channels * channels;
    std::unique_ptr<float, decltype(&free)> res(nullptr, free);   // (freed behind the batches, whose destruction waits for the stream)
    BatchHold a, b;                                               // (b goes first)
    int rc = flo_batch_create(c, FLO_MODE_LOSSLESS, n_clips, lens.data(), sample_rate, channels, 0, &a.b);
    if (rc != FLO_OK) return rc;
    rc = batch_upload_all(a.b, pcm);
    if (rc != FLO_OK) return rc;
    rc = flo_batch_mix(&a.b, 1, 1, &out_frames, n_parts, parts, &b.b);
    if (rc != FLO_OK) {
        const std::string msg = c->err, from = "flo_batch_mix: ";   // "flo_batch_mix: ..." reads "flo_mix: ..." here
        if (msg.compare(0, from.size(), from) == 0) fail(c, rc, "flo_mix: " + msg.substr(from.size()));
        return rc;
    }
    const size_t floats = b.b->n_il[0];
    res.reset((float *)malloc(floats ? floats * sizeof(float) : 1));
    if (!res) return fail(c, FLO_ERR_NOMEM, "out of memory");
    if (floats) {
        hipError_t e = hipMemcpyAsync(res.get(), b.b->d_pcm + b.b->clip_off[0], floats * sizeof(float), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return fail(c, FLO_ERR_DEVICE, std::string("flo_mix: ") + hipGetErrorString(e));
    }
    *out = res.release();
    *n_out = floats;
    return FLO_OK;
}
