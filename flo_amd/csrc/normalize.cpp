// normalize.cpp — loudness normalisation and true-peak limiting on the device (flo_batch_true_peak, flo_normalize_gain,
// flo_normalize_lookahead, flo_batch_normalize, flo_normalize): a resident batch becomes a resident batch at a target
// loudness under a true-peak ceiling. Host code only: the gain, the look-ahead and the geometry are normalize_plan.cpp,
// the kernels normalize_kernels.hip. The integrated loudness is the batched analysis pass's (flo_batch_analyze_all), called
// as it is: its K-weighting shares its launches with the fingerprint and the waveform peaks.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "batch_internal.hpp"
#include "clip_tiles.hpp"
#include "devmem.hpp"
#include "normalize_kernels.hpp"
#include "normalize_plan.hpp"

extern "C" int flo_normalize_lookahead(uint32_t rate, const flo_normalize_opts *opts, uint32_t *frames, char *err, size_t err_cap) {
    std::string m;
    uint32_t a = 0;
    if (!frames) return FLO_ERR_ARG;
    if (!normalize_lookahead(rate, opts ? opts->lookahead_frames : 0, a, m)) {
        put_err(err, err_cap, m);
        return FLO_ERR_ARG;
    }
    *frames = a;
    return FLO_OK;
}

extern "C" int flo_normalize_gain(double integrated_lufs, double sample_peak_dbfs, float true_peak_linear, const flo_normalize_opts *opts,
                                  flo_normalize_report *report, char *err, size_t err_cap) {
    flo_normalize_opts o;
    std::string m;
    if (!report) return FLO_ERR_ARG;
    if (!normalize_opts(opts, o, m)) {
        put_err(err, err_cap, m);
        return FLO_ERR_ARG;
    }
    normalize_gain(integrated_lufs, sample_peak_dbfs, true_peak_linear, o, *report);
    return FLO_OK;
}

// The lists of one launch over n clips, laid out in one block that goes up in one copy: the table, the 64-bit lists, then
// the 32-bit ones. `res` .. end of the block is what the kernels write (limited | min_q | peak_bits) and comes back.
struct NormLists {
    BlockLayout B;
    const size_t n, o_table, o_src, o_dst, o_frames, o_pre, o_gain, o_copy, o_limited, o_minq, o_peak, bytes;   // (taken in this order)
    std::vector<uint8_t> host;
    explicit NormLists(size_t n_clips)
        : n(n_clips), o_table(B.take(kNormPhases * kNormTaps * 4)), o_src(B.take(n * 8)), o_dst(B.take(n * 8)), o_frames(B.take(n * 8)),
          o_pre(B.take((n + 1) * 4)), o_gain(B.take(n * 4)), o_copy(B.take(n * 4)), o_limited(B.take(n * 8)), o_minq(B.take(n * 4)),
          o_peak(B.take(n * 4)), bytes(B.bytes), host(bytes, 0) {}
    template <class T>
    T *at(size_t off) {
        return BlockLayout::at<T>(host.data(), off);
    }
    void point(NormArgs &a, uint8_t *dev) const {
        a.table = BlockLayout::at<const float>(dev, o_table);
        a.src_off = BlockLayout::at<const unsigned long long>(dev, o_src);
        a.dst_off = BlockLayout::at<const unsigned long long>(dev, o_dst);
        a.frames = BlockLayout::at<const unsigned long long>(dev, o_frames);
        a.pre = BlockLayout::at<const unsigned int>(dev, o_pre);
        a.gain = BlockLayout::at<const float>(dev, o_gain);
        a.copy = BlockLayout::at<const unsigned int>(dev, o_copy);
        a.limited = BlockLayout::at<unsigned long long>(dev, o_limited);
        a.min_q = BlockLayout::at<unsigned int>(dev, o_minq);
        a.peak_bits = BlockLayout::at<unsigned int>(dev, o_peak);
        a.n_clips = (unsigned)n;
    }
};

// linear[i] = the 4x oversampled peak of clip i: frames[i] sample-frames of ch channels at d_pcm + off[i]. Synchronous.
static int norm_peaks(flo_ctx *c, const float *d_pcm, const std::vector<uint64_t> &off, const std::vector<uint64_t> &frames, uint8_t ch,
                      std::vector<float> &linear) {
    const size_t n = frames.size();
    linear.assign(n, 0.f);
    std::vector<uint32_t> pre;
    if (!clip_tiles(frames.data(), n, norm_tile_frames(0), pre)) return fail(c, FLO_ERR_ARG, "too many tiles for one true-peak launch");
    if (!pre[n]) return FLO_OK;
    NormLists Ls(n);   // (outlives the stream: destroyed behind `quiesce`)
    const std::vector<float> h = normalize_table();
    memcpy(Ls.at<float>(Ls.o_table), h.data(), h.size() * 4);
    memcpy(Ls.at<uint64_t>(Ls.o_src), off.data(), n * 8);
    memcpy(Ls.at<uint64_t>(Ls.o_frames), frames.data(), n * 8);
    memcpy(Ls.at<uint32_t>(Ls.o_pre), pre.data(), (n + 1) * 4);
    DevBuf<uint8_t> dev;
    QuiesceOnExit quiesce(c);
    if (!dev.alloc(Ls.bytes)) return fail(c, FLO_ERR_NOMEM, "true peak work list: device memory");
    HIPCHK(c, hipMemcpyAsync(dev.p, Ls.host.data(), Ls.bytes, hipMemcpyHostToDevice, c->stream));
    NormArgs A;
    A.src = d_pcm;
    A.channels = ch;
    Ls.point(A, dev.p);
    int rc = timed_launch(c, "norm_peak", [&] { return launch_norm_peak(A, pre[n], c->stream); });
    if (rc != FLO_OK) return rc;
    std::vector<uint32_t> bits(n);
    HIPCHK(c, hipMemcpyAsync(bits.data(), dev.p + Ls.o_peak, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < n; i++) {
        const uint32_t v = bits[i] > 0x7F800000u ? 0x7FC00000u : bits[i];   // any NaN: the one quiet NaN
        memcpy(&linear[i], &v, 4);
    }
    return FLO_OK;
}

extern "C" int flo_batch_true_peak(flo_batch *b, float *linear) {
    if (!b || (!linear && b->n_clips)) return FLO_ERR_ARG;
    flo_ctx *c = b->ctx;
    if (!b->n_clips) return FLO_OK;
    if (!b->pcm_written) return batch_no_pcm(b, "flo_batch_true_peak");
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<float> out;
    int rc = norm_peaks(c, b->d_pcm, b->clip_off, batch_whole_frames(b), b->ch, out);
    if (rc != FLO_OK) return rc;
    memcpy(linear, out.data(), b->n_clips * sizeof(float));
    return FLO_OK;
}

static bool norm_no_skip() {
    const char *e = getenv("FLO_NORM_NO_SKIP");
    return e && *e && strcmp(e, "0") != 0;
}

extern "C" int flo_batch_normalize(flo_batch *src, const flo_normalize_opts *opts, flo_batch **out, flo_normalize_report *reports) {
    if (!src || !out) return FLO_ERR_ARG;
    *out = nullptr;
    flo_ctx *c = src->ctx;
    flo_normalize_opts o;
    std::string m;
    uint32_t la = 0;
    if (!normalize_opts(opts, o, m) || !normalize_lookahead(src->sr, o.lookahead_frames, la, m)) return fail(c, FLO_ERR_ARG, "flo_batch_normalize: " + m);
    const size_t n = src->n_clips;
    const uint8_t ch = src->ch;
    if (n && !src->pcm_written) return batch_no_pcm(src, "flo_batch_normalize");
    HIPCHK(c, hipSetDevice(c->device));
    const std::vector<uint64_t> frames = batch_whole_frames(src);
    std::vector<size_t> n_il(n);
    for (size_t i = 0; i < n; i++) n_il[i] = (size_t)(frames[i] * ch);
    // the measurements: loudness and sample peak of every clip from the batched analysis, the true peak from the envelope
    std::vector<flo_analysis> an(n ? n : 1);
    std::vector<float> tp;
    if (n) {
        std::vector<uint64_t> peak_off(n + 1);
        int rc = flo_batch_analyze_all(src, 50, nullptr, nullptr, 0, peak_off.data());
        if (rc != FLO_OK) return rc;
        std::vector<float> wave_peaks(peak_off[n] ? peak_off[n] : 1);
        rc = flo_batch_analyze_all(src, 50, an.data(), wave_peaks.data(), wave_peaks.size(), peak_off.data());
        if (rc != FLO_OK) return rc;
        rc = norm_peaks(c, src->d_pcm, src->clip_off, frames, ch, tp);
        if (rc != FLO_OK) return rc;
    }
    std::vector<flo_normalize_report> rep(n);
    for (size_t i = 0; i < n; i++) normalize_gain(an[i].integrated_lufs, an[i].sample_peak_dbfs, tp[i], o, rep[i]);

    BatchHold made;
    int rc = batch_derive(src, n, n_il.data(), src->sr, ch, &made.b);
    if (rc != FLO_OK) return rc;
    flo_batch *b = made.b;
    const bool limit = o.mode == FLO_NORM_LIMIT;
    std::vector<uint32_t> pre;
    if (!clip_tiles(frames.data(), n, norm_tile_frames(limit ? la : 0), pre)) return fail(c, FLO_ERR_ARG, "flo_batch_normalize: too many tiles for one launch");
    if (n && pre[n]) {
        NormLists Ls(n);   // (outlives the stream: destroyed behind `quiesce`)
        const std::vector<float> h = normalize_table();
        memcpy(Ls.at<float>(Ls.o_table), h.data(), h.size() * 4);
        memcpy(Ls.at<uint64_t>(Ls.o_src), src->clip_off.data(), n * 8);
        memcpy(Ls.at<uint64_t>(Ls.o_dst), b->clip_off.data(), n * 8);
        memcpy(Ls.at<uint64_t>(Ls.o_frames), frames.data(), n * 8);
        memcpy(Ls.at<uint32_t>(Ls.o_pre), pre.data(), (n + 1) * 4);
        for (size_t i = 0; i < n; i++) {
            Ls.at<float>(Ls.o_gain)[i] = rep[i].gain;
            Ls.at<uint32_t>(Ls.o_copy)[i] = rep[i].status ? 1u : 0u;
            Ls.at<uint32_t>(Ls.o_minq)[i] = kNormUnity;
        }
        DevBuf<uint8_t> dev;
        QuiesceOnExit quiesce(c);
        if (!dev.alloc(Ls.bytes)) return fail(c, FLO_ERR_NOMEM, "flo_batch_normalize: device memory");
        hipError_t e = hipMemcpyAsync(dev.p, Ls.host.data(), Ls.bytes, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) return fail(c, FLO_ERR_DEVICE, std::string("hipMemcpyAsync: ") + hipGetErrorString(e));
        NormArgs A;
        A.src = src->d_pcm;
        A.dst = b->d_pcm;
        A.channels = ch;
        A.lookahead = la;
        A.no_skip = norm_no_skip() ? 1u : 0u;
        A.ceiling = normalize_ceiling(o);
        A.bound = normalize_skip_bound(h);
        Ls.point(A, dev.p);
        rc = limit ? timed_launch(c, "norm_limit", [&] { return launch_norm_limit(A, pre[n], c->stream); })
                   : timed_launch(c, "norm_gain", [&] { return launch_norm_gain(A, pre[n], c->stream); });
        if (rc != FLO_OK) return rc;
        std::vector<uint64_t> limited(n, 0);
        std::vector<uint32_t> minq(n, kNormUnity);
        if (limit) {
            e = hipMemcpyAsync(limited.data(), dev.p + Ls.o_limited, n * 8, hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(minq.data(), dev.p + Ls.o_minq, n * 4, hipMemcpyDeviceToHost, c->stream);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return fail(c, FLO_ERR_DEVICE, std::string("flo_batch_normalize: ") + hipGetErrorString(e));
        for (size_t i = 0; i < n; i++) {
            rep[i].limited_frames = limited[i];
            rep[i].min_gain_q24 = minq[i];
        }
    }
    if (reports && n) memcpy(reports, rep.data(), n * sizeof(flo_normalize_report));
    b->pcm_written = true;
    *out = made.release();
    return FLO_OK;
}

extern "C" int flo_normalize(flo_ctx *c, const float *pcm, size_t n_interleaved, uint32_t sample_rate, uint8_t channels,
                             const flo_normalize_opts *opts, float **out, flo_normalize_report *report) {
    if (!c || !out || (!pcm && n_interleaved)) return FLO_ERR_ARG;
    *out = nullptr;
    if (channels < 1 || channels > 8) return fail(c, FLO_ERR_ARG, "flo_normalize: 1 to 8 channels");
    if (!sample_rate) return fail(c, FLO_ERR_ARG, "flo_normalize: sample_rate must be non-zero");
    return batch_one_shot(c, "flo_normalize", pcm, n_interleaved / channels * channels, sample_rate, channels,
                          [&](flo_batch *a, flo_batch **b) { return flo_batch_normalize(a, opts, b, report); }, out, nullptr);
}
