// fftconv.cpp — partitioned FFT convolution on the device (flo_batch_convolve_fft, flo_convolve_fft): the jobs of
// flo_batch_convolve for long responses. Host code only: the checks, the responses, the groups and the work lists are
// fftconv_plan.cpp, the kernels fftconv_kernels.hip.
//
// One call: every distinct response is transformed once (fftconv_ir); then, group by group, the segments of the group's
// entries are transformed (fftconv_fwd) and multiplied, accumulated and transformed back (fftconv_mac). The groups share one
// scratch block, which stream order hands from one to the next. The twiddles and every group's lists go up in one work block
// that the new batch owns; the spectra are pool blocks of this call, and the stream is idle when they go back.
#include <cstdlib>
#include <cstring>

#include "batch_internal.hpp"
#include "clip_tiles.hpp"
#include "devmem.hpp"
#include "fftconv_kernels.hpp"
#include "fftconv_plan.hpp"

static ConvSource fc_source(const flo_batch *b, const std::vector<uint64_t> &frames) {
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

// a group's segment spectra stay under this many bytes (read per call; results do not depend on it)
static uint64_t fc_group_bytes() {
    const char *e = getenv("FLO_CONV_FFT_GROUP_BYTES");
    const long long v = e ? atoll(e) : 0;
    return v > 0 ? (uint64_t)v : kFcGroupBytes;
}

extern "C" int flo_batch_convolve_fft(flo_batch *src, flo_batch *irs, size_t n_out, const flo_conv_job *jobs, flo_batch **out) {
    if (!out) return FLO_ERR_ARG;
    *out = nullptr;
    flo_ctx *c = src ? src->ctx : irs ? irs->ctx : nullptr;   // the first batch there is carries the message
    if (!c) return FLO_ERR_ARG;
    const std::vector<uint64_t> n_src = src ? batch_whole_frames(src) : std::vector<uint64_t>(),
                                n_ir = irs ? batch_whole_frames(irs) : std::vector<uint64_t>();
    FcPlan P;
    std::string m;
    if (!fftconv_plan(fc_source(src, n_src), fc_source(irs, n_ir), n_out, jobs, fc_group_bytes(), P, m))
        return fail(c, FLO_ERR_ARG, "flo_batch_convolve_fft: " + m);
    if (n_out && !src->pcm_written) return batch_no_pcm(src, "flo_batch_convolve_fft");
    if (n_out && !irs->pcm_written) return batch_no_pcm(irs, "flo_batch_convolve_fft");
    const uint8_t ch = src->ch;
    std::vector<size_t> n_il(n_out);
    for (size_t k = 0; k < n_out; k++) n_il[k] = (size_t)(jobs[k].frames * ch);
    BatchHold made;
    int rc = batch_derive(src, n_out, n_il.data(), src->sr, ch, &made.b);
    if (rc != FLO_OK) return rc;
    flo_batch *b = made.b;
    if (!P.groups.empty()) {
        hipError_t e = hipSetDevice(c->device);
        if (e != hipSuccess) return fail(c, FLO_ERR_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));
        DevMem d_h, d_x;
        QuiesceOnExit idle(c);
        if ((e = pool_alloc(&d_h.p, P.h_elems ? P.h_elems * 8 : 16)) != hipSuccess || (e = pool_alloc(&d_x.p, P.x_elems ? P.x_elems * 8 : 16)) != hipSuccess)
            return fail(c, e == hipErrorOutOfMemory ? FLO_ERR_NOMEM : FLO_ERR_DEVICE, std::string("flo_batch_convolve_fft: spectra: ") + hipGetErrorString(e));

        // twiddles | response jobs | their prefix | per group: segment jobs | prefix | multiply jobs | prefix. Every byte the
        // kernels read is written here first (the unused words of a job included)
        struct Lists {
            size_t o_spec = 0, o_pre_spec = 0, o_mac = 0, o_pre_mac = 0;
            std::vector<uint32_t> pre_spec, pre_mac;
        };
        std::vector<float> tw;
        fftconv_twiddles(tw);
        std::vector<uint32_t> pre_ir;
        fftconv_response_tiles(P, pre_ir);   // (the plan has checked that they fit)
        BlockLayout B;
        const size_t n_resp = P.responses.size();
        const size_t o_tw = B.take(tw.size() * 4), o_ir = B.take(n_resp * sizeof(FcSpecJob)), o_pre_ir = B.take((n_resp + 1) * 4);
        std::vector<Lists> L(P.groups.size());
        for (size_t g = 0; g < P.groups.size(); g++) {
            const size_t n = P.groups[g].count;
            fftconv_group_tiles(P, P.groups[g], L[g].pre_spec, L[g].pre_mac);
            L[g].o_spec = B.take(n * sizeof(FcSpecJob));
            L[g].o_pre_spec = B.take((n + 1) * 4);
            L[g].o_mac = B.take(n * sizeof(FcMacJob));
            L[g].o_pre_mac = B.take((n + 1) * 4);
        }
        rc = work_block_get(c, B.bytes, "flo_batch_convolve_fft: work list", b->pin_work, b->d_work);
        if (rc != FLO_OK) return rc;
        void *const host = b->pin_work, *const dev = b->d_work;
        memcpy(B.at<float>(host, o_tw), tw.data(), tw.size() * 4);
        FcSpecJob *hr = B.at<FcSpecJob>(host, o_ir);
        for (size_t r = 0; r < n_resp; r++) {
            const FcResponse &R = P.responses[r];
            FcSpecJob j{};
            j.base = irs->d_pcm + irs->clip_off[R.ir] + R.ir_start * irs->ch;   // (inside the clip: ir_start < P unless K == 0)
            j.start = 0;
            j.len = R.taps;
            j.out = R.h_off;
            j.channels = irs->ch;
            j.live = kFcBlock;
            j.items = R.parts * irs->ch;
            hr[r] = j;
        }
        memcpy(B.at<uint32_t>(host, o_pre_ir), pre_ir.data(), (n_resp + 1) * 4);
        for (size_t g = 0; g < P.groups.size(); g++) {
            const FcGroup &G = P.groups[g];
            FcSpecJob *hs = B.at<FcSpecJob>(host, L[g].o_spec);
            FcMacJob *hm = B.at<FcMacJob>(host, L[g].o_mac);
            for (size_t i = 0; i < G.count; i++) {
                const FcEntry &E = P.entries[G.first + i];
                const FcJob &J = P.jobs[E.job];
                const flo_conv_job &u = jobs[E.job];
                FcSpecJob s{};
                s.base = src->d_pcm + src->clip_off[u.clip];
                s.start = (E.s0 - 1) * (long long)kFcBlock + (long long)J.skip;
                s.len = n_src[u.clip];
                s.out = E.x_off;
                s.channels = ch;
                s.live = 2 * kFcBlock;
                s.items = (unsigned)((uint64_t)(E.s1 - E.s0) * ch);
                hs[i] = s;
                FcMacJob q{};
                q.x_off = E.x_off;
                q.h_off = P.responses[J.response].h_off;
                q.dst_off = b->clip_off[E.job];
                q.frames = u.frames;
                q.s0 = E.s0;
                q.s1 = E.s1;
                q.b0 = E.b0;
                q.parts = J.parts;
                q.ir_channels = irs->ch;
                hm[i] = q;
            }
            memcpy(B.at<uint32_t>(host, L[g].o_pre_spec), L[g].pre_spec.data(), (G.count + 1) * 4);
            memcpy(B.at<uint32_t>(host, L[g].o_pre_mac), L[g].pre_mac.data(), (G.count + 1) * 4);
        }
        e = hipMemcpyAsync(dev, host, B.bytes, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) return fail(c, FLO_ERR_DEVICE, std::string("hipMemcpyAsync: ") + hipGetErrorString(e));

        const float2 *const d_tw = B.at<const float2>(dev, o_tw);
        FcSpecArgs S;
        S.out = d_h.as<float2>();
        S.jobs = B.at<const FcSpecJob>(dev, o_ir);
        S.pre = B.at<const unsigned int>(dev, o_pre_ir);
        S.tw = d_tw;
        S.n_jobs = (unsigned)n_resp;
        if (pre_ir[n_resp]) {
            rc = timed_launch(c, "fftconv_ir", [&] { return launch_fftconv_spectra(S, pre_ir[n_resp], c->stream); });
            if (rc != FLO_OK) return rc;
        }
        for (size_t g = 0; g < P.groups.size(); g++) {
            const unsigned n = (unsigned)P.groups[g].count;
            S.out = d_x.as<float2>();
            S.jobs = B.at<const FcSpecJob>(dev, L[g].o_spec);
            S.pre = B.at<const unsigned int>(dev, L[g].o_pre_spec);
            S.n_jobs = n;
            if (L[g].pre_spec[n]) {
                rc = timed_launch(c, "fftconv_fwd", [&] { return launch_fftconv_spectra(S, L[g].pre_spec[n], c->stream); });
                if (rc != FLO_OK) return rc;
            }
            FcMacArgs A;
            A.dst = b->d_pcm;
            A.x = d_x.as<float2>();
            A.h = d_h.as<float2>();
            A.tw = d_tw;
            A.jobs = B.at<const FcMacJob>(dev, L[g].o_mac);
            A.pre = B.at<const unsigned int>(dev, L[g].o_pre_mac);
            A.n_jobs = n;
            A.channels = ch;
            if (L[g].pre_mac[n]) {
                rc = timed_launch(c, "fftconv_mac", [&] { return launch_fftconv_mac(A, L[g].pre_mac[n], c->stream); });
                if (rc != FLO_OK) return rc;
            }
        }
        e = hipStreamSynchronize(c->stream);   // the spectra go back to the pool on the way out
        if (e != hipSuccess) return fail(c, FLO_ERR_DEVICE, std::string("flo_batch_convolve_fft: ") + hipGetErrorString(e));
    }
    b->pcm_written = true;
    *out = made.release();
    return FLO_OK;
}

extern "C" int flo_convolve_fft(flo_ctx *c, const float *pcm, size_t n_interleaved, const float *ir, size_t ir_interleaved, uint32_t sample_rate,
                                uint8_t channels, uint8_t ir_channels, const flo_conv_job *job, float **out, size_t *n_out) {
    return conv_one_clip(c, "flo_convolve_fft", "flo_batch_convolve_fft", flo_batch_convolve_fft, pcm, n_interleaved, ir, ir_interleaved, sample_rate,
                         channels, ir_channels, job, out, n_out);
}
