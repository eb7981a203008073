// corpus.cpp — flo_corpus_*: many .flo files resident in HBM, short windows of their decoded signal decoded in batches.
//
// Once, at creation: every file parsed on the host (container.cpp, Reader::read's semantics and messages), all bytes
// uploaded into one device buffer, the frame tables built. Per call: O(windows) host work that writes one descriptor
// block into pinned staging, one copy of it, and the launches - all on the ctx stream, ordered against the caller's
// stream by events. Nothing synchronises the host in steady state: scratch only grows (the blocks it replaces are freed
// at the next flo_corpus_sync), and a staging slot is reused only once the copy out of it has completed.
//   lossy files:    lossy_decode_kernel<kDecWindow> (decode_kernels.hip): runs of blocks per window, trimmed to the window
//   lossless files: the frames a window touches (each window its own: a frame two windows share is decoded twice) go
//                   through the parallel Rice / predictor kernels (lldec_kernels.hip) on a per-call wrapper list, then
//                   ll_window_finish_kernel writes the window's part of each frame to the window's slot
//   every window:   window_tail_kernel writes the zeros past the end of its file
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "container.hpp"
#include "ctx_internal.hpp"
#include "decode_kernels.hpp"
#include "decode_plan.hpp"
#include "devpool.hpp"

namespace {
struct CorpusFile {
    bool lossy = false;
    uint64_t n_out = 0;     // flo_decode's length in sample-frames
    uint64_t frame0 = 0;    // lossy: first entry in the compacted blob list; lossless: first entry in ll_frames
    uint32_t n_frames = 0;  // lossy: compacted frames; lossless: frames
};
struct LlFrame {
    uint64_t start;         // first sample-frame of the frame in the file's decoded signal
    uint32_t samples;
    uint32_t first_wrapper; // into ll_wr
    uint32_t n_channels;
    uint32_t mid_side;
};
struct LlWrapper {
    LlChannelDev d;         // off: absolute in the corpus buffer; out_off filled per call
    LlRoute r;              // routed once, here
};
struct Grow {               // device scratch that only grows; replaced blocks wait for the next sync
    void *p = nullptr;
    size_t cap = 0;
};
}  // namespace

struct flo_corpus {
    flo_ctx *ctx = nullptr;
    uint32_t sample_rate = 0;
    uint8_t channels = 0;
    std::vector<CorpusFile> files;
    uint8_t *d_bytes = nullptr;
    TableSet *ts = nullptr;
    unsigned long long *d_blob_off = nullptr;
    unsigned int *d_blob_len = nullptr;
    int *d_err = nullptr;
    std::vector<LlFrame> ll_frames;
    std::vector<LlWrapper> ll_wr;
    Grow desc, scr, tabs, ent;
    std::vector<void *> retired;
    StageRing ring;
    // per-call host lists (kept: no allocation in steady state)
    std::vector<LossyWinDev> wins;
    std::vector<WinTailDev> tails;
    LlWrapperList ll;
    std::vector<LlWinItem> items;
};

static void corpus_free(flo_corpus *c) {
    if (c->ctx && c->ctx->stream) hipStreamSynchronize(c->ctx->stream);
    for (void *p : c->retired) pool_free(p);
    for (Grow *g : {&c->desc, &c->scr, &c->tabs, &c->ent})
        if (g->p) pool_free(g->p);
    for (void *p : {(void *)c->d_bytes, (void *)c->d_blob_off, (void *)c->d_blob_len, (void *)c->d_err})
        if (p) pool_free(p);
    delete c;
}

extern "C" void flo_corpus_destroy(flo_corpus *c) {
    if (c) corpus_free(c);
}

extern "C" int flo_corpus_create(flo_ctx *ctx, size_t n_files, const uint8_t *const *files, const size_t *lens, flo_corpus **out) {
    if (!ctx || !out || !n_files || !files || !lens) return fail(ctx, FLO_ERR_ARG, "null argument or empty corpus");
    *out = nullptr;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    flo_corpus *c = new flo_corpus();
    c->ctx = ctx;
    auto bail = [&](int rc) {
        corpus_free(c);
        return rc;
    };
    // parse every file; lay the bytes out back to back (16-byte aligned starts)
    std::vector<uint64_t> base(n_files);
    std::vector<unsigned long long> blob_off;
    std::vector<unsigned int> blob_len;
    uint64_t total = 0;
    bool any_lossy = false;
    for (size_t i = 0; i < n_files; i++) {
        if (!files[i] && lens[i]) return bail(fail(ctx, FLO_ERR_ARG, "null file"));
        ParsedFile f;
        const char *perr = "";
        if (parse_file(files[i], lens[i], f, &perr) != 0) return bail(fail(ctx, FLO_ERR_FORMAT, perr));
        if (i == 0) {
            c->sample_rate = f.sample_rate;
            c->channels = f.channels;
        } else if (f.sample_rate != c->sample_rate || f.channels != c->channels) {
            return bail(fail(ctx, FLO_ERR_ARG, "corpus files differ in sample rate or channel count (file " + std::to_string(i) + ")"));
        }
        if (f.channels == 0) return bail(fail(ctx, FLO_ERR_ARG, "corpus files have no channels"));
        base[i] = total;
        total += (lens[i] + 15) & ~(uint64_t)15;
        CorpusFile cf;
        cf.lossy = f.is_transform;
        if (f.is_transform) {   // decode_transform_file (lib.rs:325-352): the frames with channels, the first one dropped
            any_lossy = true;
            cf.frame0 = blob_off.size();
            for (const FrameDesc &fr : f.frames) {
                if (!fr.n_channels) continue;
                const ChannelDesc &cd = f.channels_desc[fr.first_channel];
                blob_off.push_back(base[i] + cd.off);
                blob_len.push_back(cd.len);
            }
            cf.n_frames = (uint32_t)(blob_off.size() - cf.frame0);
            cf.n_out = cf.n_frames > 1 ? (uint64_t)(cf.n_frames - 1) * 1024u : 0;
        } else {   // lossless/decoder.rs:21-72: every frame, its wrappers
            cf.frame0 = c->ll_frames.size();
            cf.n_frames = (uint32_t)f.frames.size();
            uint64_t at = 0;
            for (const FrameDesc &fr : f.frames) {
                LlFrame lf{at, fr.samples, (uint32_t)c->ll_wr.size(), fr.n_channels,
                           (f.channels == 2 && (fr.flags & 1)) ? 1u : 0u};
                for (unsigned k = 0; k < fr.n_channels; k++) {
                    const ChannelDesc &cd = f.channels_desc[fr.first_channel + k];
                    LlWrapper w{ll_channel(base[i] + cd.off, cd.len, cd.n_coeffs, cd.shift_bits, cd.rice_k, cd.coeffs), {}};
                    w.d.samples = fr.samples;
                    w.r = ll_route(w.d, false);
                    c->ll_wr.push_back(w);
                }
                c->ll_frames.push_back(lf);
                at += fr.samples;
            }
            cf.n_out = at;
        }
        c->files.push_back(cf);
    }
    // one device buffer for all bytes (+ slack: the lossy kernel prefetches up to three bytes past a blob), through the stager
    if (pool_alloc(&c->d_bytes, total + 32) != hipSuccess) return bail(fail(ctx, FLO_ERR_NOMEM, "corpus bytes"));
    int rc = ctx_stager(ctx);
    if (rc != FLO_OK) return bail(rc);
    {
        std::vector<UploadSeg> segs;
        for (size_t i = 0; i < n_files; i++)
            if (lens[i]) segs.push_back({c->d_bytes + base[i], files[i], lens[i]});
        std::string uerr;
        if (stager_upload(ctx->stager, segs, ctx->stream, uerr) != 0) return bail(fail(ctx, FLO_ERR_DEVICE, uerr));
    }
    if (any_lossy) {
        if ((rc = get_tables(ctx, c->sample_rate, 0.5f, &c->ts)) != FLO_OK) return bail(rc);
        const size_t nb = blob_off.size();
        if (pool_alloc(&c->d_blob_off, (nb ? nb : 1) * sizeof(unsigned long long)) != hipSuccess ||
            pool_alloc(&c->d_blob_len, (nb ? nb : 1) * sizeof(unsigned int)) != hipSuccess)
            return bail(fail(ctx, FLO_ERR_NOMEM, "corpus frame tables"));
        if (nb) {
            HIPCHK(ctx, hipMemcpyAsync(c->d_blob_off, blob_off.data(), nb * sizeof(unsigned long long), hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(ctx, hipMemcpyAsync(c->d_blob_len, blob_len.data(), nb * sizeof(unsigned int), hipMemcpyHostToDevice, ctx->stream));
        }
    }
    if (pool_alloc(&c->d_err, sizeof(int)) != hipSuccess) return bail(fail(ctx, FLO_ERR_NOMEM, "corpus error word"));
    HIPCHK(ctx, hipMemsetAsync(c->d_err, 0, sizeof(int), ctx->stream));
    if (!c->ring.init()) return bail(fail(ctx, FLO_ERR_DEVICE, "hipEventCreate failed"));
    // the host vectors blob_off / blob_len die with this frame
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return bail(fail(ctx, FLO_ERR_DEVICE, "corpus upload failed"));
    *out = c;
    return FLO_OK;
}

extern "C" int flo_corpus_format(const flo_corpus *c, uint32_t *sample_rate, uint8_t *channels) {
    if (!c) return FLO_ERR_ARG;
    if (sample_rate) *sample_rate = c->sample_rate;
    if (channels) *channels = c->channels;
    return FLO_OK;
}

extern "C" int flo_corpus_file_frames(const flo_corpus *c, size_t file, uint64_t *decoded_sample_frames) {
    if (!c || !decoded_sample_frames || file >= c->files.size()) return FLO_ERR_ARG;
    *decoded_sample_frames = c->files[file].n_out;
    return FLO_OK;
}

// make `g` hold at least `bytes`; the block it replaces may still be read by queued work: it is freed at the next sync
static int grow(flo_corpus *c, Grow &g, size_t bytes) {
    if (bytes <= g.cap) return FLO_OK;
    if (g.p) c->retired.push_back(g.p);
    g.p = nullptr;
    g.cap = 0;
    const size_t want = bytes + bytes / 4;
    if (pool_alloc(&g.p, want) != hipSuccess) return fail(c->ctx, FLO_ERR_NOMEM, "corpus scratch");
    g.cap = want;
    return FLO_OK;
}

extern "C" int flo_corpus_decode_windows(flo_corpus *c, size_t n_windows, const uint32_t *file, const uint64_t *start,
                                         uint32_t window_frames, float *dst_device, size_t dst_cap_floats, void *stream) {
    if (!c) return FLO_ERR_ARG;
    flo_ctx *ctx = c->ctx;
    if (!n_windows || !window_frames) return FLO_OK;
    if (!file || !start || !dst_device) return fail(ctx, FLO_ERR_ARG, "null argument");
    const uint64_t ch = c->channels, slot_floats = (uint64_t)window_frames * ch;
    if (dst_cap_floats / slot_floats < n_windows) return fail(ctx, FLO_ERR_ARG, "destination too small for the windows");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    c->wins.clear();
    c->tails.clear();
    c->ll.clear();
    c->items.clear();
    unsigned max_count = 0;
    for (size_t w = 0; w < n_windows; w++) {
        if (file[w] >= c->files.size()) return fail(ctx, FLO_ERR_ARG, "window file index out of range");
        const CorpusFile &F = c->files[file[w]];
        const uint64_t s = start[w], dst = (uint64_t)w * slot_floats;
        const uint64_t valid = s < F.n_out ? std::min<uint64_t>(window_frames, F.n_out - s) : 0;
        if (valid < window_frames) c->tails.push_back({dst, (unsigned)(valid * ch), (unsigned)slot_floats});
        if (!valid) continue;
        if (F.lossy) {
            c->wins.push_back({F.frame0, s, dst, F.n_frames, 0u});
            continue;
        }
        // the frames of [s, s + valid): the last one starting at or before s, and those behind it
        const LlFrame *fb = c->ll_frames.data() + F.frame0, *fe = fb + F.n_frames;
        const LlFrame *fr = std::upper_bound(fb, fe, s, [](uint64_t v, const LlFrame &x) { return v < x.start; }) - 1;
        for (; fr < fe && fr->start < s + valid; fr++) {
            if (!fr->samples) continue;
            const uint64_t a = std::max<uint64_t>(s, fr->start), b = std::min<uint64_t>(s + valid, fr->start + fr->samples);
            if (a >= b) continue;
            LlWinItem it{};
            it.dst = dst + (a - s) * ch;
            it.first_channel = (unsigned)c->ll.chs.size();
            it.n_channels = fr->n_channels;
            it.from = (unsigned)(a - fr->start);
            it.count = (unsigned)(b - a);
            it.mid_side = fr->mid_side;
            max_count = std::max(max_count, it.count);
            for (unsigned k = 0; k < fr->n_channels; k++) {
                const LlWrapper &x = c->ll_wr[fr->first_wrapper + k];
                c->ll.push(x.d, x.r);
            }
            c->items.push_back(it);
        }
    }
    // one descriptor block
    enum { kWin, kTail, kCh, kT0, kSer, kOth, kItem };
    const LlWrapperList &ll = c->ll;
    const DescBlock blk{desc_part(c->wins), desc_part(c->tails), desc_part(ll.chs), desc_part(ll.tile0),
                        desc_part(ll.serial), desc_part(ll.others), desc_part(c->items)};
    uint8_t *pin;
    int rc;
    if ((rc = c->ring.acquire(ctx, blk.bytes, &pin)) != FLO_OK) return rc;
    blk.fill(pin);
    if ((rc = grow(c, c->desc, blk.bytes)) != FLO_OK) return rc;
    if (!ll.chs.empty()) {
        const size_t tiles = ll.tiles();
        if ((rc = grow(c, c->scr, ll.scratch * sizeof(int))) != FLO_OK || (rc = grow(c, c->tabs, (tiles ? tiles : 1) * kRiceStates * sizeof(unsigned int))) != FLO_OK ||
            (rc = grow(c, c->ent, (tiles ? tiles : 1) * sizeof(uint2))) != FLO_OK)
            return rc;
    }
    hipStream_t us = (hipStream_t)stream, cs = ctx->stream;
    if ((rc = c->ring.fence_in(ctx, us)) != FLO_OK || (rc = c->ring.upload(ctx, c->desc.p, blk.bytes)) != FLO_OK) return rc;
    void *d = c->desc.p;
    if (!c->tails.empty()) {
        const WinTailDev *t = blk.at<const WinTailDev>(d, kTail);
        if ((rc = timed_launch(ctx, "window_tail", [&] { return launch_window_tail(t, (unsigned)c->tails.size(), dst_device, cs); })) != FLO_OK) return rc;
    }
    if (!c->wins.empty()) {
        const unsigned max_blocks = (window_frames - 1u) / 1024u + 2u;   // blocks a window of this length can touch
        const unsigned rpw = (max_blocks + 15u) / 16u, run = (max_blocks + rpw - 1u) / rpw;   // balanced runs of <= 16 blocks
        LossyDecArgs A{};
        A.T = c->ts->dev;
        A.window = c->ts->dev_window;
        A.bytes = c->d_bytes;
        A.blob_off = c->d_blob_off;
        A.blob_len = c->d_blob_len;
        A.channels = c->channels;
        A.out = dst_device;
        A.error = c->d_err;
        LossyWinArgs W{blk.at<const LossyWinDev>(d, kWin), (unsigned)c->wins.size(), rpw, window_frames};
        if ((rc = timed_launch(ctx, "lossy_window", [&] { return launch_lossy_window(A, W, run, cs); })) != FLO_OK) return rc;
    }
    if (!ll.chs.empty()) {
        const LlChannelDev *d_ch = blk.at<const LlChannelDev>(d, kCh);
        if ((rc = launch_ll_wrappers(ctx, ll, c->d_bytes, d_ch, blk.at<const unsigned int>(d, kT0), blk.at<int>(d, kSer),
                                     blk.at<const unsigned int>(d, kOth), (int *)c->scr.p, (unsigned int *)c->tabs.p, (uint2 *)c->ent.p,
                                     "window_ll_decode_parallel", "window_ll_decode")) != FLO_OK)
            return rc;
        LlWinFinishArgs F{blk.at<const LlWinItem>(d, kItem), d_ch, (unsigned)c->items.size(), (int)c->channels, (const int *)c->scr.p, dst_device};
        if ((rc = timed_launch(ctx, "window_ll_finish", [&] { return launch_ll_window_finish(F, max_count, cs); })) != FLO_OK) return rc;
    }
    return c->ring.fence_out(ctx, us);
}

extern "C" int flo_corpus_sync(flo_corpus *c) {
    if (!c) return FLO_ERR_ARG;
    flo_ctx *ctx = c->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int herr = 0;
    HIPCHK(ctx, hipMemcpyAsync(&herr, c->d_err, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (void *p : c->retired) pool_free(p);
    c->retired.clear();
    if (herr) {
        HIPCHK(ctx, hipMemsetAsync(c->d_err, 0, sizeof(int), ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        return fail(ctx, FLO_ERR_FORMAT, "Failed to deserialize transform frame");
    }
    return FLO_OK;
}
