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
#include <cstring>
#include <string>
#include <vector>

#include "container.hpp"
#include "ctx_internal.hpp"
#include "decode_kernels.hpp"
#include "devpool.hpp"

namespace {
constexpr int kStageSlots = 8;   // pinned descriptor slots in flight

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
    uint32_t tiles;         // Rice tiles of the parallel form (0: none, or serial)
    uint8_t serial, other;
};
struct Slot {
    void *pin = nullptr;
    size_t cap = 0;
    hipEvent_t ev = nullptr;
    bool used = false;
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
    Slot slots[kStageSlots];
    unsigned next_slot = 0;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    // per-call host lists (kept: no allocation in steady state)
    std::vector<LossyWinDev> wins;
    std::vector<WinTailDev> tails;
    std::vector<LlChannelDev> chs;
    std::vector<unsigned int> tile0, others;
    std::vector<int> serial;
    std::vector<LlWinItem> items;
};

static void corpus_free(flo_corpus *c) {
    if (c->ctx && c->ctx->stream) hipStreamSynchronize(c->ctx->stream);
    for (void *p : c->retired) pool_free(p);
    for (Grow *g : {&c->desc, &c->scr, &c->tabs, &c->ent})
        if (g->p) pool_free(g->p);
    for (void *p : {(void *)c->d_bytes, (void *)c->d_blob_off, (void *)c->d_blob_len, (void *)c->d_err})
        if (p) pool_free(p);
    for (Slot &s : c->slots) {
        if (s.ev) hipEventSynchronize(s.ev), hipEventDestroy(s.ev);
        if (s.pin) hipHostFree(s.pin);
    }
    if (c->ev_in) hipEventDestroy(c->ev_in);
    if (c->ev_out) hipEventDestroy(c->ev_out);
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
        } else {   // lossless/decoder.rs:21-72: every frame, its wrappers (as flo_decode's LlWork)
            cf.frame0 = c->ll_frames.size();
            cf.n_frames = (uint32_t)f.frames.size();
            uint64_t at = 0;
            for (const FrameDesc &fr : f.frames) {
                LlFrame lf{at, fr.samples, (uint32_t)c->ll_wr.size(), fr.n_channels,
                           (f.channels == 2 && (fr.flags & 1)) ? 1u : 0u};
                for (unsigned k = 0; k < fr.n_channels; k++) {
                    const ChannelDesc &cd = f.channels_desc[fr.first_channel + k];
                    LlWrapper w{};
                    w.d.off = base[i] + cd.off;
                    w.d.len = cd.len;
                    w.d.samples = fr.samples;
                    w.d.n_coeffs = cd.n_coeffs;
                    w.d.shift_bits = cd.shift_bits;
                    w.d.rice_k = cd.rice_k;
                    memcpy(w.d.coeffs, cd.coeffs, sizeof w.d.coeffs);
                    // which kernels take the wrapper: the same rules as flo_decode (ll_decode_device in flo_api.cpp)
                    const LlChannelDev &d = w.d;
                    const bool rice = d.len > 0 && (d.n_coeffs > 0 || d.shift_bits >= 128);
                    long long csum = 0;
                    for (unsigned q = 0; q < d.n_coeffs; q++) csum += d.coeffs[q] < 0 ? -(long long)d.coeffs[q] : (long long)d.coeffs[q];
                    bool ser = (rice && d.rice_k > kRiceMaxK) || csum >= (1ll << 21) || (d.n_coeffs && (d.shift_bits & 63u) > 20u);
                    if (rice && d.len > 16u * 1024u * (unsigned)kRiceTileBits) ser = true;
                    w.serial = ser ? 1 : 0;
                    w.other = !(d.n_coeffs > 0 && d.n_coeffs <= 12 && d.len > 0 && d.samples > d.n_coeffs) ? 1 : 0;
                    w.tiles = rice && !ser ? (d.len + (unsigned)kRiceTileBits / 8u - 1u) / ((unsigned)kRiceTileBits / 8u) : 0u;
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
    for (Slot &s : c->slots)
        if (hipEventCreateWithFlags(&s.ev, hipEventDisableTiming) != hipSuccess) return bail(fail(ctx, FLO_ERR_DEVICE, "hipEventCreate failed"));
    if (hipEventCreateWithFlags(&c->ev_in, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_out, hipEventDisableTiming) != hipSuccess)
        return bail(fail(ctx, FLO_ERR_DEVICE, "hipEventCreate failed"));
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
    c->chs.clear();
    c->tile0.assign(1, 0u);
    c->others.clear();
    c->serial.clear();
    c->items.clear();
    uint64_t scratch = 0;
    unsigned max_tiles = 0, max_count = 0;
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
            it.first_channel = (unsigned)c->chs.size();
            it.n_channels = fr->n_channels;
            it.from = (unsigned)(a - fr->start);
            it.count = (unsigned)(b - a);
            it.mid_side = fr->mid_side;
            max_count = std::max(max_count, it.count);
            for (unsigned k = 0; k < fr->n_channels; k++) {
                const LlWrapper &x = c->ll_wr[fr->first_wrapper + k];
                const unsigned i = (unsigned)c->chs.size();
                c->chs.push_back(x.d);
                c->chs.back().out_off = scratch;
                scratch += fr->samples;
                c->serial.push_back(x.serial);
                if (x.other) c->others.push_back(i);
                c->tile0.push_back(c->tile0.back() + x.tiles);
                max_tiles = std::max(max_tiles, x.tiles);
            }
            c->items.push_back(it);
        }
    }
    // one descriptor block: [lossy windows][tails][wrappers][tile0][serial][others][items]
    auto up256 = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t o_win = 0, o_tail = o_win + up256(c->wins.size() * sizeof(LossyWinDev)),
                 o_ch = o_tail + up256(c->tails.size() * sizeof(WinTailDev)), o_t0 = o_ch + up256(c->chs.size() * sizeof(LlChannelDev)),
                 o_ser = o_t0 + up256(c->tile0.size() * sizeof(unsigned int)), o_oth = o_ser + up256(c->serial.size() * sizeof(int)),
                 o_it = o_oth + up256(c->others.size() * sizeof(unsigned int)), bytes = o_it + up256(c->items.size() * sizeof(LlWinItem));
    // the staging slot: reused only after the copy out of it has completed (in steady state long since)
    Slot &sl = c->slots[c->next_slot++ % kStageSlots];
    if (sl.used) HIPCHK(ctx, hipEventSynchronize(sl.ev));
    if (sl.cap < bytes) {
        if (sl.pin) hipHostFree(sl.pin);
        sl.pin = nullptr;
        sl.cap = 0;
        const size_t want = bytes + bytes / 4;
        HIPCHK(ctx, hipHostMalloc(&sl.pin, want, hipHostMallocDefault));
        sl.cap = want;
    }
    uint8_t *pin = (uint8_t *)sl.pin;
    memcpy(pin + o_win, c->wins.data(), c->wins.size() * sizeof(LossyWinDev));
    memcpy(pin + o_tail, c->tails.data(), c->tails.size() * sizeof(WinTailDev));
    memcpy(pin + o_ch, c->chs.data(), c->chs.size() * sizeof(LlChannelDev));
    memcpy(pin + o_t0, c->tile0.data(), c->tile0.size() * sizeof(unsigned int));
    memcpy(pin + o_ser, c->serial.data(), c->serial.size() * sizeof(int));
    memcpy(pin + o_oth, c->others.data(), c->others.size() * sizeof(unsigned int));
    memcpy(pin + o_it, c->items.data(), c->items.size() * sizeof(LlWinItem));
    int rc;
    if ((rc = grow(c, c->desc, bytes)) != FLO_OK) return rc;
    if (!c->chs.empty()) {
        const size_t tiles = c->tile0.back();
        if ((rc = grow(c, c->scr, scratch * sizeof(int))) != FLO_OK || (rc = grow(c, c->tabs, (tiles ? tiles : 1) * kRiceStates * sizeof(unsigned int))) != FLO_OK ||
            (rc = grow(c, c->ent, (tiles ? tiles : 1) * sizeof(uint2))) != FLO_OK)
            return rc;
    }
    // order: after what the caller queued on `stream`; the caller's later work after ours
    hipStream_t us = (hipStream_t)stream, cs = ctx->stream;
    if (us != cs) {
        HIPCHK(ctx, hipEventRecord(c->ev_in, us));
        HIPCHK(ctx, hipStreamWaitEvent(cs, c->ev_in, 0));
    }
    uint8_t *d = (uint8_t *)c->desc.p;
    HIPCHK(ctx, hipMemcpyAsync(d, pin, bytes, hipMemcpyHostToDevice, cs));
    HIPCHK(ctx, hipEventRecord(sl.ev, cs));
    sl.used = true;
    if (!c->tails.empty()) {
        const WinTailDev *t = reinterpret_cast<const WinTailDev *>(d + o_tail);
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
        LossyWinArgs W{reinterpret_cast<const LossyWinDev *>(d + o_win), (unsigned)c->wins.size(), rpw, window_frames};
        if ((rc = timed_launch(ctx, "lossy_window", [&] { return launch_lossy_window(A, W, run, cs); })) != FLO_OK) return rc;
    }
    if (!c->chs.empty()) {
        const LlChannelDev *d_ch = reinterpret_cast<const LlChannelDev *>(d + o_ch);
        int *d_ser = reinterpret_cast<int *>(d + o_ser);
        LlParArgs P{c->d_bytes, d_ch, (unsigned)c->chs.size(), (int *)c->scr.p, reinterpret_cast<const unsigned int *>(d + o_t0),
                    (unsigned int *)c->tabs.p, (uint2 *)c->ent.p, d_ser, reinterpret_cast<const unsigned int *>(d + o_oth),
                    (unsigned)c->others.size()};
        if ((rc = timed_launch(ctx, "window_ll_decode_parallel", [&] { return launch_ll_decode_parallel(P, max_tiles, cs); })) != FLO_OK) return rc;
        LlDecArgs S{c->d_bytes, d_ch, (unsigned)c->chs.size(), (int *)c->scr.p, d_ser};
        if ((rc = timed_launch(ctx, "window_ll_decode", [&] { return launch_ll_decode(S, cs); })) != FLO_OK) return rc;
        LlWinFinishArgs F{reinterpret_cast<const LlWinItem *>(d + o_it), d_ch, (unsigned)c->items.size(), (int)c->channels,
                          (const int *)c->scr.p, dst_device};
        if ((rc = timed_launch(ctx, "window_ll_finish", [&] { return launch_ll_window_finish(F, max_count, cs); })) != FLO_OK) return rc;
    }
    if (us != cs) {
        HIPCHK(ctx, hipEventRecord(c->ev_out, cs));
        HIPCHK(ctx, hipStreamWaitEvent(us, c->ev_out, 0));
    }
    return FLO_OK;
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
