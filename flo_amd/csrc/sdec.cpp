// sdec.cpp — flo_sdec_*: libflo's StreamingDecoder (libflo/src/streaming/decoder.rs), with a batched form that decodes
// the newly complete frames of many streams in one set of launches.
//
// The state machine, the counters and the frame parser are restated from decoder.rs statement by statement on the host
// (cited as :line). The decode itself runs on the device:
//   transform frames: lossy_decode_kernel<kDecStream> (decode_kernels.hip) on a per-call list of the frames that
//                     deserialise, cut into runs of at most 16 blocks; a stream's overlap (the TransformDecoder's
//                     overlap buffer, mdct.rs:449-456) stays in device memory between calls
//   other frames:     the parallel Rice / predictor kernels (lldec_kernels.hip) on a per-call wrapper list, then
//                     ll_finish_kernel writes each frame's samples to its place in its decoder's output range
// Per call only the payload bytes of the frames decoded in it are gathered into a pinned staging slot and uploaded,
// together with the descriptors, as one copy.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "container.hpp"
#include "ctx_internal.hpp"
#include "decode_kernels.hpp"
#include "decode_plan.hpp"
#include "devpool.hpp"

namespace {
constexpr size_t kHeaderBytes = 70;           // try_parse_header reads a fixed 70 bytes (:177-180)
constexpr uint32_t kMaxFrameSamples = 2000000;   // the container reader's limit (reader.rs); the device path keeps it

uint16_t rd16(const uint8_t *p) { return (uint16_t)(p[0] | (p[1] << 8)); }
uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
uint64_t rd64(const uint8_t *p) { return (uint64_t)rd32(p) | ((uint64_t)rd32(p + 4) << 32); }

// One channel wrapper as parse_frame / parse_alpc_channel leave it (:356-473). Offsets are relative to the frame.
struct SdChannel {
    uint32_t off = 0, len = 0;       // "residuals"
    uint8_t n_coeffs = 0, shift = 0, enc = 0, rice_k = 0;
    int32_t coeffs[12] = {};
};
struct SdFrame {
    uint8_t type = 0, flags = 0;
    uint32_t samples = 0;
    std::vector<SdChannel> ch;
};

// parse_alpc_channel (:427-473); false with the reference's message
bool parse_alpc_channel(const uint8_t *d, uint32_t base, uint32_t len, SdChannel &c, const char **err) {
    c = SdChannel();
    if (len == 0) return true;   // empty: silence (:428-430)
    const uint32_t order = d[0];
    if (order > 12) {
        *err = "Invalid LPC order";
        return false;
    }
    if (len < 1 + order * 4 + 2) {   // order + coeffs + shift + encoding (:437-441)
        *err = "ALPC channel too small";
        return false;
    }
    for (uint32_t i = 0; i < order; i++) c.coeffs[i] = (int32_t)rd32(d + 1 + 4 * i);
    c.n_coeffs = (uint8_t)order;
    uint32_t pos = 1 + order * 4;
    c.shift = d[pos++];
    c.enc = d[pos++];   // ResidualEncoding::from: 0 Rice, 1 Golomb, else Raw (types.rs)
    if (c.enc == 0) {   // the rice parameter only for Rice (:458-465)
        if (pos >= len) {
            *err = "Missing rice parameter";
            return false;
        }
        c.rice_k = d[pos++];
    }
    c.off = base + pos;   // the rest is residuals
    c.len = len - pos;
    return true;
}

// parse_frame (:356-425)
bool parse_frame(const uint8_t *d, uint32_t len, uint8_t channels, SdFrame &f, const char **err) {
    if (len < 6) {
        *err = "Frame too small";
        return false;
    }
    f.type = d[0];
    f.samples = rd32(d + 1);
    f.flags = d[5];
    f.ch.clear();
    const unsigned n = f.type == 253 ? 1u : channels;   // a transform frame has one wrapper (:374-378)
    uint32_t pos = 6;
    for (unsigned k = 0; k < n; k++) {
        if ((uint64_t)pos + 4 > len) {
            *err = "Frame truncated";
            return false;
        }
        const uint32_t cs = rd32(d + pos);
        pos += 4;
        if ((uint64_t)pos + cs > len) {
            *err = "Channel data truncated";
            return false;
        }
        SdChannel c;
        if (f.type == 0) {
            // Silence: no residuals
        } else if (f.type == 253 || f.type == 254) {   // Raw / Transform: the whole wrapper is the residuals
            c.off = pos;
            c.len = cs;
        } else if (!parse_alpc_channel(d + pos, pos, cs, c, err)) {   // ALPC and the reserved types (:403)
            return false;
        }
        pos += cs;
        f.ch.push_back(c);
    }
    return true;
}

// deserialize_frame (lossy/decoder.rs:61-131) reduced to what decides between None and Some: every failure is structural.
enum { kBlobOk = 0, kBlobNone = 1, kBlobUnsupported = 2 };
int classify_blob(const uint8_t *b, uint32_t len, uint8_t channels) {
    if (len < 2) return kBlobNone;
    if (b[0] > 3) return kBlobNone;
    const uint32_t nch = b[1];
    uint64_t pos = 2 + 50ull * nch;
    if (pos > len) return kBlobNone;
    for (uint32_t k = 0; k < nch; k++) {
        if (pos + 4 > len) return kBlobNone;
        const uint32_t l = rd32(b + pos);
        pos += 4;
        if (pos + l > len) return kBlobNone;
        pos += l;
    }
    // deserialisable; what the device kernel does not take: Short / Start / Stop blocks, more channels than the stream
    if (b[0] != 0 || nch > channels) return kBlobUnsupported;
    return kBlobOk;
}

enum : uint8_t { kItemLossless = 0, kItemBlock = 1, kItemPreroll = 2, kItemSkipped = 3 };
struct SdItem {
    uint32_t frame;    // TOC index
    uint8_t kind;
    uint64_t floats;   // output floats
};
struct SdPlan {
    std::vector<SdItem> items;
    uint64_t floats = 0;
    int status = FLO_OK;
    std::string err;
    bool finish = false;   // a next_frame call would find current_frame >= toc.len() (:93-96)
};
}  // namespace

struct flo_sdec {
    flo_ctx *ctx = nullptr;
    std::vector<uint8_t> buffer;
    int state = FLO_SDEC_WAITING_HEADER;
    bool have_header = false;
    flo_sdec_audio_info info{};
    uint16_t flags = 0;
    uint64_t toc_size = 0;
    std::vector<TocDesc> toc;
    size_t current = 0;
    size_t data_offset = 0;
    bool is_lossy = false;
    bool skipped_preroll = false;
    std::string err;
    uint64_t version = 0;       // bumped by every change a plan depends on (flo_sdec_decode_ready's sizing reuse)
    // device side
    float *d_state = nullptr;   // [2][channels][1024] overlap of the last transform frame decoded: read half `parity`,
    size_t state_floats = 0;    // a call's last run writes the other one (the runs of one launch are not ordered)
    unsigned parity = 0;
    bool stored = false;        // the queued launch writes the other half: flip `parity` at commit
    float *d_one = nullptr;     // next_frame's output
    size_t one_cap = 0;
};

// The per-context workspace of flo_sdec_decode_ready: staging slots, device blocks that only grow, host lists.
struct SdecWork {
    StageRing ring;
    void *desc = nullptr, *scr = nullptr, *tabs = nullptr, *ent = nullptr;
    size_t desc_cap = 0, scr_cap = 0, tabs_cap = 0, ent_cap = 0;
    std::vector<SdPlan> plans;
    // the plans of the last sizing call (NULL destination), reused by a call with the same decoders, cap and versions
    bool sized = false;
    uint32_t sized_cap = 0;
    std::vector<const flo_sdec *> sized_decs;
    std::vector<uint64_t> sized_ver;
    std::vector<LossyRunDev> runs;
    std::vector<unsigned long long> blob_off;
    std::vector<unsigned int> blob_len;
    LlWrapperList ll;
    std::vector<std::pair<const uint8_t *, uint32_t>> segs;   // payload bytes to gather, in upload order
};

void sdec_work_free(flo_ctx *c) {
    SdecWork *w = c ? c->sdec : nullptr;
    if (!w) return;
    hipStreamSynchronize(c->stream);
    for (void *p : {w->desc, w->scr, w->tabs, w->ent})
        if (p) pool_free(p);
    delete w;
    c->sdec = nullptr;
}

namespace {
int sd_fail(flo_sdec *d, flo_ctx *ctx, int code, const std::string &msg) {
    d->err = msg;
    return fail(ctx, code, msg);
}

// try_parse_header (:176-276): 70 bytes; bad magic is the only error
bool try_parse_header(flo_sdec *d) {
    if (d->buffer.size() < kHeaderBytes) return false;
    const uint8_t *b = d->buffer.data();
    if (memcmp(b, "FLO!", 4) != 0) {
        d->state = FLO_SDEC_ERROR;
        d->err = "Invalid flo file: bad magic";
        return false;
    }
    d->flags = rd16(b + 6);
    d->info.sample_rate = rd32(b + 8);
    d->info.channels = b[12];
    d->info.bit_depth = b[13];
    d->info.total_samples = rd64(b + 14);
    d->toc_size = rd64(b + 38);   // header_size (30..37) is read and ignored
    d->is_lossy = (d->flags & 0x01) != 0;
    d->info.is_lossy = d->is_lossy ? 1 : 0;
    d->have_header = true;
    return true;
}

// try_parse_toc (:278-341). Entries are pushed as they are read; a TOC shorter than its count says leaves the ones read
// pushed, and the next feed reads (and pushes) them again.
bool try_parse_toc(flo_sdec *d) {
    const uint64_t toc_start = kHeaderBytes;
    const uint64_t toc_end = toc_start + d->toc_size;
    if (toc_end < toc_start || d->buffer.size() < toc_end) return false;   // (a wrapping sum: the reference would panic)
    const uint8_t *b = d->buffer.data();
    if (d->toc_size >= 4) {
        const uint64_t n = rd32(b + toc_start);
        const uint64_t es = toc_start + 4;
        for (uint64_t i = 0; i < n; i++) {
            const uint64_t o = es + i * 20;
            if (o + 20 > d->buffer.size()) return false;
            TocDesc e;
            e.frame_index = rd32(b + o);
            e.byte_offset = rd64(b + o + 4);
            e.frame_size = rd32(b + o + 12);
            e.timestamp_ms = rd32(b + o + 16);
            d->toc.push_back(e);
        }
    }
    d->data_offset = (size_t)toc_end;
    return true;
}

// [start, end) of TOC entry i in the buffer; false when the sum does not fit (never complete)
bool frame_span(const flo_sdec *d, size_t i, uint64_t &start, uint64_t &end) {
    const TocDesc &e = d->toc[i];
    start = (uint64_t)d->data_offset + e.byte_offset;
    if (start < e.byte_offset) return false;
    end = start + e.frame_size;
    return end >= start;
}

// count_complete_frames (:343-354)
size_t count_complete(const flo_sdec *d) {
    size_t n = 0;
    for (size_t i = 0; i < d->toc.size(); i++) {
        uint64_t s, e;
        if (!frame_span(d, i, s, e) || e > d->buffer.size()) break;
        n++;
    }
    return n;
}

// try_advance_state (:153-174)
bool try_advance(flo_sdec *d) {
    for (;;) {
        if (d->state == FLO_SDEC_WAITING_HEADER) {
            if (!try_parse_header(d)) return false;
            d->state = FLO_SDEC_WAITING_TOC;
            continue;
        }
        if (d->state == FLO_SDEC_WAITING_TOC) {
            if (!try_parse_toc(d)) return false;
            d->state = FLO_SDEC_READY;
            return true;
        }
        if (d->state == FLO_SDEC_READY) return count_complete(d) > d->current;
        return false;
    }
}

// What `cap` next_frame calls (0: as many as there are complete frames) would return, without changing the decoder.
// A frame the device path does not take stops the plan like a parse error, with FLO_ERR_FORMAT.
void plan_frames(const flo_sdec *d, uint32_t cap, SdPlan &p) {
    p.items.clear();
    p.floats = 0;
    p.status = FLO_OK;
    p.err.clear();
    p.finish = false;
    if (d->state != FLO_SDEC_READY) return;
    if (d->current >= d->toc.size()) {
        p.finish = true;
        return;
    }
    const size_t complete = count_complete(d);
    const uint64_t ch = d->info.channels;
    bool pre = d->skipped_preroll;
    SdFrame f;
    for (size_t j = d->current; j < complete && (cap == 0 || p.items.size() < cap); j++) {
        uint64_t s, e;
        frame_span(d, j, s, e);
        const uint8_t *fb = d->buffer.data() + s;
        const char *perr = "";
        if (!parse_frame(fb, (uint32_t)(e - s), d->info.channels, f, &perr)) {
            p.status = FLO_ERR_FORMAT;
            p.err = perr;
            return;
        }
        SdItem it{(uint32_t)j, kItemLossless, 0};
        if (f.type == 253) {
            if (!d->is_lossy) {
                p.status = FLO_ERR_FORMAT;
                p.err = "Transform frame in a lossless stream: not supported by the device decoder";
                return;
            }
            const int cls = classify_blob(fb + f.ch[0].off, f.ch[0].len, d->info.channels);
            if (cls == kBlobUnsupported) {
                p.status = FLO_ERR_FORMAT;
                p.err = "Transform frame with a non-Long block or more channels than the stream: not supported by the device decoder";
                return;
            }
            if (cls == kBlobNone) {
                it.kind = kItemSkipped;   // an empty frame; the overlap is untouched (:487-499)
            } else if (!pre) {
                it.kind = kItemPreroll;   // the first frame that deserialises: empty, feeds the overlap (:493-497)
                pre = true;
            } else {
                it.kind = kItemBlock;
                it.floats = 1024 * ch;
            }
        } else {
            if (d->is_lossy) {
                p.status = FLO_ERR_FORMAT;
                p.err = "Non-transform frame in a lossy stream: not supported by the device decoder";
                return;
            }
            if (f.samples > kMaxFrameSamples) {
                p.status = FLO_ERR_FORMAT;
                p.err = "Invalid frame: too many samples";
                return;
            }
            for (const SdChannel &c : f.ch)
                if (c.n_coeffs && c.enc != 0) {
                    p.status = FLO_ERR_FORMAT;
                    p.err = "ALPC channel with coefficients and non-Rice residuals: not supported by the device decoder";
                    return;
                }
            it.floats = (uint64_t)f.samples * ch;
        }
        p.items.push_back(it);
        p.floats += it.floats;
    }
}

// the decoder's counters after its plan ran (next_frame :98-112, once per item)
void commit_plan(flo_sdec *d, const SdPlan &p) {
    d->version++;
    if (d->stored) {   // the next call reads what this one's last run wrote
        d->parity ^= 1u;
        d->stored = false;
    }
    if (p.finish) {
        d->state = FLO_SDEC_FINISHED;
        return;
    }
    for (const SdItem &it : p.items)
        if (it.kind == kItemPreroll) d->skipped_preroll = true;
    d->current += p.items.size();
}

// make `p` hold `bytes`; growth waits for the queued work that may still read the old block
int grow(flo_ctx *ctx, void *&p, size_t &cap, size_t bytes) {
    if (bytes <= cap) return FLO_OK;
    if (p) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        pool_free(p);
    }
    p = nullptr;
    cap = 0;
    const size_t want = bytes + bytes / 4 + 256;
    if (pool_alloc(&p, want) != hipSuccess) return fail(ctx, FLO_ERR_NOMEM, "streaming decoder scratch");
    cap = want;
    return FLO_OK;
}

SdecWork *work(flo_ctx *ctx) {
    if (ctx->sdec) return ctx->sdec;
    SdecWork *w = new SdecWork();
    w->ring.init();   // (a slot without its event fails when it is taken)
    ctx->sdec = w;
    return w;
}


// Enqueue the decode of the plans in w->plans (decoder i's output at dst + off[i]) on the ctx stream, ordered after what
// is queued on `us` and before its later work. Changes no decoder's counters.
int launch_plans(flo_ctx *ctx, SdecWork *w, size_t n, flo_sdec *const *decs, const uint64_t *off, float *dst, hipStream_t us) {
    uint32_t sr = 0;
    int nch = -1;
    w->runs.clear();
    w->blob_off.clear();
    w->blob_len.clear();
    w->ll.clear();
    w->segs.clear();
    uint64_t bytes_up = 0;
    auto add_seg = [&](const uint8_t *p, uint32_t len) -> uint64_t {   // -> the payload's offset in the uploaded bytes
        const uint64_t at = bytes_up;
        w->segs.push_back({p, len});
        bytes_up += ((uint64_t)len + 15) & ~(uint64_t)15;
        return at;
    };
    SdFrame f;
    const char *perr = "";
    for (size_t i = 0; i < n; i++) {
        flo_sdec *d = decs[i];
        const SdPlan &p = w->plans[i];
        d->stored = false;
        bool dev = false;
        for (const SdItem &it : p.items) dev = dev || it.kind != kItemSkipped;
        if (!dev) continue;
        if (nch < 0) {
            sr = d->info.sample_rate;
            nch = d->info.channels;
        } else if (sr != d->info.sample_rate || nch != (int)d->info.channels) {
            return fail(ctx, FLO_ERR_ARG, "decoders of one call differ in sample rate or channel count (decoder " + std::to_string(i) + ")");
        }
        if (d->ctx && d->ctx != ctx) return fail(ctx, FLO_ERR_ARG, "decoder " + std::to_string(i) + " belongs to another context");
        const uint64_t ch = d->info.channels;
        if (!ch) continue;   // no channel: every frame is empty
        if (d->is_lossy) {
            // the stream's frames that deserialise, in order (the first may be the pre-roll: it writes no block); their
            // blocks follow each other from off[i]
            const uint64_t first = w->blob_off.size();
            bool preroll = false;
            for (const SdItem &it : p.items) {
                if (it.kind != kItemBlock && it.kind != kItemPreroll) continue;
                preroll = preroll || it.kind == kItemPreroll;
                uint64_t s, e;
                frame_span(d, it.frame, s, e);
                const uint8_t *fb = d->buffer.data() + s;
                parse_frame(fb, (uint32_t)(e - s), d->info.channels, f, &perr);
                w->blob_off.push_back(add_seg(fb + f.ch[0].off, f.ch[0].len));
                w->blob_len.push_back(f.ch[0].len);
            }
            const uint64_t m = w->blob_off.size() - first;
            if (!m) continue;
            // two halves of 1024 x channels floats; a stream reset to more channels gets a larger block. The state is
            // written before it is first read: the pre-roll's run stores without loading.
            if (d->state_floats < 2 * 1024 * ch) {
                if (d->d_state) {
                    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // queued work may still use the old block
                    pool_free(d->d_state);
                    d->d_state = nullptr;
                    d->state_floats = 0;
                }
                if (pool_alloc(&d->d_state, 2 * 1024 * ch * sizeof(float)) != hipSuccess) return fail(ctx, FLO_ERR_NOMEM, "streaming decoder state");
                d->state_floats = 2 * 1024 * ch;
                d->ctx = ctx;
            }
            // runs of at most 16 blocks: the first from the stored overlap (or from the pre-roll), each later one one frame
            // early, re-decoding the frame before its first block for that frame's second half; the last stores the overlap
            const uint64_t ws = preroll ? 1 : 0, blk = 1024 * ch;
            uint64_t a = ws;
            bool head = true;
            do {
                const uint64_t b = std::min<uint64_t>(m, a + (uint64_t)16);
                LossyRunDev r{};
                if (head && ws == 0) {
                    r.frame0 = first;
                    r.n_frames = (unsigned)b;
                    r.flags = kRunLoad | kRunWriteFirst;
                } else {
                    r.frame0 = first + a - 1;
                    r.n_frames = (unsigned)(b - a + 1);
                    // a channel the lead frame does not carry keeps an older overlap: the kernel looks for it in the
                    // call's earlier frames of this stream, then in the stored state (the pre-roll has nothing before it)
                    r.back = (unsigned)(a - 1);
                    if (ws == 0) r.flags |= kRunBackLoad;
                }
                r.dst = off[i] + (a - ws) * blk;
                r.state = d->d_state;
                if (d->parity) r.flags |= kRunOdd;
                if (b == m) r.flags |= kRunStore;
                w->runs.push_back(r);
                head = false;
                a = b;
            } while (a < m);
            d->stored = true;
            continue;
        }
        if (!d->ctx) d->ctx = ctx;
        uint64_t at = off[i];
        for (const SdItem &it : p.items) {
            uint64_t s, e;
            frame_span(d, it.frame, s, e);
            const uint8_t *fb = d->buffer.data() + s;
            parse_frame(fb, (uint32_t)(e - s), d->info.channels, f, &perr);
            w->ll.add_frame(at / ch, f.samples, ch == 2 && (f.flags & 1), (unsigned)f.ch.size(), false, [&](unsigned k) {
                const SdChannel &sc = f.ch[k];
                return ll_channel(sc.len ? add_seg(fb + sc.off, sc.len) : 0, sc.len, sc.n_coeffs, sc.shift, sc.rice_k, sc.coeffs);
            });
            at += it.floats;
        }
    }
    const LlWrapperList &ll = w->ll;
    if (w->runs.empty() && ll.chs.empty()) return FLO_OK;
    TableSet *ts = nullptr;
    int rc;
    if (!w->runs.empty() && (rc = get_tables(ctx, sr, 0.5f, &ts)) != FLO_OK) return rc;
    // one block, the payload bytes last (the lossy kernel reads up to three bytes past a blob)
    enum { kRun, kBlobOff, kBlobLen, kCh, kT0, kSer, kOth, kFr, kErr, kBytes };
    const DescBlock blk{desc_part(w->runs), desc_part(w->blob_off), desc_part(w->blob_len), desc_part(ll.chs), desc_part(ll.tile0),
                        desc_part(ll.serial), desc_part(ll.others), desc_part(ll.frs), {nullptr, 256}, {nullptr, bytes_up + 32}};
    uint8_t *pin;
    if ((rc = w->ring.acquire(ctx, blk.bytes, &pin)) != FLO_OK) return rc;
    blk.fill(pin);
    memset(pin + blk.off[kErr], 0, 256);
    {
        uint8_t *by = pin + blk.off[kBytes];
        uint64_t at = 0;
        for (const auto &sg : w->segs) {
            memcpy(by + at, sg.first, sg.second);
            at += ((uint64_t)sg.second + 15) & ~(uint64_t)15;
        }
        memset(by + at, 0, 32);
    }
    if ((rc = grow(ctx, w->desc, w->desc_cap, blk.bytes)) != FLO_OK) return rc;
    if (!ll.chs.empty()) {
        const size_t tiles = ll.tiles();
        if ((rc = grow(ctx, w->scr, w->scr_cap, (ll.scratch ? ll.scratch : 1) * sizeof(int))) != FLO_OK ||
            (rc = grow(ctx, w->tabs, w->tabs_cap, (tiles ? tiles : 1) * kRiceStates * sizeof(unsigned int))) != FLO_OK ||
            (rc = grow(ctx, w->ent, w->ent_cap, (tiles ? tiles : 1) * sizeof(uint2))) != FLO_OK)
            return rc;
    }
    hipStream_t cs = ctx->stream;
    if ((rc = w->ring.fence_in(ctx, us)) != FLO_OK || (rc = w->ring.upload(ctx, w->desc, blk.bytes)) != FLO_OK) return rc;
    void *dd = w->desc;
    const uint8_t *d_bytes = blk.at<const uint8_t>(dd, kBytes);
    if (!w->runs.empty()) {
        LossyDecArgs A{};
        A.T = ts->dev;
        A.window = ts->dev_window;
        A.bytes = d_bytes;
        A.blob_off = blk.at<const unsigned long long>(dd, kBlobOff);
        A.blob_len = blk.at<const unsigned int>(dd, kBlobLen);
        A.channels = nch;
        A.out = dst;
        A.error = blk.at<int>(dd, kErr);   // (never set: the host has checked every frame)
        LossyStreamArgs S{blk.at<const LossyRunDev>(dd, kRun), (unsigned)w->runs.size(), 0u};
        if ((rc = timed_launch(ctx, "sdec_lossy", [&] { return launch_lossy_stream(A, S, cs); })) != FLO_OK) return rc;
    }
    if (!ll.chs.empty()) {
        const LlChannelDev *d_ch = blk.at<const LlChannelDev>(dd, kCh);
        if ((rc = launch_ll_wrappers(ctx, ll, d_bytes, d_ch, blk.at<const unsigned int>(dd, kT0), blk.at<int>(dd, kSer),
                                     blk.at<const unsigned int>(dd, kOth), (int *)w->scr, (unsigned int *)w->tabs, (uint2 *)w->ent,
                                     "sdec_ll_decode_parallel", "sdec_ll_decode")) != FLO_OK)
            return rc;
        LlFinishArgs F{blk.at<const LlFrameDev>(dd, kFr), d_ch, (unsigned)ll.frs.size(), nch, (const int *)w->scr, dst, nullptr};
        if ((rc = timed_launch(ctx, "sdec_ll_finish", [&] { return launch_ll_finish(F, ll.max_samples, cs); })) != FLO_OK) return rc;
    }
    return w->ring.fence_out(ctx, us);
}

// decode_with_standard_decoder for transform files (:741-767) skips a frame that does not deserialise; flo_decode fails on
// it. The same file without those frames: the header with a new TOC and DATA holding the kept frames' bytes.
std::vector<uint8_t> without_frames(const uint8_t *b, const ParsedFile &f, const std::vector<char> &keep) {
    std::vector<uint8_t> data;
    std::vector<uint8_t> toc;
    uint32_t kept = 0;
    for (size_t i = 0; i < f.frames.size(); i++) {
        if (!keep[i]) continue;
        const FrameDesc &fr = f.frames[i];
        const TocDesc &e = f.toc[i];
        const uint64_t s = f.data_start + e.byte_offset;
        uint64_t end = std::max<uint64_t>(s + e.frame_size, s + 6 + 4ull * fr.n_channels);
        for (unsigned k = 0; k < fr.n_channels; k++) {
            const ChannelDesc &cd = f.channels_desc[fr.first_channel + k];
            end = std::max<uint64_t>(end, cd.off + cd.len);
        }
        uint8_t ent[20];
        const uint64_t bo = data.size();
        memcpy(ent, &kept, 4);
        memcpy(ent + 4, &bo, 8);
        memcpy(ent + 12, &e.frame_size, 4);
        memcpy(ent + 16, &e.timestamp_ms, 4);
        toc.insert(toc.end(), ent, ent + 20);
        data.insert(data.end(), b + s, b + end);
        kept++;
    }
    std::vector<uint8_t> out(b, b + kHeaderBytes);
    const uint64_t toc_size = 4 + toc.size(), data_size = data.size(), zero = 0;
    memcpy(out.data() + 38, &toc_size, 8);
    memcpy(out.data() + 46, &data_size, 8);
    memcpy(out.data() + 54, &zero, 8);   // no EXTRA
    memcpy(out.data() + 62, &zero, 8);   // no META
    out.insert(out.end(), (const uint8_t *)&kept, (const uint8_t *)&kept + 4);
    out.insert(out.end(), toc.begin(), toc.end());
    out.insert(out.end(), data.begin(), data.end());
    return out;
}
}  // namespace

extern "C" int flo_sdec_create(flo_ctx *ctx, flo_sdec **out) {
    if (!out) return FLO_ERR_ARG;
    flo_sdec *d = new flo_sdec();
    d->ctx = ctx;
    d->buffer.reserve(64 * 1024);
    *out = d;
    return FLO_OK;
}

static void sdec_free_device(flo_sdec *d) {
    if ((d->d_state || d->d_one) && d->ctx) hipStreamSynchronize(d->ctx->stream);
    if (d->d_state) pool_free(d->d_state);
    if (d->d_one) pool_free(d->d_one);
    d->d_state = d->d_one = nullptr;
    d->state_floats = d->one_cap = 0;
}

extern "C" void flo_sdec_destroy(flo_sdec *d) {
    if (!d) return;
    sdec_free_device(d);
    delete d;
}

extern "C" int flo_sdec_attach(flo_sdec *d, flo_ctx *ctx) {
    if (!d || !ctx) return FLO_ERR_ARG;
    if (d->ctx && d->ctx != ctx) return FLO_ERR_STATE;
    d->ctx = ctx;
    return FLO_OK;
}

extern "C" const char *flo_sdec_last_error(const flo_sdec *d) { return d ? d->err.c_str() : ""; }

// feed (:70-78)
extern "C" int flo_sdec_feed(flo_sdec *d, const uint8_t *data, size_t len, int *new_frames) {
    if (!d || (!data && len)) return FLO_ERR_ARG;
    if (new_frames) *new_frames = 0;
    if (d->state == FLO_SDEC_ERROR || d->state == FLO_SDEC_FINISHED) return FLO_OK;
    d->buffer.insert(d->buffer.end(), data, data + len);
    d->version++;
    const bool more = try_advance(d);
    if (d->state == FLO_SDEC_ERROR) return fail(d->ctx, FLO_ERR_FORMAT, d->err);   // bad magic (:182-185)
    if (new_frames) *new_frames = more ? 1 : 0;
    return FLO_OK;
}

extern "C" int flo_sdec_state(const flo_sdec *d) { return d ? d->state : FLO_SDEC_ERROR; }

extern "C" int flo_sdec_info(const flo_sdec *d, flo_sdec_audio_info *out) {
    if (!d || !out) return FLO_ERR_ARG;
    if (!d->have_header) return FLO_ERR_STATE;   // info() is None before the header (:51-60)
    *out = d->info;
    return FLO_OK;
}

// frames_available (:63-68): complete frames, not minus the current one
extern "C" size_t flo_sdec_frames_available(const flo_sdec *d) {
    if (!d || d->state != FLO_SDEC_READY) return 0;
    return count_complete(d);
}

// available_frames (:143-149)
extern "C" size_t flo_sdec_available_frames(const flo_sdec *d) {
    if (!d || d->state != FLO_SDEC_READY) return 0;
    const size_t n = count_complete(d);
    return n > d->current ? n - d->current : 0;
}

extern "C" size_t flo_sdec_current_frame_index(const flo_sdec *d) { return d ? d->current : 0; }
extern "C" size_t flo_sdec_buffered_bytes(const flo_sdec *d) { return d ? d->buffer.size() : 0; }

// reset (:124-134); the device blocks are kept (the overlap state is written before it is next read)
extern "C" void flo_sdec_reset(flo_sdec *d) {
    if (!d) return;
    d->buffer.clear();
    d->state = FLO_SDEC_WAITING_HEADER;
    d->have_header = false;
    d->info = flo_sdec_audio_info{};
    d->flags = 0;
    d->toc_size = 0;
    d->toc.clear();
    d->current = 0;
    d->data_offset = 0;
    d->is_lossy = false;
    d->skipped_preroll = false;
    d->err.clear();
    d->stored = false;
    d->version++;
}

// next_frame (:81-112)
extern "C" int flo_sdec_next_frame(flo_sdec *d, float **pcm, size_t *n) {
    if (!d || !pcm || !n) return -FLO_ERR_ARG;
    *pcm = nullptr;
    *n = 0;
    if (d->state != FLO_SDEC_READY) return 0;
    flo_ctx *ctx = d->ctx;
    if (!ctx) {
        d->err = "streaming decoder has no context: it can parse but not decode";
        return -FLO_ERR_STATE;
    }
    SdecWork *w = work(ctx);
    w->sized = false;   // the plans below replace the sizing call's
    w->plans.resize(1);
    SdPlan &p = w->plans[0];
    plan_frames(d, 1, p);
    if (p.finish) {
        d->state = FLO_SDEC_FINISHED;
        d->version++;
        return 0;
    }
    if (p.items.empty()) {
        if (p.status == FLO_OK) return 0;   // the frame is not complete yet (:104-106)
        sd_fail(d, ctx, p.status, p.err);     // the same frame fails again on the next call (:109)
        return -p.status;
    }
    if (hipSetDevice(ctx->device) != hipSuccess) return -fail(ctx, FLO_ERR_DEVICE, "hipSetDevice failed");
    const uint64_t floats = p.floats;
    if (p.items[0].kind != kItemSkipped) {
        if (floats > d->one_cap) {
            if (d->d_one) {
                hipStreamSynchronize(ctx->stream);
                pool_free(d->d_one);
            }
            d->d_one = nullptr;
            d->one_cap = 0;
            if (pool_alloc(&d->d_one, floats * sizeof(float)) != hipSuccess) return -fail(ctx, FLO_ERR_NOMEM, "next_frame buffer");
            d->one_cap = floats;
        }
        const uint64_t off0 = 0;
        flo_sdec *one[1] = {d};
        int rc = launch_plans(ctx, w, 1, one, &off0, d->d_one, ctx->stream);
        if (rc != FLO_OK) {
            d->stored = false;
            d->err = ctx->err;
            return -rc;
        }
    }
    float *h = nullptr;
    if (floats) {
        h = (float *)malloc(floats * sizeof(float));
        if (!h) return -fail(ctx, FLO_ERR_NOMEM, "next_frame output");
        if (hipMemcpyAsync(h, d->d_one, floats * sizeof(float), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
            hipStreamSynchronize(ctx->stream) != hipSuccess) {
            free(h);
            return -fail(ctx, FLO_ERR_DEVICE, "next_frame download failed");
        }
    } else if (p.items[0].kind != kItemSkipped && hipStreamSynchronize(ctx->stream) != hipSuccess) {
        return -fail(ctx, FLO_ERR_DEVICE, "next_frame: device work failed");
    }
    commit_plan(d, p);
    *pcm = h;
    *n = floats;
    return 1;
}

// decode_available (:114-122) = decode_with_standard_decoder (:741-774) over the whole buffer
extern "C" int flo_sdec_decode_available(flo_sdec *d, float **pcm, size_t *n) {
    if (!d || !pcm || !n) return FLO_ERR_ARG;
    *pcm = nullptr;
    *n = 0;
    if (d->state != FLO_SDEC_READY) return FLO_OK;
    flo_ctx *ctx = d->ctx;
    if (!ctx) return sd_fail(d, nullptr, FLO_ERR_STATE, "streaming decoder has no context: it can parse but not decode");
    ParsedFile f;
    const char *perr = "";
    const uint8_t *b = d->buffer.data();
    if (parse_file(b, d->buffer.size(), f, &perr) != 0) return sd_fail(d, ctx, FLO_ERR_FORMAT, perr);   // state unchanged
    std::vector<uint8_t> kept;
    const uint8_t *src = b;
    size_t src_len = d->buffer.size();
    if (f.is_transform) {
        std::vector<char> keep(f.frames.size(), 1);
        bool drop = false;
        for (size_t i = 0; i < f.frames.size(); i++) {
            const FrameDesc &fr = f.frames[i];
            if (!fr.n_channels) continue;   // flo_decode skips these itself
            const ChannelDesc &cd = f.channels_desc[fr.first_channel];
            const int cls = classify_blob(b + cd.off, cd.len, f.channels);
            if (cls == kBlobUnsupported)
                return sd_fail(d, ctx, FLO_ERR_FORMAT, "Transform frame with a non-Long block or more channels than the stream: not supported by the device decoder");
            if (cls == kBlobNone) keep[i] = 0, drop = true;
        }
        if (drop) {
            kept = without_frames(b, f, keep);
            src = kept.data();
            src_len = kept.size();
        }
    }
    const int rc = flo_decode(ctx, src, src_len, pcm, n, nullptr, nullptr);
    if (rc != FLO_OK) {
        d->err = ctx->err;
        return rc;
    }
    d->state = FLO_SDEC_FINISHED;
    d->version++;
    return FLO_OK;
}

extern "C" int flo_sdec_decode_ready(flo_ctx *ctx, size_t n, flo_sdec *const *decs, uint32_t max_frames_per_stream, float *dst_device,
                                     size_t dst_cap_floats, uint64_t *offsets, int *status, void *stream) {
    if (!ctx) return FLO_ERR_ARG;
    if (!offsets) return fail(ctx, FLO_ERR_ARG, "null offsets");
    offsets[0] = 0;
    if (!n) return FLO_OK;
    if (!decs || !status) return fail(ctx, FLO_ERR_ARG, "null argument");
    {   // one decoder at most once per call: its plan starts from its counters
        std::vector<const flo_sdec *> v(decs, decs + n);
        std::sort(v.begin(), v.end());
        if (!v[0]) return fail(ctx, FLO_ERR_ARG, "null decoder");
        if (std::adjacent_find(v.begin(), v.end()) != v.end()) return fail(ctx, FLO_ERR_ARG, "a decoder appears twice in one call");
    }
    for (size_t i = 0; i < n; i++)
        if (decs[i]->ctx && decs[i]->ctx != ctx) return fail(ctx, FLO_ERR_ARG, "decoder " + std::to_string(i) + " belongs to another context");
    SdecWork *w = work(ctx);
    // a call right behind a sizing call over the same decoders, none changed since, takes its plans instead of parsing
    // every frame again
    bool reuse = w->sized && w->sized_cap == max_frames_per_stream && w->sized_decs.size() == n && w->plans.size() == n;
    for (size_t i = 0; reuse && i < n; i++) reuse = w->sized_decs[i] == decs[i] && w->sized_ver[i] == decs[i]->version;
    w->sized = false;
    if (!reuse) {
        w->plans.resize(n);
        for (size_t i = 0; i < n; i++) plan_frames(decs[i], max_frames_per_stream, w->plans[i]);
    }
    for (size_t i = 0; i < n; i++) {
        offsets[i + 1] = offsets[i] + w->plans[i].floats;
        status[i] = w->plans[i].status;
    }
    if (!dst_device) {   // sizing only: nothing decoded, nothing changed
        w->sized = true;
        w->sized_cap = max_frames_per_stream;
        w->sized_decs.assign(decs, decs + n);
        w->sized_ver.resize(n);
        for (size_t i = 0; i < n; i++) w->sized_ver[i] = decs[i]->version;
        return FLO_OK;
    }
    if (offsets[n] > dst_cap_floats) return fail(ctx, FLO_ERR_ARG, "destination too small for the decoded frames");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int rc = launch_plans(ctx, w, n, decs, offsets, dst_device, (hipStream_t)stream);
    if (rc != FLO_OK) {
        for (size_t i = 0; i < n; i++) decs[i]->stored = false;
        return rc;
    }
    for (size_t i = 0; i < n; i++) {
        commit_plan(decs[i], w->plans[i]);
        if (status[i] != FLO_OK) decs[i]->err = w->plans[i].err;
    }
    return FLO_OK;
}
