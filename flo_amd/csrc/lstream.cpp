// lstream.cpp — the lossy streaming encoder (flo_stream_create_lossy) and flo_stream_encode_ready: the new frames of many
// streams per device pass.
//
// Frame h of encode_to_flo covers input sample-frames [(h - 1) * 1024, (h + 1) * 1024) behind a 1024-frame zero pre-roll
// (lossy/encoder.rs:167-239), so it can be encoded once (h + 1) * 1024 sample-frames have been pushed. Across frames a
// stream carries only its last 1024 sample-frames and the temporal masking level of every (channel, Bark band),
// s_t = max(a_t, 0.7 s_(t-1)) (psychoacoustic.rs:196-203). Both stay on the host and go up with the new samples: a stream
// owns no device memory. One step per configuration (sample rate, channels, quality) of a call:
//   upload    ONE pinned copy: descriptors, carried levels and every stream's window (carried block + new frames)
//   kernels   pass 1 (a_t of the step's flat frame list), the seeded scan, pass 2 (frames into slots), compaction into
//             one contiguous run of bytes
//   read-back ONE copy of sizes, new levels and the bytes (a guess of their size: a larger result fetches its remainder)
// and the call synchronises once. The frame passes are the frame-parallel kernels' stream-step instantiations, so a
// stream's frames are byte for byte those of the offline encoder (tests/test_gpu_lossy_stream.py).
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "ctx_internal.hpp"
#include "devpool.hpp"
#include "lossy_kernels.hpp"

namespace {
constexpr size_t kStreamHop = 1024;
constexpr int kBands = 25;
// guessed bytes per frame and channel of the read-back (quality 0.55 makes about 210): a step whose frames are larger
// fetches the rest after the sync
constexpr size_t kGuessPerChannel = 384;

size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

uint32_t lossy_timestamp(uint64_t frame, uint32_t sr) {   // the TOC's floor(samples * 1000 / rate) (writer.rs:193-224)
    return (uint32_t)(frame * kStreamHop * 1000ull / sr);
}
}  // namespace

struct LstreamWork {
    void *dev = nullptr;   // every group's input, scratch and output of one call; grows to the largest call
    size_t cap = 0;
};

void lstream_work_free(flo_ctx *c) {
    LstreamWork *w = c ? c->lstream : nullptr;
    if (!w) return;
    hipStreamSynchronize(c->stream);
    if (w->dev) pool_free(w->dev);
    delete w;
    c->lstream = nullptr;
}

extern "C" int flo_stream_create_lossy(flo_ctx *c, uint32_t sample_rate, uint8_t channels, float quality, flo_stream **out) {
    if (!c || !out) return FLO_ERR_ARG;
    *out = nullptr;
    if (!sample_rate) return fail(c, FLO_ERR_ARG, "sample_rate must be non-zero");
    if (channels < 1 || channels > kMaxLossyChannels) return fail(c, FLO_ERR_ARG, "lossy encode on device supports 1 to 8 channels");
    // TransformEncoder::new: quality.clamp(0.0, 1.0) (NaN as get_tables treats it)
    const float q = quality != quality ? 0.f : (quality < 0.f ? 0.f : (quality > 1.f ? 1.f : quality));
    TableSet *ts = nullptr;
    int rc = get_tables(c, sample_rate, q, &ts);   // (made here, so that a step never builds tables)
    if (rc != FLO_OK) return rc;
    flo_stream *s = new flo_stream();
    s->ctx = c;
    s->sr = sample_rate;
    s->ch = channels;
    s->lossy = true;
    s->quality = q;
    s->carry.assign(kStreamHop * channels, 0.f);
    s->mask.assign((size_t)kBands * channels, 0.f);
    *out = s;
    return FLO_OK;
}

extern "C" int flo_stream_append(flo_stream *s, const float *samples, size_t n) {
    if (!s || (n && !samples)) return FLO_ERR_ARG;
    if (s->lossy && s->flushed) return fail(s->ctx, FLO_ERR_STATE, "the stream has been flushed: its input has ended");
    s->buf.insert(s->buf.end(), samples, samples + n);
    return FLO_OK;
}

namespace {
size_t lossy_ready_frames(const flo_stream *s) { return s->buf.size() / s->ch / kStreamHop; }
size_t lossless_ready_seconds(const flo_stream *s) { return s->buf.size() / ((size_t)s->sr * s->ch); }

// one configuration's step: upload, kernels and read-back are enqueued on the ctx stream; finish_group() after the sync
struct LossyGroup {
    std::vector<flo_stream *> st;
    std::vector<size_t> idx;   // positions in the call's stream list
    std::vector<uint32_t> k;   // new frames per stream
    unsigned nch = 0;
    TableSet *ts = nullptr;
    uint64_t frames = 0;
    size_t in_bytes = 0, work_bytes = 0, out_bytes = 0;
    // offsets inside the group's part of the device buffer
    size_t o_desc = 0, o_hops = 0, o_seed = 0, o_win = 0;      // input (one upload)
    size_t o_at = 0, o_bmax = 0, o_sprev = 0, o_slots = 0, o_foff = 0, o_inf = 0;
    size_t o_out = 0, r_lvl = 0, r_tot = 0, r_bytes = 0;       // output (one read-back): sizes | levels | total | bytes
    size_t guess = 0;      // bytes read back in the first copy
    uint8_t *dev = nullptr;
    void *pin_in = nullptr, *pin_out = nullptr;

    void layout() {
        const size_t S = st.size();
        frames = 0;
        uint64_t win = 0;
        for (uint32_t x : k) {
            frames += x;
            win += (x + 1) * kStreamHop * nch;
        }
        o_desc = 0;
        o_hops = al(o_desc + (3 * S + 2) * 8);
        o_seed = al(o_hops + (S + 1) * 4);
        o_win = al(o_seed + S * nch * kBands * 4);
        in_bytes = al(o_win + win * 4);
        const size_t lv = (size_t)frames * nch * 32 * 4;
        o_at = in_bytes;
        o_bmax = al(o_at + lv);
        o_sprev = al(o_bmax + lv);
        o_slots = al(o_sprev + lv);
        o_foff = al(o_slots + (size_t)frames * lossy_slot_bytes((int)nch));
        o_inf = al(o_foff + (frames + 1) * 8);   // LossyArgs::inf_mark, zeroed per step
        o_out = al(o_inf + S * nch * 32 * 8);
        work_bytes = o_out - in_bytes;
        r_lvl = al(frames * 4);
        r_tot = al(r_lvl + S * nch * kBands * 4);
        r_bytes = al(r_tot + 8);
        const size_t max_frame = 12 + 50 * (size_t)nch + (size_t)nch * (4 + 2064);
        out_bytes = al(r_bytes + (size_t)frames * max_frame + 64);
        guess = std::min((size_t)frames * (kGuessPerChannel * nch + 64), out_bytes - r_bytes);
    }
};

int release(flo_ctx *c, std::vector<LossyGroup> &groups, int rc) {
    for (LossyGroup &g : groups) {
        if (g.pin_in) stager_pinned_put(c->stager, g.pin_in);
        if (g.pin_out) stager_pinned_put(c->stager, g.pin_out);
        g.pin_in = g.pin_out = nullptr;
    }
    return rc;
}

int enqueue_group(flo_ctx *c, LossyGroup &g) {
    const size_t S = g.st.size();
    const unsigned nch = g.nch;
    std::string err;
    g.pin_in = stager_pinned_get(c->stager, g.in_bytes, err);
    if (!g.pin_in) return fail(c, FLO_ERR_NOMEM, err);
    g.pin_out = stager_pinned_get(c->stager, g.r_bytes + g.guess, err);
    if (!g.pin_out) return fail(c, FLO_ERR_NOMEM, err);
    uint8_t *pin = (uint8_t *)g.pin_in;
    // descriptors: window offset (floats), window sample-frames, first frame | the compaction's one-clip view: frame 0, DATA offset
    uint64_t *desc = (uint64_t *)(pin + g.o_desc);
    uint32_t *hops = (uint32_t *)(pin + g.o_hops);
    float *seed = (float *)(pin + g.o_seed);
    float *win = (float *)(pin + g.o_win);
    std::vector<UploadSeg> fill;
    uint64_t woff = 0, f0 = 0;
    uint32_t max_k = 0;
    for (size_t i = 0; i < S; i++) {
        const flo_stream *s = g.st[i];
        const uint32_t k = g.k[i];
        desc[i] = woff;
        desc[S + i] = (uint64_t)(k + 1) * kStreamHop;
        desc[2 * S + i] = f0;
        hops[i] = k;
        memcpy(seed + i * nch * kBands, s->mask.data(), nch * kBands * 4);
        fill.push_back({win + woff, s->carry.data(), kStreamHop * nch * 4});
        fill.push_back({win + woff + kStreamHop * nch, s->buf.data(), (size_t)k * kStreamHop * nch * 4});
        woff += (uint64_t)(k + 1) * kStreamHop * nch;
        f0 += k;
        max_k = std::max(max_k, k);
    }
    desc[3 * S] = 0;
    desc[3 * S + 1] = 0;
    hops[S] = (uint32_t)g.frames;
    stager_memcpy_many(c->stager, fill);
    uint8_t *d = g.dev;
    HIPCHK(c, hipMemcpyAsync(d, pin, g.in_bytes, hipMemcpyHostToDevice, c->stream));

    LossyArgs A{};
    A.T = g.ts->dev;
    A.pcm = (const float *)(d + g.o_win);
    const unsigned long long *dd = (const unsigned long long *)(d + g.o_desc);
    A.clip_off = dd;
    A.clip_nsf = dd + S;
    A.clip_frame0 = dd + 2 * S;
    A.clip_hops = (const unsigned *)(d + g.o_hops);
    A.nch = (int)nch;
    A.n_clips = (int)S;
    A.total_frames = g.frames;
    A.max_hops = max_k;
    uint8_t *out = d + g.o_out;
    A.frame_size = (unsigned *)out;
    A.a_t = (float *)(d + g.o_at);
    A.bmax_t = (float *)(d + g.o_bmax);
    A.s_prev_out = (float *)(d + g.o_sprev);
    A.s_prev = A.s_prev_out;
    A.slots = d + g.o_slots;
    A.slot_bytes = lossy_slot_bytes((int)nch);
    A.frame_off = (unsigned long long *)(d + g.o_foff);
    A.n_cus = c->prop.multiProcessorCount;
    A.exact = lossy_exact(false, A.T);
    A.inf_mark = (unsigned long long *)(d + g.o_inf);
    A.inf_tag = 1;
    HIPCHK(c, hipMemsetAsync(A.inf_mark, 0, S * nch * 32 * 8, c->stream));
    const float *d_seed = (const float *)(d + g.o_seed);
    float *d_lvl = (float *)(out + g.r_lvl);
    int rc;
    if ((rc = timed_launch(c, "lstream_bands", [&] { return launch_lossy_stream_pass(A, 1, c->stream); })) != FLO_OK) return rc;
    if ((rc = timed_launch(c, "lstream_scan", [&] { return launch_lossy_stream_scan(A, d_seed, d_lvl, c->stream); })) != FLO_OK) return rc;
    if ((rc = timed_launch(c, "lstream_frames", [&] { return launch_lossy_stream_pass(A, 2, c->stream); })) != FLO_OK) return rc;
    // compaction: the step's frames as ONE clip of the batch kernels, its DATA chunk right behind the read-back header
    LossyArgs K = A;
    K.n_clips = 1;
    K.clip_frame0 = dd + 3 * S;
    K.out_off = dd + 3 * S + 1;
    K.clip_hops = A.clip_hops + S;
    K.max_hops = (unsigned)g.frames;
    K.out = out + g.r_bytes;
    K.clip_bytes = (unsigned long long *)(out + g.r_tot);
    const CompactKernel ck = g.frames <= 4096 ? CompactKernel::Fused : CompactKernel::Offsets1024;
    if ((rc = timed_launch(c, "lstream_compact", [&] { return launch_lossy_compact(K, ck, c->stream); })) != FLO_OK) return rc;
    HIPCHK(c, hipMemcpyAsync(g.pin_out, out, g.r_bytes + g.guess, hipMemcpyDeviceToHost, c->stream));
    return FLO_OK;
}

// after the sync: frames to the streams' queues, carried block and levels forward, consumed samples out of the buffers
int finish_group(flo_ctx *c, LossyGroup &g) {
    const size_t S = g.st.size();
    const unsigned nch = g.nch;
    const uint8_t *o = (const uint8_t *)g.pin_out;
    const uint32_t *sizes = (const uint32_t *)o;
    const float *lvl = (const float *)(o + g.r_lvl);
    uint64_t total = 0;
    memcpy(&total, o + g.r_tot, 8);
    uint64_t sum = 0;
    const uint32_t slot = lossy_slot_bytes((int)nch);
    for (uint64_t f = 0; f < g.frames; f++) {
        if (sizes[f] > slot) return fail(c, FLO_ERR_DEVICE, "a stream frame overran its slot");
        sum += sizes[f];
    }
    if (sum != total || g.r_bytes + total > g.out_bytes) return fail(c, FLO_ERR_DEVICE, "stream step: frame sizes and DATA size disagree");
    std::vector<uint8_t> rest;
    const uint8_t *bytes = o + g.r_bytes;
    if (total > g.guess) {   // larger than the guess: the remainder in a second copy
        rest.resize(total);
        memcpy(rest.data(), bytes, g.guess);
        HIPCHK(c, hipMemcpy(rest.data() + g.guess, g.dev + g.o_out + g.r_bytes + g.guess, total - g.guess, hipMemcpyDeviceToHost));
        bytes = rest.data();
    }
    uint64_t f = 0, pos = 0;
    for (size_t i = 0; i < S; i++) {
        flo_stream *s = g.st[i];
        const uint32_t k = g.k[i];
        for (uint32_t j = 0; j < k; j++, f++) {
            StreamFrame fr;
            fr.index = s->frame_index;
            fr.timestamp_ms = lossy_timestamp(s->frame_index, s->sr);
            fr.samples = (uint32_t)kStreamHop;
            fr.data.assign(bytes + pos, bytes + pos + sizes[f]);
            pos += sizes[f];
            s->pending.push_back(std::move(fr));
            s->frame_index++;
            s->total_samples += kStreamHop;
        }
        const size_t used = (size_t)k * kStreamHop * nch;
        memcpy(s->carry.data(), s->buf.data() + used - kStreamHop * nch, kStreamHop * nch * 4);
        memcpy(s->mask.data(), lvl + i * nch * kBands, nch * kBands * 4);
        s->buf.erase(s->buf.begin(), s->buf.begin() + used);
    }
    return FLO_OK;
}
}  // namespace

extern "C" int flo_stream_encode_ready(flo_ctx *c, size_t n, flo_stream *const *streams, int *status) {
    if (!c) return FLO_ERR_ARG;
    if (!n) return FLO_OK;
    if (!streams || !status) return fail(c, FLO_ERR_ARG, "null argument");
    {
        std::vector<const flo_stream *> v(streams, streams + n);
        std::sort(v.begin(), v.end());
        if (!v[0]) return fail(c, FLO_ERR_ARG, "null stream");
        if (std::adjacent_find(v.begin(), v.end()) != v.end()) return fail(c, FLO_ERR_ARG, "a stream appears twice in one call");
    }
    HIPCHK(c, hipSetDevice(c->device));
    int first_err = FLO_OK;
    auto set = [&](size_t i, int rc) {
        status[i] = rc;
        if (rc != FLO_OK && first_err == FLO_OK) first_err = rc;
    };
    // configuration groups, in order of first appearance
    std::map<std::tuple<uint32_t, unsigned, float>, size_t> lossy_key;
    std::map<std::tuple<uint32_t, unsigned, unsigned, unsigned>, size_t> ll_key;
    std::vector<LossyGroup> groups;
    std::vector<std::vector<std::pair<flo_stream *, size_t>>> ll_groups;
    std::vector<std::vector<size_t>> ll_idx;
    for (size_t i = 0; i < n; i++) {
        flo_stream *s = streams[i];
        status[i] = FLO_OK;
        if (s->ctx != c) {
            set(i, fail(c, FLO_ERR_ARG, "stream " + std::to_string(i) + " belongs to another context"));
            continue;
        }
        if (s->lossy) {
            const size_t k = lossy_ready_frames(s);
            if (!k) continue;
            auto key = std::make_tuple(s->sr, (unsigned)s->ch, s->quality);
            auto it = lossy_key.find(key);
            if (it == lossy_key.end()) {
                it = lossy_key.emplace(key, groups.size()).first;
                groups.emplace_back();
                groups.back().nch = s->ch;
                int rc = get_tables(c, s->sr, s->quality, &groups.back().ts);
                if (rc != FLO_OK) return rc;
            }
            LossyGroup &g = groups[it->second];
            g.st.push_back(s);
            g.idx.push_back(i);
            g.k.push_back((uint32_t)k);
        } else {
            const size_t secs = lossless_ready_seconds(s);
            if (!secs) continue;
            auto key = std::make_tuple(s->sr, (unsigned)s->ch, (unsigned)s->bit_depth, (unsigned)s->level);
            auto it = ll_key.find(key);
            if (it == ll_key.end()) {
                it = ll_key.emplace(key, ll_groups.size()).first;
                ll_groups.emplace_back();
                ll_idx.emplace_back();
            }
            ll_groups[it->second].push_back({s, secs});
            ll_idx[it->second].push_back(i);
        }
    }
    if (!groups.empty()) {
        int rc = ctx_stager(c);
        if (rc != FLO_OK) return rc;
        size_t need = 0;
        for (LossyGroup &g : groups) {
            g.layout();
            need += g.in_bytes + g.work_bytes + g.out_bytes;
        }
        LstreamWork *w = c->lstream ? c->lstream : (c->lstream = new LstreamWork());
        if (need > w->cap) {   // scratch grows to the largest call (the stream is idle behind the previous call's sync)
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (w->dev) pool_free(w->dev);
            w->dev = nullptr;
            w->cap = 0;
            const size_t cap = need + need / 4;
            hipError_t e = pool_alloc(&w->dev, cap);
            if (e != hipSuccess) return fail(c, e == hipErrorOutOfMemory ? FLO_ERR_NOMEM : FLO_ERR_DEVICE, "stream step scratch");
            w->cap = cap;
        }
        size_t off = 0;
        for (LossyGroup &g : groups) {
            g.dev = (uint8_t *)w->dev + off;
            off += g.in_bytes + g.work_bytes + g.out_bytes;
        }
        // every group's step is enqueued, then ONE sync
        for (LossyGroup &g : groups) {
            rc = enqueue_group(c, g);
            if (rc != FLO_OK) {
                hipStreamSynchronize(c->stream);
                return release(c, groups, rc);
            }
        }
        const hipError_t e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return release(c, groups, fail(c, FLO_ERR_DEVICE, std::string("stream step: ") + hipGetErrorString(e)));
        for (LossyGroup &g : groups) {
            const int grc = finish_group(c, g);
            for (size_t i : g.idx) set(i, grc);
        }
        release(c, groups, FLO_OK);
    }
    for (size_t gi = 0; gi < ll_groups.size(); gi++) {   // lossless: one batch per configuration, as flo_stream_push's
        std::vector<std::vector<uint8_t>> frames;
        const int rc = stream_encode_lossless(c, ll_groups[gi], frames);
        size_t first = 0;
        for (size_t j = 0; j < ll_groups[gi].size(); j++) {
            if (rc == FLO_OK) {
                stream_queue_lossless(ll_groups[gi][j].first, frames, first, ll_groups[gi][j].second);
                first += ll_groups[gi][j].second;
            }
            set(ll_idx[gi][j], rc);
        }
    }
    return first_err;
}

// flo_stream_push of a lossy stream: append, then the stream's complete frames in a step of its own
int lossy_stream_push(flo_stream *s, const float *samples, size_t n) {
    int rc = flo_stream_append(s, samples, n);
    if (rc != FLO_OK) return rc;
    int st = FLO_OK;
    rc = flo_stream_encode_ready(s->ctx, 1, &s, &st);
    return rc != FLO_OK ? rc : st;
}

// the end of a lossy stream's input (flush / finalize): the partial sample-frame is dropped (encoder.rs:174) and the
// zero padding of encode_to_flo's last one or two frames is appended (encoder.rs:177-185), which completes them
int lossy_stream_end(flo_stream *s) {
    if (s->flushed) return FLO_OK;
    const size_t sf = s->buf.size() / s->ch;
    const std::vector<float> part(s->buf.begin() + sf * s->ch, s->buf.end());
    const size_t frames = sf / kStreamHop + 1 + (sf % kStreamHop ? 1 : 0);
    s->buf.resize(sf * s->ch);
    s->buf.resize(frames * kStreamHop * s->ch, 0.f);
    int st = FLO_OK;
    int rc = flo_stream_encode_ready(s->ctx, 1, &s, &st);
    if (rc == FLO_OK) rc = st;
    if (rc != FLO_OK) {   // (a failed step consumed nothing: the input is as it was)
        s->buf.resize(sf * s->ch);
        s->buf.insert(s->buf.end(), part.begin(), part.end());
        return rc;
    }
    s->flushed = true;
    return FLO_OK;
}
