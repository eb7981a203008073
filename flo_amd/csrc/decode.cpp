// decode.cpp — file and batch decode (flo_probe_container, flo_decode*, flo_batch_decode, flo_decode_frame_at): parse on
// the host, decode on the device. Host code only; the kernels live in decode_kernels.hip / lldec_kernels.hip.
#include <sys/mman.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "batch_internal.hpp"
#include "container.hpp"
#include "decode_kernels.hpp"
#include "decode_plan.hpp"
#include "devmem.hpp"

// A decoded file's PCM goes to the caller in fresh memory (flo_free = free). A fresh 60 MB of 4 KB pages is 15 000 page
// faults under the copy that fills it - 30 ms for a 3-minute file whose kernels take 1 ms - so large results are asked for
// in transparent huge pages (2 MB alignment + MADV_HUGEPAGE: a hint; where the host does not honour it nothing changes).
static void *alloc_result(size_t bytes) {
    if (bytes < ((size_t)4 << 20)) return malloc(bytes ? bytes : 1);
    void *p = nullptr;
    if (posix_memalign(&p, (size_t)2 << 20, bytes) != 0) return malloc(bytes);
    madvise(p, bytes, MADV_HUGEPAGE);
    return p;
}
// a result on its way to the caller: freed on every return but the one that releases it
using HostResult = std::unique_ptr<void, decltype(&free)>;

template <class T>
static int upload(flo_ctx *c, DevMem &m, const std::vector<T> &v) {
    size_t bytes = v.size() * sizeof(T);
    HIPCHK(c, pool_alloc(&m.p, bytes ? bytes : 16));
    if (bytes) HIPCHK(c, hipMemcpyAsync(m.p, v.data(), bytes, hipMemcpyHostToDevice, c->stream));
    return FLO_OK;
}

extern "C" int flo_probe_container(const uint8_t *flo, size_t len, flo_container_info *out, char *err, size_t err_cap) {
    if (!out || (!flo && len)) return FLO_ERR_ARG;
    memset(out, 0, sizeof *out);
    if (err && err_cap) err[0] = 0;
    ParsedFile f;
    const char *perr = "";
    if (parse_file(flo, len, f, &perr) != 0) {
        if (err && err_cap) snprintf(err, err_cap, "%s", perr);
        return FLO_ERR_FORMAT;
    }
    out->version_major = f.version_major;
    out->version_minor = f.version_minor;
    out->channels = f.channels;
    out->bit_depth = f.bit_depth;
    out->compression_level = f.compression_level;
    out->is_transform = f.is_transform ? 1 : 0;
    out->flags = f.flags;
    out->sample_rate = f.sample_rate;
    out->data_crc32 = f.data_crc32;
    out->n_frames = (uint32_t)f.frames.size();
    out->total_samples = f.total_samples;
    out->data_start = f.data_start;
    out->data_size = f.data_size;
    for (const FrameDesc &fr : f.frames) out->frame_samples_sum += fr.samples;
    return FLO_OK;
}

// Device -> caller-owned pageable memory. A copy engine writes pageable memory at a fraction of the PCIe rate, so a
// large result comes down in 8 MiB pieces through two pinned buffers: while the copy threads move piece i into the
// caller's buffer, the copy engine is already filling the other pinned buffer with piece i + 1.
static int download(flo_ctx *c, void *dst, const void *d_src, size_t bytes) {
    constexpr size_t kPieceBytes = 8u << 20;
    if (bytes <= kPieceBytes / 2) {
        HIPCHK(c, hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return FLO_OK;
    }
    int rc = ctx_stager(c);
    if (rc != FLO_OK) return rc;
    std::string err;
    void *pin[2] = {stager_pinned_get(c->stager, kPieceBytes, err), stager_pinned_get(c->stager, kPieceBytes, err)};
    hipEvent_t ev[2] = {nullptr, nullptr};
    auto done = [&](int r) {
        for (int i = 0; i < 2; i++) {
            if (pin[i]) stager_pinned_put(c->stager, pin[i]);
            if (ev[i]) hipEventDestroy(ev[i]);
        }
        return r;
    };
    if (!pin[0] || !pin[1]) return done(fail(c, FLO_ERR_NOMEM, err));
    for (int i = 0; i < 2; i++)
        if (hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) != hipSuccess) return done(fail(c, FLO_ERR_DEVICE, "hipEventCreate failed"));
    const size_t pieces = (bytes + kPieceBytes - 1) / kPieceBytes;
    auto issue = [&](size_t i) -> hipError_t {
        const size_t off = i * kPieceBytes, n = bytes - off < kPieceBytes ? bytes - off : kPieceBytes;
        hipError_t e = hipMemcpyAsync(pin[i & 1], (const char *)d_src + off, n, hipMemcpyDeviceToHost, c->stream);
        return e == hipSuccess ? hipEventRecord(ev[i & 1], c->stream) : e;
    };
    hipError_t e = issue(0);
    if (e == hipSuccess && pieces > 1) e = issue(1);
    for (size_t i = 0; i < pieces && e == hipSuccess; i++) {
        const size_t off = i * kPieceBytes, n = bytes - off < kPieceBytes ? bytes - off : kPieceBytes;
        e = hipEventSynchronize(ev[i & 1]);
        if (e != hipSuccess) break;
        stager_memcpy_many(c->stager, {{(char *)dst + off, pin[i & 1], n}});
        if (i + 2 < pieces) e = issue(i + 2);
    }
    if (e != hipSuccess) return done(fail(c, FLO_ERR_DEVICE, std::string("download: ") + hipGetErrorString(e)));
    return done(FLO_OK);
}

// FLO_LL_DECODE_SERIAL: every wrapper to the serial kernel (read once per decode call)
static bool ll_force_serial() { return getenv("FLO_LL_DECODE_SERIAL") != nullptr; }

// Frame `fr` of a parsed lossless file whose bytes start the device buffer, to sample-frame `out_off` of the output
// (lossless/decoder.rs:21-72).
static void add_parsed_frame(LlWrapperList &w, const ParsedFile &f, const FrameDesc &fr, uint64_t out_off, bool force_serial) {
    w.add_frame(out_off, fr.samples, f.channels == 2 && (fr.flags & 1), fr.n_channels, force_serial, [&](unsigned k) {
        const ChannelDesc &cd = f.channels_desc[fr.first_channel + k];
        return ll_channel(cd.off, cd.len, cd.n_coeffs, cd.shift_bits, cd.rice_k, cd.coeffs);
    });
}
uint64_t file_ll_wrappers(const ParsedFile &f, LlWrapperList &w) {
    uint64_t out_sf = 0;
    const bool force_serial = ll_force_serial();
    for (const FrameDesc &fr : f.frames) {
        add_parsed_frame(w, f, fr, out_sf, force_serial);
        out_sf += fr.samples;
    }
    return out_sf;
}
void file_transform_blobs(const ParsedFile &f, std::vector<unsigned long long> &blob_off, std::vector<unsigned int> &blob_len) {
    for (const FrameDesc &fr : f.frames) {
        if (!fr.n_channels) continue;
        const ChannelDesc &cd = f.channels_desc[fr.first_channel];
        blob_off.push_back(cd.off);
        blob_len.push_back(cd.len);
    }
}

int ll_decode_device(flo_ctx *c, const LlWrapperList &w, uint64_t out_sf, const uint8_t *d_bytes, int nch, float *d_out, int *d_out_i32) {
    const size_t n_out = (size_t)out_sf * (size_t)nch;
    if (!n_out) return FLO_OK;
    const auto t_enter = std::chrono::steady_clock::now();
    DevMem d_desc, d_scr, d_tabs, d_ent;
    QuiesceOnExit quiesce_d_desc(c);
    int rc;
    if (getenv("FLO_TRACE")) {
        size_t lpc = 0, lpc8 = 0, fixed = 0, other = 0, ser = 0;
        for (size_t i = 0; i < w.chs.size(); i++) {
            const LlChannelDev &d = w.chs[i];
            if (w.serial[i]) ser++;
            else if (d.n_coeffs && d.len) (d.n_coeffs <= 8 ? lpc8 : lpc)++;
            else if (d.len && d.shift_bits >= 128) fixed++;
            else other++;
        }
        fprintf(stderr, "[flo] ll decode: %zu wrappers: LPC order <= 8 %zu, order 9..12 %zu, fixed %zu, raw/silent/empty %zu, serial %zu\n", w.chs.size(), lpc8,
                lpc, fixed, other, ser);
    }
    // the descriptor arrays go up as ONE copy out of pinned memory, queued in front of the kernels (a copy per array out
    // of pageable vectors each held the host until the driver had staged them: 0.15 ms of an idle device per call)
    enum { kCh, kFr, kT0, kSer, kOth };
    const DescBlock blk{desc_part(w.chs), desc_part(w.frs), desc_part(w.tile0), desc_part(w.serial), desc_part(w.others)};
    if ((rc = ctx_stager(c)) != FLO_OK) return rc;
    {
        std::string perr;
        uint8_t *pin = (uint8_t *)stager_pinned(c->stager, blk.bytes, perr);
        if (!pin) return fail(c, FLO_ERR_NOMEM, perr);
        blk.fill(pin);
        HIPCHK(c, pool_alloc(&d_desc.p, blk.bytes));
        HIPCHK(c, hipMemcpyAsync(d_desc.p, pin, blk.bytes, hipMemcpyHostToDevice, c->stream));   // (read before this function's final synchronise)
    }
    const LlChannelDev *const d_ch = blk.at<const LlChannelDev>(d_desc.p, kCh);
    const size_t tiles = w.tiles();
    hipError_t e = pool_alloc(&d_scr.p, w.scratch ? w.scratch * sizeof(int) : 16);
    if (e == hipSuccess) e = pool_alloc(&d_tabs.p, tiles ? tiles * kRiceStates * sizeof(unsigned int) : 16);
    if (e == hipSuccess) e = pool_alloc(&d_ent.p, tiles ? tiles * sizeof(uint2) : 16);
    // the output is cleared only when some frame carries fewer channels than the file (ll_finish writes every sample
    // of every channel a frame has; the scratch needs no clearing: each wrapper's kernels write all of its samples)
    bool partial = false;
    for (const LlFrameDev &fd : w.frs)
        if ((int)fd.n_channels < nch) partial = true;
    if (e == hipSuccess && d_out && partial) e = hipMemsetAsync(d_out, 0, n_out * sizeof(float), c->stream);
    if (e == hipSuccess && d_out_i32 && partial) e = hipMemsetAsync(d_out_i32, 0, n_out * sizeof(int), c->stream);
    if (e != hipSuccess) return fail(c, FLO_ERR_NOMEM, std::string("decode buffers: ") + hipGetErrorString(e));
    rc = launch_ll_wrappers(c, w, d_bytes, d_ch, blk.at<const unsigned int>(d_desc.p, kT0), blk.at<int>(d_desc.p, kSer),
                            blk.at<const unsigned int>(d_desc.p, kOth), d_scr.as<int>(), d_tabs.as<unsigned int>(), d_ent.as<uint2>(),
                            "ll_decode_parallel", "ll_decode");
    if (rc != FLO_OK) return rc;
    LlFinishArgs F{blk.at<const LlFrameDev>(d_desc.p, kFr), d_ch, (unsigned)w.frs.size(), nch, d_scr.as<int>(), d_out, d_out_i32};
    rc = timed_launch(c, "ll_finish", [&] { return launch_ll_finish(F, w.max_samples, c->stream); });
    if (rc != FLO_OK) return rc;
    if (getenv("FLO_TRACE"))
        fprintf(stderr, "[flo] ll decode: host time until the last launch %.0f us\n",
                (double)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_enter).count() / 1e3);
    // the temporaries go back to the pool
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (getenv("FLO_TRACE")) {
        // the serial flags as the kernels left them: what the host set, plus the wrappers the parallel form gave up
        // (a 256-ones escape, a sample outside i32); read before the descriptor block returns to the pool
        std::vector<int> flags(w.serial.size());
        if (!flags.empty()) HIPCHK(c, hipMemcpy(flags.data(), blk.at<int>(d_desc.p, kSer), flags.size() * sizeof(int), hipMemcpyDeviceToHost));
        size_t by_host = 0, by_device = 0;
        for (size_t i = 0; i < flags.size(); i++) {
            if (w.serial[i]) by_host++;
            else if (flags[i]) by_device++;
        }
        fprintf(stderr, "[flo] ll decode: serial by the host %zu, by the device %zu\n", by_host, by_device);
    }
    return FLO_OK;
}

int lossy_decode_whole(flo_ctx *c, const TableSet *ts, const uint8_t *bytes, int channels, const std::vector<unsigned long long> &blob_off,
                       const std::vector<unsigned int> &blob_len, const std::vector<unsigned long long> &clip_frame0,
                       const std::vector<unsigned int> &clip_frames, const std::vector<unsigned long long> &clip_out,
                       unsigned max_frames, float *out, const LossyCmpArgs *cmp, unsigned lead) {
    DevMem d_off, d_len, d_c0, d_cn, d_co, d_err;
    QuiesceOnExit quiesce_d_off(c);
    const std::vector<int> zero{0};
    int rc;
    if ((rc = upload(c, d_off, blob_off)) || (rc = upload(c, d_len, blob_len)) || (rc = upload(c, d_c0, clip_frame0)) ||
        (rc = upload(c, d_cn, clip_frames)) || (rc = upload(c, d_co, clip_out)) || (rc = upload(c, d_err, zero)))
        return rc;
    LossyDecArgs A{};
    A.T = ts->dev;
    A.window = ts->dev_window;
    A.bytes = bytes;
    A.blob_off = d_off.as<unsigned long long>();
    A.blob_len = d_len.as<unsigned int>();
    A.clip_frame0 = d_c0.as<unsigned long long>();
    A.clip_frames = d_cn.as<unsigned int>();
    A.clip_out = d_co.as<unsigned long long>();
    A.n_clips = (int)clip_frame0.size();
    A.channels = channels;
    A.out = out;
    A.error = d_err.as<int>();
    A.lead = lead;
    if (cmp) {
        A.cmp = *cmp;
        if ((rc = timed_launch(c, "fidelity", [&] { return launch_lossy_compare(A, max_frames, c->stream); })) != FLO_OK) return rc;
    } else if ((rc = timed_launch(c, "lossy_decode", [&] { return launch_lossy_decode(A, max_frames, c->stream); })) != FLO_OK) {
        return rc;
    }
    int herr = 0;
    HIPCHK(c, hipMemcpyAsync(&herr, d_err.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (herr) return fail(c, FLO_ERR_FORMAT, "Failed to deserialize transform frame");
    return FLO_OK;
}

// libflo::decode (lib.rs:296-315): parse on the host (a few bytes per frame), decode on the device.
static int decode_impl(flo_ctx *c, const uint8_t *flo, size_t len, float **pcm, int32_t **pcm_i32, size_t *n_interleaved,
                       uint32_t *sample_rate, uint8_t *channels) {
    if (!c || !flo || !n_interleaved || (!pcm && !pcm_i32)) return fail(c, FLO_ERR_ARG, "null argument");
    if (pcm) *pcm = nullptr;
    if (pcm_i32) *pcm_i32 = nullptr;
    *n_interleaved = 0;
    HIPCHK(c, hipSetDevice(c->device));
    ParsedFile f;
    const char *perr = "";
    if (parse_file(flo, len, f, &perr) != 0) return fail(c, FLO_ERR_FORMAT, perr);
    if (sample_rate) *sample_rate = f.sample_rate;
    if (channels) *channels = f.channels;
    const int nch = f.channels;
    DevMem d_bytes;
    QuiesceOnExit quiesce_d_bytes(c);
    HIPCHK(c, pool_alloc(&d_bytes.p, len + 32));
    {
        int rc = ctx_stager(c);
        if (rc != FLO_OK) return rc;
        std::string uerr;
        if (stager_upload(c->stager, {{d_bytes.p, flo, len}}, c->stream, uerr) != 0) return fail(c, FLO_ERR_DEVICE, uerr);
    }

    if (f.is_transform) {
        if (pcm_i32 && !pcm) return fail(c, FLO_ERR_ARG, "integer output exists for lossless files only");
        // decode_transform_file (lib.rs:325-352): frames without channels are skipped, the first decoded frame is dropped
        std::vector<unsigned long long> blob_off;
        std::vector<unsigned int> blob_len;
        file_transform_blobs(f, blob_off, blob_len);
        const size_t nf = blob_off.size();
        const size_t n_out = nf > 1 ? (nf - 1) * 1024 * (size_t)nch : 0;
        HostResult host(alloc_result(n_out * sizeof(float)), free);
        if (!host) return fail(c, FLO_ERR_NOMEM, "out of host memory");
        if (nf) {
            if (nch == 0) return fail(c, FLO_ERR_FORMAT, "Failed to deserialize transform frame");
            TableSet *ts;
            int rc = get_tables(c, f.sample_rate, 0.5f, &ts);
            if (rc != FLO_OK) return rc;
            DevMem d_out;
            QuiesceOnExit quiesce_d_out(c);
            hipError_t e = pool_alloc(&d_out.p, n_out ? n_out * sizeof(float) : 16);
            // (no clearing: the decode kernel writes every sample of every output block exactly once)
            if (e != hipSuccess) return fail(c, FLO_ERR_NOMEM, std::string("decode output: ") + hipGetErrorString(e));
            rc = lossy_decode_whole(c, ts, d_bytes.as<uint8_t>(), nch, blob_off, blob_len, {0}, {(unsigned int)nf}, {0}, (unsigned)nf, d_out.as<float>());
            if (rc == FLO_OK && n_out) rc = download(c, host.get(), d_out.p, n_out * sizeof(float));
            if (rc != FLO_OK) return rc;
        }
        *pcm = (float *)host.release();
        *n_interleaved = n_out;
        return FLO_OK;
    }

    // lossless (lossless/decoder.rs:21-72)
    LlWrapperList w;
    const uint64_t out_sf = file_ll_wrappers(f, w);
    const size_t n_out = nch ? (size_t)out_sf * (size_t)nch : 0;
    HostResult host(pcm ? alloc_result(n_out * sizeof(float)) : nullptr, free);
    HostResult host_i(pcm_i32 ? alloc_result(n_out * sizeof(int32_t)) : nullptr, free);
    if ((pcm && !host) || (pcm_i32 && !host_i)) return fail(c, FLO_ERR_NOMEM, "out of host memory");
    if (n_out) {
        DevMem d_out, d_outi;
        QuiesceOnExit quiesce_d_out(c);
        int rc;
        hipError_t e = hipSuccess;
        if (host) e = pool_alloc(&d_out.p, n_out * sizeof(float));
        if (e == hipSuccess && host_i) e = pool_alloc(&d_outi.p, n_out * sizeof(int));
        if (e != hipSuccess) return fail(c, FLO_ERR_NOMEM, std::string("decode buffers: ") + hipGetErrorString(e));
        if ((rc = ll_decode_device(c, w, out_sf, d_bytes.as<uint8_t>(), nch, d_out.as<float>(), d_outi.as<int>())) != FLO_OK) return rc;
        if (host && (rc = download(c, host.get(), d_out.p, n_out * sizeof(float))) != FLO_OK) return rc;
        if (host_i && (rc = download(c, host_i.get(), d_outi.p, n_out * sizeof(int))) != FLO_OK) return rc;
        e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return fail(c, FLO_ERR_DEVICE, std::string("lossless decode: ") + hipGetErrorString(e));
    }
    if (pcm) *pcm = (float *)host.release();
    if (pcm_i32) *pcm_i32 = (int32_t *)host_i.release();
    *n_interleaved = n_out;
    return FLO_OK;
}

// Lossless batches: the finished files stay where the encoder left them in HBM, and what a reader would find in them
// is known from the encoder's own frame and channel records (lossless_describe): nothing is read back or parsed, every
// wrapper of every clip is decoded in one set of launches.
static int batch_decode_lossless(flo_batch *b, float *dst, size_t dst_cap, uint64_t *offsets) {
    flo_ctx *c = b->ctx;
    std::vector<LosslessFrameInfo> fr;
    std::vector<LosslessWrapperInfo> wr;
    const uint8_t *base = nullptr;
    std::string err;
    const bool trace = getenv("FLO_TRACE") != nullptr;
    const auto t_0 = std::chrono::steady_clock::now();
    if (lossless_describe(b->ll, fr, wr, &base, err) != 0) return fail(c, FLO_ERR_STATE, err);
    const auto t_1 = std::chrono::steady_clock::now();
    LlWrapperList w;
    w.chs.reserve(wr.size());
    w.frs.reserve(fr.size());
    uint64_t out_sf = 0;
    const bool force_serial = ll_force_serial();
    for (size_t i = 0; i < b->n_clips; i++) offsets[i] = 0;
    uint32_t cur = 0xFFFFFFFFu;
    for (const LosslessFrameInfo &f : fr) {
        if (f.clip != cur) {   // frames are in clip order: a clip's PCM starts where its first frame's does
            cur = f.clip;
            if (cur < b->n_clips) offsets[cur] = out_sf * b->ch;
        }
        w.add_frame(out_sf, f.samples, b->ch == 2 && (f.flags & 1), f.n_wrappers, force_serial, [&](unsigned k) {
            const LosslessWrapperInfo &x = wr[f.first_wrapper + k];
            return ll_channel(x.off, x.len, x.n_coeffs, x.shift_bits, x.rice_k, x.coeffs);
        });
        out_sf += f.samples;
    }
    // clips without frames (empty input) keep the offset of whatever follows them
    {
        uint64_t next = out_sf * b->ch;
        std::vector<char> has(b->n_clips, 0);
        for (const LosslessFrameInfo &f : fr)
            if (f.clip < b->n_clips) has[f.clip] = 1;
        for (size_t i = b->n_clips; i-- > 0;) {
            if (has[i]) next = offsets[i];
            else offsets[i] = next;
        }
    }
    const uint64_t total = out_sf * b->ch;
    if (total > dst_cap) return fail(c, FLO_ERR_ARG, "destination too small for the decoded batch");
    const auto t_2 = std::chrono::steady_clock::now();
    const int rc = ll_decode_device(c, w, out_sf, base, b->ch, dst, nullptr);
    if (trace) {
        const auto t_3 = std::chrono::steady_clock::now();
        auto us = [](auto a, auto b2) { return (double)std::chrono::duration_cast<std::chrono::nanoseconds>(b2 - a).count() / 1e3; };
        fprintf(stderr, "[flo] batch lossless decode: describe %.0f us, descriptors %.0f us, device %.0f us\n", us(t_0, t_1), us(t_1, t_2), us(t_2, t_3));
    }
    return rc;
}

int batch_lossy_tables(flo_batch *b, std::vector<unsigned long long> &blob_off, std::vector<unsigned int> &blob_len,
                       std::vector<unsigned long long> &c0, std::vector<unsigned int> &cn, std::vector<unsigned long long> &co,
                       uint64_t &total, unsigned &max_hops) {
    flo_ctx *c = b->ctx;
    if (b->h_frame_size.size() != b->total_frames) {
        b->h_frame_size.assign(b->total_frames, 0);
        if (b->total_frames)
            HIPCHK(c, hipMemcpy(b->h_frame_size.data(), b->d_frame_size, b->total_frames * 4, hipMemcpyDeviceToHost));
    }
    blob_off.assign(b->total_frames, 0);
    blob_len.assign(b->total_frames, 0);
    c0.assign(b->n_clips, 0);
    cn.assign(b->n_clips, 0);
    co.assign(b->n_clips, 0);
    total = 0;
    max_hops = 0;
    for (size_t i = 0; i < b->n_clips; i++) {
        uint64_t off = b->out_off[i];
        for (uint32_t h = 0; h < b->hops[i]; h++) {
            const uint32_t fs = b->h_frame_size[b->clip_frame0[i] + h];
            if (fs < 10) return fail(c, FLO_ERR_STATE, "batch holds a frame shorter than its header");
            blob_off[b->clip_frame0[i] + h] = off + 10;   // [type][u32 samples][flags][u32 size] (writer.rs:236-254)
            blob_len[b->clip_frame0[i] + h] = fs - 10;
            off += fs;
        }
        c0[i] = b->clip_frame0[i];
        cn[i] = b->hops[i];
        co[i] = total;
        total += b->hops[i] > 1 ? (uint64_t)(b->hops[i] - 1) * 1024 * b->ch : 0;
        if (b->hops[i] > max_hops) max_hops = b->hops[i];
    }
    return FLO_OK;
}

// Decode every clip of an encoded batch from its device bitstreams (no host round trip of the payload).
extern "C" int flo_batch_decode(flo_batch *b, float *dst, size_t dst_cap, uint64_t *offsets) {
    if (!b || !offsets || (!dst && dst_cap)) return FLO_ERR_ARG;
    flo_ctx *c = b->ctx;
    if (!b->synced) return fail(c, FLO_ERR_STATE, "call flo_batch_encode + flo_batch_sync first");
    HIPCHK(c, hipSetDevice(c->device));
    if (b->mode != FLO_MODE_LOSSY) return batch_decode_lossless(b, dst, dst_cap, offsets);
    std::vector<unsigned long long> blob_off, c0, co;
    std::vector<unsigned int> blob_len, cn;
    uint64_t total = 0;
    unsigned max_hops = 0;
    const int rc = batch_lossy_tables(b, blob_off, blob_len, c0, cn, co, total, max_hops);
    if (rc != FLO_OK) return rc;
    for (size_t i = 0; i < b->n_clips; i++) offsets[i] = co[i];
    if (total > dst_cap) return fail(c, FLO_ERR_ARG, "destination too small for the decoded batch");
    if (!total) return FLO_OK;
    // (dst needs no clearing: the decode kernel writes every sample of every output block exactly once)
    return lossy_decode_whole(c, b->ts, b->d_out, b->ch, blob_off, blob_len, c0, cn, co, max_hops, dst);
}

extern "C" int flo_decode(flo_ctx *c, const uint8_t *flo, size_t len, float **pcm, size_t *n_interleaved,
                          uint32_t *sample_rate, uint8_t *channels) {
    return decode_impl(c, flo, len, pcm, nullptr, n_interleaved, sample_rate, channels);
}
extern "C" int flo_decode_lossless_i32(flo_ctx *c, const uint8_t *flo, size_t len, int32_t **pcm, size_t *n_interleaved,
                                       uint32_t *sample_rate, uint8_t *channels) {
    return decode_impl(c, flo, len, nullptr, pcm, n_interleaved, sample_rate, channels);
}

// decode_frame_at (seeking.rs:43-63): one frame, by its type. Lossless (decode_frame_lossless, :161-176): the frame alone
// through the device lossless path. Transform (decode_frame_lossy, :179-207): the reference warms a TransformDecoder up on
// every earlier frame, which leaves the second half of the last earlier frame with channels in the overlap buffer
// (mdct.rs:437-468); here flo_decode's kernel runs on just that frame and frame i (a two-byte blob of no channels
// stands in for a missing predecessor: it leaves the overlap at zero), so the block is flo_decode's bit for bit.
extern "C" int flo_decode_frame_at(flo_ctx *c, const uint8_t *flo, size_t len, uint32_t frame_index, float **pcm,
                                   size_t *n_interleaved) {
    if (!c || !flo || !pcm || !n_interleaved) return fail(c, FLO_ERR_ARG, "null argument");
    *pcm = nullptr;
    *n_interleaved = 0;
    HIPCHK(c, hipSetDevice(c->device));
    ParsedFile f;
    const char *perr = "";
    if (parse_file(flo, len, f, &perr) != 0) return fail(c, FLO_ERR_FORMAT, perr);
    if ((size_t)frame_index >= f.frames.size())
        return fail(c, FLO_ERR_FORMAT, "Frame index " + std::to_string(frame_index) + " out of bounds (total frames: " +
                                           std::to_string(f.frames.size()) + ")");
    const FrameDesc &fr = f.frames[frame_index];
    const int nch = f.channels;
    DevMem d_bytes;
    QuiesceOnExit quiesce_d_bytes(c);
    HIPCHK(c, pool_alloc(&d_bytes.p, len + 32));
    HIPCHK(c, hipMemcpyAsync(d_bytes.p, flo, len, hipMemcpyHostToDevice, c->stream));
    if (fr.type != 253) {
        LlWrapperList w;
        add_parsed_frame(w, f, fr, 0, ll_force_serial());
        const size_t n_out = nch ? (size_t)fr.samples * (size_t)nch : 0;
        HostResult host(malloc(n_out ? n_out * sizeof(float) : 1), free);
        if (!host) return fail(c, FLO_ERR_NOMEM, "out of host memory");
        if (n_out) {
            DevMem d_out;
            QuiesceOnExit quiesce_d_out(c);
            int rc;
            if (pool_alloc(&d_out.p, n_out * sizeof(float)) != hipSuccess) return fail(c, FLO_ERR_NOMEM, "decode buffers");
            if ((rc = ll_decode_device(c, w, fr.samples, d_bytes.as<uint8_t>(), nch, d_out.as<float>(), nullptr)) != FLO_OK ||
                (rc = download(c, host.get(), d_out.p, n_out * sizeof(float))) != FLO_OK)
                return rc;
        }
        *pcm = (float *)host.release();
        *n_interleaved = n_out;
        return FLO_OK;
    }
    if (!fr.n_channels) return fail(c, FLO_ERR_FORMAT, "Transform frame has no channel data");
    if (nch == 0) return fail(c, FLO_ERR_FORMAT, "Failed to deserialize transform frame");
    // A clip of two blobs: the last earlier frame with channels (or the empty stand-in behind the file's bytes), then frame
    // i. The file's frames before them stay in front of the clip in the list (`lead` of them): a channel the predecessor does
    // not carry overlaps with the last earlier frame that does (seeking.rs:189-200 runs every earlier frame through the decoder)
    static const uint8_t kNoChannels[2] = {0, 0};   // deserialize_frame: Long block, zero channels
    std::vector<unsigned long long> blob_off;
    std::vector<unsigned int> blob_len;
    for (size_t j = 0; j < (size_t)frame_index; j++)
        if (f.frames[j].n_channels) {
            const ChannelDesc &cd = f.channels_desc[f.frames[j].first_channel];
            blob_off.push_back(cd.off);
            blob_len.push_back(cd.len);
        }
    if (blob_off.empty()) {
        blob_off.push_back(len);
        blob_len.push_back(2);
    }
    const unsigned lead = (unsigned)(blob_off.size() - 1);
    blob_off.push_back(f.channels_desc[fr.first_channel].off);
    blob_len.push_back(f.channels_desc[fr.first_channel].len);
    HIPCHK(c, hipMemcpyAsync(d_bytes.as<uint8_t>() + len, kNoChannels, 2, hipMemcpyHostToDevice, c->stream));
    TableSet *ts;
    int rc = get_tables(c, f.sample_rate, 0.5f, &ts);
    if (rc != FLO_OK) return rc;
    const size_t n_out = 1024 * (size_t)nch;
    DevMem d_out;
    QuiesceOnExit quiesce_d_out(c);
    HIPCHK(c, pool_alloc(&d_out.p, n_out * sizeof(float)));
    if ((rc = lossy_decode_whole(c, ts, d_bytes.as<uint8_t>(), nch, blob_off, blob_len, {(unsigned long long)lead}, {2u}, {0}, 2u, d_out.as<float>(), nullptr, lead)) != FLO_OK) return rc;
    HostResult host(malloc(n_out * sizeof(float)), free);
    if (!host) return fail(c, FLO_ERR_NOMEM, "out of host memory");
    if ((rc = download(c, host.get(), d_out.p, n_out * sizeof(float))) != FLO_OK) return rc;
    *pcm = (float *)host.release();
    *n_interleaved = n_out;
    return FLO_OK;
}
