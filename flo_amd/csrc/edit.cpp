// edit.cpp — trimming, fades, padding and channel remixing on the device (flo_batch_edit, flo_batch_active_range, flo_edit,
// flo_edit_tile_frames): a resident batch becomes a resident batch of cuts of its clips, every output clip in one launch.
// Host code only: the checks, the tile geometry and the class of a tile are edit_plan.cpp, the kernels edit_kernels.hip.
#include <cstdlib>
#include <cstring>

#include "batch_internal.hpp"
#include "clip_tiles.hpp"
#include "devmem.hpp"
#include "edit_kernels.hpp"
#include "edit_plan.hpp"

extern "C" int flo_edit_tile_frames(uint8_t in_channels, uint8_t out_channels, uint32_t *frames) {
    if (!frames || in_channels < 1 || out_channels < 1) return FLO_ERR_ARG;
    *frames = edit_tile_frames(out_channels);
    return FLO_OK;
}

extern "C" int flo_batch_edit(flo_batch *src, size_t n_out, const flo_edit_segment *segs, uint8_t out_channels, const float *matrix,
                              flo_batch **out) {
    if (!src || !out) return FLO_ERR_ARG;
    *out = nullptr;
    flo_ctx *c = src->ctx;
    const uint8_t cin = src->ch, cout = out_channels;
    const std::vector<uint64_t> n_src = batch_whole_frames(src);
    std::vector<uint64_t> T;
    EditSource S;
    S.n_clips = src->n_clips;
    S.clip_frames = n_src.data();
    S.channels = cin;
    S.lossy = src->mode == FLO_MODE_LOSSY;
    std::string m;
    if (!edit_check(S, n_out, segs, cout, matrix, T, m)) return fail(c, FLO_ERR_ARG, "flo_batch_edit: " + m);
    if (n_out && !src->pcm_written) return batch_no_pcm(src, "flo_batch_edit");
    std::vector<size_t> n_il(n_out);
    for (size_t k = 0; k < n_out; k++) n_il[k] = (size_t)(T[k] * cout);
    BatchHold made;
    int rc = batch_derive(src, n_out, n_il.data(), src->sr, cout, &made.b);
    if (rc != FLO_OK) return rc;
    flo_batch *b = made.b;
    std::vector<uint32_t> pre;
    if (!clip_tiles(T.data(), n_out, edit_tile_frames(cout), pre)) return fail(c, FLO_ERR_ARG, "flo_batch_edit: too many tiles for one launch");
    if (n_out && pre[n_out]) {
        hipError_t e = hipSetDevice(c->device);
        if (e != hipSuccess) return fail(c, FLO_ERR_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));
        // segments | pre: up through pinned memory into a pool block, both the new batch's until it goes
        BlockLayout B;
        const size_t o_segs = B.take(n_out * sizeof(EditSeg)), o_pre = B.take((n_out + 1) * 4);
        rc = work_block_get(c, B.bytes, "flo_batch_edit: work list", b->pin_work, b->d_work);
        if (rc != FLO_OK) return rc;
        void *const host = b->pin_work, *const dev = b->d_work;
        EditSeg *hs = B.at<EditSeg>(host, o_segs);
        for (size_t k = 0; k < n_out; k++) {
            const flo_edit_segment &g = segs[k];
            EditSeg s{};
            s.src_off = src->clip_off[g.clip];
            s.n_src = n_src[g.clip];
            s.start = g.start;
            s.frames = g.frames;
            s.dst_off = b->clip_off[k];
            s.pad_head = g.pad_head;
            s.pad_tail = g.pad_tail;
            s.fade_in = g.fade_in;
            s.fade_out = g.fade_out;
            hs[k] = s;
        }
        memcpy(B.at<uint32_t>(host, o_pre), pre.data(), (n_out + 1) * 4);
        e = hipMemcpyAsync(dev, host, B.bytes, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) return fail(c, FLO_ERR_DEVICE, std::string("hipMemcpyAsync: ") + hipGetErrorString(e));
        EditArgs A;
        A.src = src->d_pcm;
        A.dst = b->d_pcm;
        A.segs = B.at<const EditSeg>(dev, o_segs);
        A.pre = B.at<const unsigned int>(dev, o_pre);
        A.n_segs = (unsigned)n_out;
        A.cin = cin;
        A.cout = cout;
        edit_matrix_rows(matrix, cin, cout, A.m);
        const EditForm form = !matrix ? kEditCopy : cin == 2 && cout == 1 ? kEditTwoToOne : cin == 1 && cout == 2 ? kEditOneToTwo : kEditGeneric;
        static const char *const names[] = {"edit_copy", "edit_2to1", "edit_1to2", "edit_mix"};
        rc = timed_launch(c, names[form], [&] { return launch_edit(A, form, pre[n_out], c->stream); });
        if (rc != FLO_OK) return rc;
    }
    b->pcm_written = true;
    *out = made.release();
    return FLO_OK;
}

extern "C" int flo_batch_active_range(flo_batch *b, float threshold, uint64_t *first, uint64_t *end) {
    if (!b || ((!first || !end) && b->n_clips)) return FLO_ERR_ARG;
    flo_ctx *c = b->ctx;
    std::string m;
    if (!edit_threshold(threshold, m)) return fail(c, FLO_ERR_ARG, "flo_batch_active_range: " + m);
    const size_t n = b->n_clips;
    if (!n) return FLO_OK;
    if (!b->pcm_written) return batch_no_pcm(b, "flo_batch_active_range");
    HIPCHK(c, hipSetDevice(c->device));
    const std::vector<uint64_t> frames = batch_whole_frames(b);
    std::vector<uint32_t> pre;
    if (!clip_tiles(frames.data(), n, edit_tile_frames(b->ch), pre)) return fail(c, FLO_ERR_ARG, "flo_batch_active_range: too many tiles for one launch");
    for (size_t i = 0; i < n; i++) first[i] = end[i] = 0;
    if (!pre[n]) return FLO_OK;
    // src_off | frames | first, end | pre in one block that goes up in one copy; first and end start from ~0 and 0 here,
    // so nothing depends on what the pool block held (and stay one region: they come back in one copy)
    BlockLayout B;
    const size_t o_off = B.take(n * 8), o_frames = B.take(n * 8), o_first = B.take(2 * n * 8), o_end = o_first + n * 8, o_pre = B.take((n + 1) * 4),
                 bytes = B.bytes;
    std::vector<uint8_t> host(bytes, 0);   // (outlives the stream: destroyed behind `quiesce`)
    memcpy(host.data() + o_off, b->clip_off.data(), n * 8);
    memcpy(host.data() + o_frames, frames.data(), n * 8);
    memset(host.data() + o_first, 0xFF, n * 8);
    memcpy(host.data() + o_pre, pre.data(), (n + 1) * 4);
    std::vector<uint64_t> back(2 * n);   // (likewise: the copy back targets it)
    DevBuf<uint8_t> dev;
    QuiesceOnExit quiesce(c);
    if (!dev.alloc(bytes)) return fail(c, FLO_ERR_NOMEM, "flo_batch_active_range: device memory");
    HIPCHK(c, hipMemcpyAsync(dev.p, host.data(), bytes, hipMemcpyHostToDevice, c->stream));
    EditActiveArgs A;
    A.src = b->d_pcm;
    A.src_off = B.at<const unsigned long long>(dev.p, o_off);
    A.frames = B.at<const unsigned long long>(dev.p, o_frames);
    A.first = B.at<unsigned long long>(dev.p, o_first);
    A.end = B.at<unsigned long long>(dev.p, o_end);
    A.pre = B.at<const unsigned int>(dev.p, o_pre);
    A.n_clips = (unsigned)n;
    A.channels = b->ch;
    A.threshold = threshold;
    int rc = timed_launch(c, "edit_active", [&] { return launch_edit_active(A, pre[n], c->stream); });
    if (rc != FLO_OK) return rc;
    HIPCHK(c, hipMemcpyAsync(back.data(), dev.p + o_first, 2 * n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < n; i++) {
        const bool any = back[n + i] != 0;
        first[i] = any ? back[i] : 0;
        end[i] = any ? back[n + i] : 0;
    }
    return FLO_OK;
}

extern "C" int flo_edit(flo_ctx *c, const float *pcm, size_t n_interleaved, uint32_t sample_rate, uint8_t channels,
                        const flo_edit_segment *seg, uint8_t out_channels, const float *matrix, float **out, size_t *n_out) {
    if (!c || !out || !n_out || !seg || (!pcm && n_interleaved)) return FLO_ERR_ARG;
    *out = nullptr;
    *n_out = 0;
    if (channels < 1) return fail(c, FLO_ERR_ARG, "flo_edit: channels must be at least 1");
    if (!sample_rate) return fail(c, FLO_ERR_ARG, "flo_edit: sample_rate must be non-zero");
    return batch_one_shot(c, "flo_edit", pcm, n_interleaved / channels * channels, sample_rate, channels, [&](flo_batch *a, flo_batch **b) {
        const int rc = flo_batch_edit(a, 1, seg, out_channels, matrix, b);
        if (rc != FLO_OK) {
            const std::string msg = c->err, from = "flo_batch_edit: ";   // "flo_batch_edit: ..." reads "flo_edit: ..." here
            if (msg.compare(0, from.size(), from) == 0) fail(c, rc, "flo_edit: " + msg.substr(from.size()));
        }
        return rc;
    }, out, n_out);
}
