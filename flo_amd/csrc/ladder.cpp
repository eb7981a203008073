// ladder.cpp — quality ladders (flo_batch_encode_ladder, flo_ladder_*, flo_encode_batch_ladder): every clip of a lossy
// batch as a finished file at each of K qualities, from ONE transform pass. Host code only: the kernel that packs a frame
// at every rung is lossy_ladder_kernel (ladder_kernels.hip), the partition into groups is ladder_plan.cpp, the files'
// places are file_layout.hpp.
//
// Per group of consecutive clips: pass 1 and the scan of the frame-parallel form (curve_pass.cpp, shared with flo_batch_size_curve),
// then lossy_ladder_kernel into [rung][frame] slots. The kernel also adds up every (rung, clip)'s DATA bytes; those come
// back to the host - ONE synchronisation per group - and size the group's work buffer exactly. The existing frame-offsets
// and compaction kernels then run once over all rungs of the group: (rung, clip) is presented to them as a clip of its
// own, rung-major, so that a rung's frames are consecutive. launch_finish_files sees the same clips, once per group; the
// one header byte that differs from rung to rung, the quality level in the flags, is set behind it
// (ladder_header_levels_kernel). When every group is done the files are moved by pack_streams_kernel into one
// allocation, rung-major at 16-byte aligned offsets: that allocation is all that stays resident.
#include <cstdlib>
#include <cstring>
#include <deque>

#include "curve_pass.hpp"

struct flo_ladder {
    flo_ctx *ctx = nullptr;
    size_t n_clips = 0, n_q = 0;
    std::vector<uint64_t> off, size;   // [n_q][n_clips]: the finished files inside d_files (header + TOC + DATA, no META)
    uint8_t *d_files = nullptr;
};

// Scratch of one group of clips (slots of every rung, frame sizes and offsets, the frame-parallel levels), read per call.
// 4 GiB holds 60 000 stereo frames at 16 rungs (23 minutes of audio). A group costs one synchronisation and eight
// launches; measured on 1250 x 10 s stereo at 16 rungs: 88.6 ms with groups of 256 MiB, 38.8 ms with 1 GiB, 31.8 ms with
// 4 GiB, and 594 ms with 16 GiB, where the driver's allocation of the blocks dominates.
static size_t ladder_group_bytes() {
    const char *e = getenv("FLO_LADDER_GROUP_BYTES");
    const long long v = e ? atoll(e) : 0;
    return v > 0 ? (size_t)v : ((size_t)4 << 30);
}

extern "C" void flo_ladder_destroy(flo_ladder *l) {
    if (!l) return;
    if (l->d_files) {
        hipSetDevice(l->ctx->device);
        hipStreamSynchronize(l->ctx->stream);
        pool_free(l->d_files);
    }
    delete l;
}

extern "C" int flo_batch_encode_ladder(flo_batch *b, size_t n_q, const float *qualities, flo_ladder **out) {
    if (!b) return FLO_ERR_ARG;
    flo_ctx *c = b->ctx;
    if (out) *out = nullptr;
    if (b->mode != FLO_MODE_LOSSY) return fail(c, FLO_ERR_ARG, "a quality ladder needs a lossy batch");
    if (n_q < 1 || n_q > (size_t)kMaxCurveCandidates) return fail(c, FLO_ERR_ARG, "1 to 32 rungs");
    if (!qualities || !out) return fail(c, FLO_ERR_ARG, "null pointer");
    if (b->n_clips && !b->pcm_written) return fail(c, FLO_ERR_STATE, "upload or fill the batch's PCM before flo_batch_encode_ladder");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = b->n_clips, K = n_q;
    const int ch = b->ch;
    flo_ladder *l = new flo_ladder();
    l->ctx = c;
    l->n_clips = n;
    l->n_q = K;
    l->off.assign(n * K, 0);
    l->size.assign(n * K, 0);
    if (!n) {
        *out = l;
        return FLO_OK;
    }
    auto leave = [&](int code) {
        if (code != FLO_OK) {
            hipStreamSynchronize(c->stream);   // the ladder's files go back to the pool: nothing may still write them
            flo_ladder_destroy(l);
        }
        return code;
    };
    int rc = batch_zero_partial_frames(b);
    if (rc != FLO_OK) return leave(rc);
    CurveArgs C;
    LadderLevels levels{};   // the header's quality level of every rung (batch.cpp: flags = 0x01 | q_level << 8)
    if ((rc = curve_args_fill(b, K, qualities, C, levels.level)) != FLO_OK) return leave(rc);
    const unsigned slot_bytes = lossy_slot_bytes(ch);
    const std::vector<ClipGroup> groups = partition_clips(b->hops.data(), n, ladder_frame_bytes(ch, K, slot_bytes), ladder_group_bytes());
    size_t max_parts = 1;
    for (const ClipGroup &g : groups) {
        if (g.frames * K > 0x7FFFFFFFull) return leave(fail(c, FLO_ERR_ARG, "a clip too long for a ladder of this many rungs"));
        const size_t parts = K * g.count * finish_parts(K * g.count);
        max_parts = parts > max_parts ? parts : max_parts;
    }
    // (rung, clip) as the compaction and finish kernels see it: a clip of its own, rung-major inside its group; group g's
    // entries are [K * g.first, K * (g.first + g.count))
    const size_t V = n * K;
    std::vector<uint64_t> v_frame0(V), v_out(V), v_data(V);
    std::vector<uint32_t> v_hops(V);
    LevelRows R;
    DevBuf<unsigned long long> d_sizes, d_vframe0, d_vout, d_vbytes, d_foff, d_pack;
    DevBuf<unsigned int> d_vhops, d_fsize, d_part;
    DevBuf<uint8_t> d_slots;
    std::deque<DevBuf<uint8_t>> work;   // per group: its finished files at their DATA-aligned places, until the last move
    QuiesceOnExit quiesce(c);
    if (!R.alloc(b, groups) || !d_sizes.alloc(V) || !d_vframe0.alloc(V) || !d_vout.alloc(V) || !d_vbytes.alloc(V) || !d_vhops.alloc(V) ||
        !d_part.alloc(max_parts + 1) || !d_foff.alloc(R.max_frames * K + 1) || !d_fsize.alloc(R.max_frames * K + 1) ||
        !d_pack.alloc(3 * V) || !d_slots.alloc((size_t)R.max_frames * K * slot_bytes))
        return leave(fail(c, FLO_ERR_NOMEM, "ladder scratch"));
    for (const ClipGroup &g : groups)
        for (size_t j = 0; j < K; j++)
            for (size_t i = 0; i < g.count; i++) {
                const size_t v = K * g.first + j * g.count + i;
                v_frame0[v] = j * g.frames + R.rel[g.first + i];
                v_hops[v] = b->hops[g.first + i];
            }
    if ((rc = R.enqueue_clear(b)) != FLO_OK) return leave(rc);
    HIPCHK_OR(c, hipMemcpyAsync(d_vframe0.p, v_frame0.data(), V * 8, hipMemcpyHostToDevice, c->stream), leave);
    HIPCHK_OR(c, hipMemcpyAsync(d_vhops.p, v_hops.data(), V * 4, hipMemcpyHostToDevice, c->stream), leave);
    HIPCHK_OR(c, hipMemsetAsync(d_sizes.p, 0, V * 8, c->stream), leave);
    C.A.slots = d_slots.p;
    C.A.frame_size = d_fsize.p;
    std::vector<uint64_t> src_off(V);   // the files inside their group's work buffer
    for (const ClipGroup &g : groups) {
        const size_t base = K * g.first, vg = K * g.count;
        if ((rc = level_rows_pass(b, C, R, g, "ladder_bands", "ladder_scan")) != FLO_OK) return leave(rc);
        if ((rc = timed_launch(c, "lossy_ladder", [&] { return launch_lossy_ladder(C, R.d_at.p, R.d_sprev.p, d_sizes.p + base, c->stream); })) != FLO_OK)
            return leave(rc);
        // the group's DATA sizes -> its work buffer, exactly: every file's header + TOC right in front of its aligned DATA
        HIPCHK_OR(c, hipMemcpyAsync(v_data.data() + base, d_sizes.p + base, vg * 8, hipMemcpyDeviceToHost, c->stream), leave);
        HIPCHK_OR(c, hipStreamSynchronize(c->stream), leave);
        uint64_t o = 0;
        for (size_t v = base; v < base + vg; v++) {
            const FilePlace at = place_file(o, v_hops[v], v_data[v]);
            v_out[v] = at.data_off;
            src_off[v] = at.file_off;
        }
        work.emplace_back();
        if (!work.back().alloc(o + 64)) return leave(fail(c, FLO_ERR_NOMEM, "ladder files"));
        HIPCHK_OR(c, hipMemcpyAsync(d_vout.p + base, v_out.data() + base, vg * 8, hipMemcpyHostToDevice, c->stream), leave);
        LossyArgs B = C.A;
        B.clip_frame0 = d_vframe0.p + base;
        B.clip_hops = d_vhops.p + base;
        B.n_clips = (int)vg;
        B.total_frames = g.frames * K;
        B.out = work.back().p;
        B.out_off = d_vout.p + base;
        B.clip_bytes = d_vbytes.p + base;
        B.frame_off = d_foff.p;
        // The fused offsets-and-compaction kernel wherever its grid allows (clips in y): it copies by dwords, and what a chunk's
        // workgroup adds up in front of its chunk is one clip's frame sizes, a few hundred for the clips a group holds many of.
        // (Measured on 1250 x 10 s stereo at 16 rungs: the per-frame copy kernel behind the 256-thread offsets took 12.6 ms.)
        const CompactKernel ck = vg <= 65535 ? CompactKernel::Fused : CompactKernel::Offsets256;
        if ((rc = timed_launch(c, "ladder_compact", [&] { return launch_lossy_compact(B, ck, c->stream); })) != FLO_OK) return leave(rc);
        // header, TOC and CRC32 of every file of the group in one finish (the rungs' files differ in one header byte, the quality
        // level, which a launch of its own then sets)
        const FinishPlan fin = plan_finish(vg, g.max_hops, false);
        const FinishArgs F = lossy_finish_args(b, work.back().p, d_vout.p + base, d_vbytes.p + base, d_vframe0.p + base, d_vhops.p + base,
                                               d_fsize.p, vg, 0x01, d_part.p, g.max_hops);
        if ((rc = timed_launch(c, "ladder_finish", [&] { return launch_finish_files(F, fin, c->stream); })) != FLO_OK) return leave(rc);
        rc = timed_launch(c, "ladder_levels", [&] {
            return launch_ladder_header_levels(work.back().p, d_vout.p + base, d_vhops.p + base, (unsigned)g.count, (unsigned)vg, levels, c->stream);
        });
        if (rc != FLO_OK) return leave(rc);
    }
    // what stays resident: the files' exact bytes, rung-major, 16-byte aligned
    std::vector<uint64_t> dst_off(V), fsz(V);
    for (const ClipGroup &g : groups)
        for (size_t j = 0; j < K; j++)
            for (size_t i = 0; i < g.count; i++) {
                const size_t v = K * g.first + j * g.count + i;
                l->size[j * n + g.first + i] = head_bytes(v_hops[v]) + v_data[v];
            }
    const uint64_t total = packed_offsets(l->size.data(), V, l->off.data());
    HIPCHK_OR(c, pool_alloc(&l->d_files, total + 16), leave);
    for (const ClipGroup &g : groups)
        for (size_t j = 0; j < K; j++)
            for (size_t i = 0; i < g.count; i++) {
                const size_t v = K * g.first + j * g.count + i;
                dst_off[v] = l->off[j * n + g.first + i];
                fsz[v] = l->size[j * n + g.first + i];
            }
    HIPCHK_OR(c, hipMemcpyAsync(d_pack.p, src_off.data(), V * 8, hipMemcpyHostToDevice, c->stream), leave);
    HIPCHK_OR(c, hipMemcpyAsync(d_pack.p + V, dst_off.data(), V * 8, hipMemcpyHostToDevice, c->stream), leave);
    HIPCHK_OR(c, hipMemcpyAsync(d_pack.p + 2 * V, fsz.data(), V * 8, hipMemcpyHostToDevice, c->stream), leave);
    size_t gi = 0;
    for (const ClipGroup &g : groups) {
        const size_t base = K * g.first, vg = K * g.count;
        const uint8_t *src = work[gi++].p;
        rc = timed_launch(c, "ladder_pack", [&] {
            return launch_pack_streams(src, d_pack.p + base, d_pack.p + V + base, d_pack.p + 2 * V + base, (int)vg, l->d_files, c->stream);
        });
        if (rc != FLO_OK) return leave(rc);
    }
    HIPCHK_OR(c, hipStreamSynchronize(c->stream), leave);
    *out = l;
    return FLO_OK;
}

extern "C" int flo_ladder_shape(const flo_ladder *l, size_t *n_clips, size_t *n_q) {
    if (!l) return FLO_ERR_ARG;
    if (n_clips) *n_clips = l->n_clips;
    if (n_q) *n_q = l->n_q;
    return FLO_OK;
}

extern "C" int flo_ladder_file_bytes(const flo_ladder *l, uint64_t *file_bytes) {
    if (!l || (!file_bytes && l->n_clips)) return FLO_ERR_ARG;
    for (size_t i = 0; i < l->n_clips; i++)
        for (size_t j = 0; j < l->n_q; j++) file_bytes[i * l->n_q + j] = l->size[j * l->n_clips + i];
    return FLO_OK;
}

extern "C" int flo_ladder_fetch(flo_ladder *l, size_t clip, size_t rung, const uint8_t *meta, size_t meta_len, uint8_t **out, size_t *out_len) {
    if (!l || clip >= l->n_clips || rung >= l->n_q || !out || !out_len || (meta_len && !meta)) return FLO_ERR_ARG;
    flo_ctx *c = l->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t k = rung * l->n_clips + clip;
    return fetch_file(c, l->d_files + l->off[k], (size_t)l->size[k], meta, meta_len, -1, "ladder fetch", out, out_len);
}

extern "C" int flo_ladder_device_files(flo_ladder *l, size_t rung, const uint8_t **base, const uint64_t **offsets, const uint64_t **sizes) {
    if (!l || rung >= l->n_q) return FLO_ERR_ARG;
    if (base) *base = l->d_files;
    if (offsets) *offsets = l->off.data() + rung * l->n_clips;
    if (sizes) *sizes = l->size.data() + rung * l->n_clips;
    return FLO_OK;
}

extern "C" int flo_encode_batch_ladder(flo_ctx *c, size_t n_clips, const float *const *pcm, const size_t *n_il, uint32_t sr, uint8_t ch,
                                       size_t n_q, const float *qualities, const uint8_t *const *meta, const size_t *meta_lens,
                                       uint8_t **outs, size_t *out_lens) {
    if (!c) return FLO_ERR_ARG;
    if (n_q < 1 || n_q > (size_t)kMaxCurveCandidates) return fail(c, FLO_ERR_ARG, "1 to 32 rungs");
    if (!qualities || (n_clips && (!pcm || !n_il || !outs || !out_lens))) return fail(c, FLO_ERR_ARG, "null pointer");
    if ((meta != nullptr) != (meta_lens != nullptr)) return fail(c, FLO_ERR_ARG, "meta and meta_lens go together");
    for (size_t i = 0; i < n_clips; i++)
        if ((n_il[i] && !pcm[i]) || (meta && meta_lens[i] && !meta[i])) return fail(c, FLO_ERR_ARG, "null pointer");
    if (!n_clips) return FLO_OK;
    for (size_t k = 0; k < n_clips * n_q; k++) outs[k] = nullptr;
    flo_batch *all = nullptr;
    flo_ladder *l = nullptr;
    auto leave = [&](int code) {
        if (l) flo_ladder_destroy(l);
        if (all) flo_batch_destroy(all);
        if (code != FLO_OK)
            for (size_t k = 0; k < n_clips * n_q; k++) {
                free(outs[k]);
                outs[k] = nullptr;
            }
        return code;
    };
    int rc = flo_batch_create(c, FLO_MODE_LOSSY, n_clips, n_il, sr, ch, qualities[0], &all);
    if (rc != FLO_OK) return rc;
    if ((rc = batch_upload_all(all, pcm)) != FLO_OK) return leave(rc);
    if ((rc = flo_batch_encode_ladder(all, n_q, qualities, &l)) != FLO_OK) return leave(rc);
    for (size_t i = 0; i < n_clips; i++)
        for (size_t j = 0; j < n_q; j++)
            if ((rc = flo_ladder_fetch(l, i, j, meta ? meta[i] : nullptr, meta ? meta_lens[i] : 0, &outs[i * n_q + j], &out_lens[i * n_q + j])) != FLO_OK)
                return leave(rc);
    return leave(FLO_OK);
}
