// rate.cpp — size curves and the rate-targeted lossy encode (flo_batch_size_curve, flo_batch_set_quality, flo_rate_pick,
// flo_encode_batch_to_size). Host code only: the kernels live in lossy_kernels.hip, the choice in rate_select.cpp.
#include <cstdlib>
#include <cstring>

#include "curve_pass.hpp"
#include "rate_select.hpp"

// scratch of one group of clips: the frame-parallel levels (a_t, s_prev; band maxima for the stereo pass 1), read per call
static size_t size_curve_group_bytes() {
    const char *e = getenv("FLO_SIZE_CURVE_GROUP_BYTES");
    const long long v = e ? atoll(e) : 0;
    return v > 0 ? (size_t)v : ((size_t)256 << 20);
}

extern "C" int flo_batch_size_curve(flo_batch *b, size_t n_q, const float *qualities, uint64_t *file_bytes) {
    if (!b) return FLO_ERR_ARG;
    flo_ctx *c = b->ctx;
    if (b->mode != FLO_MODE_LOSSY) return fail(c, FLO_ERR_ARG, "a size curve needs a lossy batch");
    if (n_q < 1 || n_q > (size_t)kMaxCurveCandidates) return fail(c, FLO_ERR_ARG, "1 to 32 candidate qualities");
    if (!qualities || !file_bytes) return fail(c, FLO_ERR_ARG, "null pointer");
    if (!b->n_clips) return FLO_OK;
    if (!b->pcm_written) return fail(c, FLO_ERR_STATE, "upload or fill the batch's PCM before flo_batch_size_curve");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = b->n_clips, K = n_q;
    const int ch = b->ch;
    int rc = batch_zero_partial_frames(b);
    if (rc != FLO_OK) return rc;
    CurveArgs C;
    if ((rc = curve_args_fill(b, K, qualities, C, nullptr)) != FLO_OK) return rc;
    // groups of consecutive clips whose scratch stays under the limit (a clip larger than the limit is a group of its own)
    const std::vector<ClipGroup> groups = partition_clips(b->hops.data(), n, level_row_bytes(b->ch), size_curve_group_bytes());
    LevelRows R;
    DevBuf<unsigned long long> d_sizes;
    QuiesceOnExit quiesce(c);
    if (!R.alloc(b, groups) || !d_sizes.alloc(n * K)) return fail(c, FLO_ERR_NOMEM, "size curve scratch");
    if ((rc = R.enqueue_clear(b)) != FLO_OK) return rc;
    HIPCHK(c, hipMemsetAsync(d_sizes.p, 0, n * K * 8, c->stream));
    for (const ClipGroup &g : groups) {
        if ((rc = level_rows_pass(b, C, R, g, "curve_bands", "curve_scan")) != FLO_OK) return rc;
        if ((rc = timed_launch(c, "size_curve", [&] { return launch_lossy_curve(C, R.d_at.p, R.d_sprev.p, d_sizes.p + g.first * K, c->stream); })) != FLO_OK)
            return rc;
    }
    std::vector<uint64_t> sparse(n * K);
    HIPCHK(c, hipMemcpyAsync(sparse.data(), d_sizes.p, n * K * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // what does not depend on quality: per frame the header (10), block size and channel count (2), 25 scale words and one
    // length word per channel; per file the header and the TOC
    for (size_t i = 0; i < n; i++) {
        const uint64_t h = b->hops[i];
        const uint64_t fixed = head_bytes(h) + h * (12 + 54 * (uint64_t)ch);
        for (size_t j = 0; j < K; j++) file_bytes[i * K + j] = fixed + sparse[i * K + j];
    }
    return FLO_OK;
}

extern "C" int flo_batch_set_quality(flo_batch *b, float quality) {
    if (!b) return FLO_ERR_ARG;
    flo_ctx *c = b->ctx;
    if (b->mode != FLO_MODE_LOSSY) return fail(c, FLO_ERR_ARG, "only a lossy batch has a quality");
    HIPCHK(c, hipSetDevice(c->device));
    TableSet *ts = nullptr;
    int rc = get_tables(c, b->sr, quality, &ts);
    if (rc != FLO_OK) return rc;
    b->ts = ts;
    b->qol = quality;
    b->encoded = b->synced = b->encode_failed = false;
    return FLO_OK;
}

extern "C" int flo_rate_pick(size_t n_q, const float *qualities, const uint64_t *sizes, uint64_t budget, uint32_t *index, int *fits) {
    if (n_q < 1 || n_q > (size_t)kMaxCurveCandidates || !qualities || !sizes || !index || !fits) return FLO_ERR_ARG;
    const RatePick p = rate_pick(n_q, qualities, sizes, budget);
    *index = p.index;
    *fits = p.fits;
    return FLO_OK;
}

extern "C" int flo_encode_batch_to_size(flo_ctx *c, size_t n_clips, const float *const *pcm, const size_t *n_il, uint32_t sr, uint8_t ch,
                                        size_t n_q, const float *qualities, const uint64_t *target_bytes, const uint8_t *const *meta,
                                        const size_t *meta_lens, uint8_t **outs, size_t *out_lens, uint32_t *chosen, int *fits) {
    if (!c) return FLO_ERR_ARG;
    if (n_q < 1 || n_q > (size_t)kMaxCurveCandidates) return fail(c, FLO_ERR_ARG, "1 to 32 candidate qualities");
    if (!qualities || (n_clips && (!pcm || !n_il || !target_bytes || !outs || !out_lens || !chosen || !fits)))
        return fail(c, FLO_ERR_ARG, "null pointer");
    if ((meta != nullptr) != (meta_lens != nullptr)) return fail(c, FLO_ERR_ARG, "meta and meta_lens go together");
    for (size_t i = 0; i < n_clips; i++)
        if ((n_il[i] && !pcm[i]) || (meta && meta_lens[i] && !meta[i])) return fail(c, FLO_ERR_ARG, "null pointer");
    if (!n_clips) return FLO_OK;
    for (size_t i = 0; i < n_clips; i++) outs[i] = nullptr;
    flo_batch *all = nullptr, *child = nullptr;
    auto leave = [&](int code) {
        if (child) flo_batch_destroy(child);
        if (all) flo_batch_destroy(all);
        if (code != FLO_OK)
            for (size_t i = 0; i < n_clips; i++) {
                free(outs[i]);
                outs[i] = nullptr;
            }
        return code;
    };
    int rc = flo_batch_create(c, FLO_MODE_LOSSY, n_clips, n_il, sr, ch, qualities[0], &all);
    if (rc != FLO_OK) return rc;
    if ((rc = batch_upload_all(all, pcm)) != FLO_OK) return leave(rc);
    std::vector<uint64_t> sizes(n_clips * n_q);
    if ((rc = flo_batch_size_curve(all, n_q, qualities, sizes.data())) != FLO_OK) return leave(rc);
    std::vector<std::vector<size_t>> by_q(n_q);
    for (size_t i = 0; i < n_clips; i++) {
        const uint64_t ml = meta ? meta_lens[i] : 0;
        const RatePick p = rate_pick(n_q, qualities, &sizes[i * n_q], target_bytes[i] >= ml ? target_bytes[i] - ml : 0);
        chosen[i] = p.index;
        // (a META longer than the target leaves a budget of 0, which no file meets: even an empty clip's has a header and one frame)
        fits[i] = p.fits;
        by_q[p.index].push_back(i);
    }
    // every clip is encoded once, at its chosen quality: per candidate a batch of its clips, filled from the first batch's
    // device copy; when every clip chose the same candidate the first batch itself is re-pointed
    for (size_t j = 0; j < n_q; j++) {
        const std::vector<size_t> &m = by_q[j];
        if (m.empty()) continue;
        flo_batch *e = all;
        if (m.size() == n_clips) {
            if ((rc = flo_batch_set_quality(all, qualities[j])) != FLO_OK) return leave(rc);
        } else {
            std::vector<size_t> il(m.size());
            for (size_t k = 0; k < m.size(); k++) il[k] = n_il[m[k]];
            if ((rc = flo_batch_create(c, FLO_MODE_LOSSY, m.size(), il.data(), sr, ch, qualities[j], &child)) != FLO_OK) return leave(rc);
            for (size_t k = 0; k < m.size(); k++) {
                const size_t bytes = (size_t)(all->clip_nsf[m[k]] * ch) * sizeof(float);
                if (!bytes) continue;
                hipError_t he = hipMemcpyAsync(child->d_pcm + child->clip_off[k], all->d_pcm + all->clip_off[m[k]], bytes, hipMemcpyDeviceToDevice, c->stream);
                if (he != hipSuccess) return leave(fail(c, FLO_ERR_DEVICE, std::string("device copy: ") + hipGetErrorString(he)));
            }
            child->pcm_written = true;
            e = child;
        }
        if ((rc = flo_batch_encode(e, 0)) != FLO_OK) return leave(rc);
        if ((rc = flo_batch_sync(e)) != FLO_OK) return leave(rc);
        for (size_t k = 0; k < m.size(); k++) {
            const size_t i = m[k];
            if ((rc = flo_batch_fetch(e, e == all ? i : k, meta ? meta[i] : nullptr, meta ? meta_lens[i] : 0, &outs[i], &out_lens[i])) != FLO_OK)
                return leave(rc);
        }
        if (child) {
            flo_batch_destroy(child);
            child = nullptr;
        }
    }
    return leave(FLO_OK);
}
