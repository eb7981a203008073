// curve_pass.cpp — see curve_pass.hpp. Host code only.
#include "curve_pass.hpp"

int batch_zero_partial_frames(flo_batch *b) {
    flo_ctx *c = b->ctx;
    for (size_t i = 0; i < b->n_clips; i++) {
        const uint64_t part = b->n_il[i] % b->ch;
        if (part) HIPCHK(c, hipMemsetAsync(b->d_pcm + b->clip_off[i] + b->clip_nsf[i] * b->ch, 0, part * sizeof(float), c->stream));
    }
    return FLO_OK;
}

int curve_args_fill(flo_batch *b, size_t n_q, const float *qualities, CurveArgs &C, unsigned char *levels) {
    C = CurveArgs{};
    C.n_q = (int)n_q;
    for (size_t j = 0; j < n_q; j++) {
        TableSet *ts = nullptr;
        int rc = get_tables(b->ctx, b->sr, qualities[j], &ts);
        if (rc != FLO_OK) return rc;
        if (j == 0) C.A.T = ts->dev;
        C.smr_thr[j] = ts->dev.smr_thr;
        C.ath[j] = ts->dev.pack_g + kRowAth * 64;
        if (lossy_exact(b->exact != 0, ts->dev)) C.exact_mask |= 1u << j;
        if (ts->dev.q_transparent) C.qtrans_mask |= 1u << j;
        if (levels) levels[j] = (unsigned char)ts->host.q_level;
    }
    return FLO_OK;
}

bool LevelRows::alloc(const flo_batch *b, const std::vector<ClipGroup> &groups) {
    rel.resize(b->n_clips);
    for (const ClipGroup &g : groups) {
        max_frames = g.frames > max_frames ? g.frames : max_frames;
        uint64_t f = 0;
        for (size_t i = 0; i < g.count; i++) {
            rel[g.first + i] = f;
            f += b->hops[g.first + i];
        }
    }
    const size_t row = max_frames * b->ch * 32;
    return d_at.alloc(row) && d_inf.alloc(b->n_clips * b->ch * 32) && d_sprev.alloc(row) && (b->ch != 2 || d_bmax.alloc(row)) && d_rel.alloc(b->n_clips);
}

int LevelRows::enqueue_clear(flo_batch *b) {
    flo_ctx *c = b->ctx;
    HIPCHK(c, hipMemcpyAsync(d_rel.p, rel.data(), b->n_clips * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(d_inf.p, 0, b->n_clips * b->ch * 32 * 8, c->stream));
    return FLO_OK;
}

int level_rows_pass(flo_batch *b, CurveArgs &C, const LevelRows &R, const ClipGroup &g, const char *bands, const char *scan) {
    flo_ctx *c = b->ctx;
    const unsigned long long *plan = (const unsigned long long *)b->d_plan;
    const FrameKernel pass1 = b->ch == 1 ? FrameKernel::Mono1 : b->ch == 2 ? FrameKernel::Pair1 : FrameKernel::Multi1;
    LossyArgs &A = C.A;
    A.pcm = b->d_pcm;
    A.clip_off = plan + g.first;
    A.clip_nsf = plan + b->n_clips + g.first;
    A.clip_frame0 = R.d_rel.p + g.first;
    A.clip_hops = b->d_hops + g.first;
    A.nch = b->ch;
    A.n_clips = (int)g.count;
    A.total_frames = g.frames;
    A.max_hops = g.max_hops;
    A.a_t = R.d_at.p;
    A.bmax_t = R.d_bmax.p;
    A.s_prev_out = R.d_sprev.p;
    A.s_prev = R.d_sprev.p;
    A.inf_mark = R.d_inf.p;
    A.inf_tag++;   // (inf_tag shares its storage with epoch, which nothing sets on this struct: frame-parallel launches only)
    A.slot_bytes = lossy_slot_bytes(b->ch);
    int rc = timed_launch(c, bands, [&] { return launch_lossy_frames_pass(A, pass1, c->stream); });
    if (rc != FLO_OK) return rc;
    return timed_launch(c, scan, [&] { return launch_lossy_scan(A, c->stream); });
}

FinishArgs lossy_finish_args(const flo_batch *b, uint8_t *out, const unsigned long long *data_off, const unsigned long long *clip_bytes,
                             const unsigned long long *clip_frame0, const unsigned int *clip_frames, const unsigned int *frame_size,
                             size_t n_files, unsigned short flags, unsigned int *part_reg, unsigned int max_frames) {
    FinishArgs F{};
    F.out = out;
    F.data_off = data_off;
    F.clip_bytes = clip_bytes;
    F.clip_frame0 = clip_frame0;
    F.clip_frames = clip_frames;
    F.frame_size = frame_size;
    F.frame_samples = nullptr;
    F.const_samples = 1024;
    F.sample_rate = b->sr;
    F.flags = flags;
    F.channels = b->ch;
    F.bit_depth = 16;
    F.level = 5;
    F.n_clips = (int)n_files;
    F.part_reg = part_reg;
    F.max_frames = max_frames;
    return F;
}
