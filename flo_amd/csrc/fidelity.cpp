// fidelity.cpp — flo_batch_fidelity and flo_compare: how far the decoded audio of a batch or a file lies from its source,
// measured on the device (definitions in include/flo_hip.h; kernels in fidelity_kernels.hip and
// lossy_decode_kernel<kDecCompare>, decode_kernels.hip).
//
// Every pass makes one record per (decoded block, channel) (FidBlockDev): a lossy batch or file in the fused decode pass,
// which loads the source where the plain decode stores its output and writes no PCM; a lossless batch or file, and a
// lossy batch under FLO_FIDELITY_UNFUSED=1, by decoding into device scratch through the usual decode path and comparing
// behind it (fid_compare_kernel). One thread per clip and channel then walks its records in block order
// (fid_totals_kernel): only the per-clip records, and the block records when asked for, come back over PCIe.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <string>
#include <vector>

#include "batch_internal.hpp"
#include "container.hpp"
#include "decode_plan.hpp"
#include "devmem.hpp"
#include "fidelity_kernels.hpp"

static_assert(sizeof(FidTotal) == sizeof(flo_fidelity) && sizeof(FidPublicBlock) == sizeof(flo_fidelity_block),
              "device records mirror the C ABI's");

namespace {

// FLO_FIDELITY_UNFUSED=1 (read per call): lossy batches decode into scratch and compare behind the decode
bool unfused() {
    const char *e = std::getenv("FLO_FIDELITY_UNFUSED");
    return e && std::atoi(e) != 0;
}

// The clips' descriptors: blocks of the decoded signal (records) and of the compared range (public), running.
uint64_t plan_clips(std::vector<FidClipDev> &cl, uint64_t *pub_off, uint64_t &dec_blocks) {
    uint64_t pub = 0;
    dec_blocks = 0;
    for (size_t i = 0; i < cl.size(); i++) {
        const uint64_t cmp = cl[i].src_frames < cl[i].dec_frames ? cl[i].src_frames : cl[i].dec_frames;
        cl[i].blk0 = dec_blocks;
        cl[i].pub0 = pub;
        if (pub_off) pub_off[i] = pub;
        pub += (cmp + 1023) / 1024;
        dec_blocks += (cl[i].dec_frames + 1023) / 1024;
    }
    if (pub_off) pub_off[cl.size()] = pub;
    return pub;
}

// the totals of every clip from its records, and the public block records if `blocks`; copied back, stream idle on return
int finish(flo_ctx *c, const FidClipDev *d_cl, size_t n_clips, int ch, const FidBlockDev *d_blk, uint64_t n_pub,
           flo_fidelity *out, flo_fidelity_block *blocks) {
    DevBuf<FidTotal> d_out;
    DevBuf<FidPublicBlock> d_pub;
    QuiesceOnExit q(c);
    const size_t n_out = n_clips * (size_t)ch;
    if (!d_out.alloc(n_out) || (blocks && !d_pub.alloc(n_pub * ch))) return fail(c, FLO_ERR_NOMEM, "fidelity records");
    FidTotalsArgs A{};
    A.clip = d_cl;
    A.blk = d_blk;
    A.out = d_out.p;
    A.pub = blocks ? d_pub.p : nullptr;
    A.n_clips = (unsigned)n_clips;
    A.channels = ch;
    int rc = timed_launch(c, "fidelity", [&] { return launch_fid_totals(A, c->stream); });
    if (rc != FLO_OK) return rc;
    HIPCHK(c, hipMemcpyAsync(out, d_out.p, n_out * sizeof(flo_fidelity), hipMemcpyDeviceToHost, c->stream));
    if (blocks && n_pub)
        HIPCHK(c, hipMemcpyAsync(blocks, d_pub.p, n_pub * ch * sizeof(flo_fidelity_block), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return FLO_OK;
}

// fid_compare_kernel over decoded PCM in device memory (clips' dec offsets set)
int compare_decoded(flo_ctx *c, const float *src, const float *dec, const FidClipDev *d_cl, size_t n_clips, int ch, FidBlockDev *d_blk,
                    uint64_t dec_blocks) {
    FidCompareArgs A{};
    A.src = src;
    A.dec = dec;
    A.clip = d_cl;
    A.blk = d_blk;
    A.n_clips = (unsigned)n_clips;
    A.channels = ch;
    A.n_units = dec_blocks * (unsigned)ch;
    return timed_launch(c, "fidelity", [&] { return launch_fid_compare(A, c->stream); });
}

}  // namespace

extern "C" int flo_batch_fidelity(flo_batch *b, flo_fidelity *out, flo_fidelity_block *blocks, size_t blocks_cap, uint64_t *block_off) {
    if (!b || !block_off) return FLO_ERR_ARG;
    flo_ctx *c = b->ctx;
    if (!b->synced) return fail(c, FLO_ERR_STATE, "call flo_batch_encode + flo_batch_sync first");
    // clip i's source is the batch's device copy, clip_nsf[i] whole frames at d_pcm + clip_off[i]; dec_frames: what its file decodes to
    const size_t n = b->n_clips;
    const int ch = b->ch;
    const bool lossy = b->mode == FLO_MODE_LOSSY;
    int rc;
    std::vector<FidClipDev> cl(n);
    for (size_t i = 0; i < n; i++) {
        cl[i].src = b->clip_off[i];
        cl[i].src_frames = b->clip_nsf[i];
        if (lossy) cl[i].dec_frames = b->hops[i] > 1 ? (uint64_t)(b->hops[i] - 1) * 1024 : 0;
    }
    if (!lossy) {
        std::vector<LosslessFrameInfo> fr;
        std::vector<LosslessWrapperInfo> wr;
        const uint8_t *base = nullptr;
        std::string err;
        if (lossless_describe(b->ll, fr, wr, &base, err) != 0) return fail(c, FLO_ERR_STATE, err);
        for (const LosslessFrameInfo &f : fr)
            if (f.clip < n) cl[f.clip].dec_frames += f.samples;
    }
    uint64_t dec_blocks = 0;
    const uint64_t n_pub = plan_clips(cl, block_off, dec_blocks);
    if (!out) return FLO_OK;   // the sizing call
    if (blocks && blocks_cap < n_pub * (uint64_t)ch) return fail(c, FLO_ERR_ARG, "block record buffer too small");
    if (!n) return FLO_OK;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf<FidClipDev> d_cl;
    DevBuf<FidBlockDev> d_blk;
    DevBuf<float> d_dec;
    QuiesceOnExit q(c);
    if (!d_cl.alloc(n) || !d_blk.alloc(dec_blocks * ch)) return fail(c, FLO_ERR_NOMEM, "fidelity records");
    if (lossy && !unfused()) {   // the fused pass: lossy_decode_kernel<kDecCompare>, clip i against cmp's clip i
        HIPCHK(c, hipMemcpyAsync(d_cl.p, cl.data(), n * sizeof(FidClipDev), hipMemcpyHostToDevice, c->stream));
        const LossyCmpArgs cmp{b->d_pcm, d_cl.p, d_blk.p};
        std::vector<unsigned long long> blob_off, c0, co;
        std::vector<unsigned int> blob_len, cn;
        uint64_t total = 0;
        unsigned max_hops = 0;
        if ((rc = batch_lossy_tables(b, blob_off, blob_len, c0, cn, co, total, max_hops)) != FLO_OK) return rc;
        if (total && (rc = lossy_decode_whole(c, b->ts, b->d_out, ch, blob_off, blob_len, c0, cn, co, max_hops, nullptr, &cmp)) != FLO_OK) return rc;
    } else {
        uint64_t total = 0;
        for (size_t i = 0; i < n; i++) total += cl[i].dec_frames * (uint64_t)ch;
        if (!d_dec.alloc(total)) return fail(c, FLO_ERR_NOMEM, "fidelity decode scratch");
        std::vector<uint64_t> offs(n);
        if ((rc = flo_batch_decode(b, d_dec.p, total, offs.data())) != FLO_OK) return rc;
        for (size_t i = 0; i < n; i++) cl[i].dec = offs[i];
        HIPCHK(c, hipMemcpyAsync(d_cl.p, cl.data(), n * sizeof(FidClipDev), hipMemcpyHostToDevice, c->stream));
        if ((rc = compare_decoded(c, b->d_pcm, d_dec.p, d_cl.p, n, ch, d_blk.p, dec_blocks)) != FLO_OK) return rc;
    }
    return finish(c, d_cl.p, n, ch, d_blk.p, n_pub, out, blocks);
}

extern "C" int flo_compare(flo_ctx *c, const float *pcm, size_t n_interleaved, const uint8_t *flo, size_t len, flo_fidelity *out,
                           flo_fidelity_block *blocks, size_t blocks_cap, size_t *n_blocks) {
    if (!c) return FLO_ERR_ARG;
    if (!flo || !out || (!pcm && n_interleaved)) return fail(c, FLO_ERR_ARG, "null argument");
    HIPCHK(c, hipSetDevice(c->device));
    ParsedFile f;
    const char *perr = "";
    if (parse_file(flo, len, f, &perr) != 0) return fail(c, FLO_ERR_FORMAT, perr);
    const int ch = f.channels;
    if (ch == 0) return fail(c, FLO_ERR_FORMAT, "Failed to deserialize transform frame");
    std::vector<FidClipDev> cl(1);
    cl[0].src_frames = n_interleaved / (size_t)ch;
    std::vector<unsigned long long> blob_off;
    std::vector<unsigned int> blob_len;
    if (f.is_transform) {
        file_transform_blobs(f, blob_off, blob_len);
        cl[0].dec_frames = blob_off.size() > 1 ? (uint64_t)(blob_off.size() - 1) * 1024 : 0;
    } else {
        for (const FrameDesc &fr : f.frames) cl[0].dec_frames += fr.samples;
    }
    uint64_t dec_blocks = 0, pub_off[2];
    const uint64_t n_pub = plan_clips(cl, pub_off, dec_blocks);
    if (n_blocks) *n_blocks = (size_t)n_pub;
    if (blocks && blocks_cap < n_pub * (uint64_t)ch) return fail(c, FLO_ERR_ARG, "block record buffer too small");
    DevBuf<uint8_t> d_bytes;
    DevBuf<float> d_src, d_dec;
    DevBuf<FidClipDev> d_cl;
    DevBuf<FidBlockDev> d_blk;
    QuiesceOnExit q(c);
    const size_t n_src = cl[0].src_frames * (size_t)ch;
    if (!d_bytes.alloc(len + 32) || !d_src.alloc(n_src) || !d_cl.alloc(1) || !d_blk.alloc(dec_blocks * ch))
        return fail(c, FLO_ERR_NOMEM, "fidelity buffers");
    int rc = ctx_stager(c);
    if (rc != FLO_OK) return rc;
    {
        std::string uerr;
        std::vector<UploadSeg> segs{{d_bytes.p, flo, len}};
        if (n_src) segs.push_back({d_src.p, pcm, n_src * sizeof(float)});
        if (stager_upload(c->stager, segs, c->stream, uerr) != 0) return fail(c, FLO_ERR_DEVICE, uerr);
    }
    if (f.is_transform) {
        HIPCHK(c, hipMemcpyAsync(d_cl.p, cl.data(), sizeof(FidClipDev), hipMemcpyHostToDevice, c->stream));
        const LossyCmpArgs cmp{d_src.p, d_cl.p, d_blk.p};
        if (const unsigned nf = (unsigned)blob_off.size()) {   // the fused pass over the file's one clip
            TableSet *ts;
            if ((rc = get_tables(c, f.sample_rate, 0.5f, &ts)) != FLO_OK) return rc;
            if ((rc = lossy_decode_whole(c, ts, d_bytes.p, ch, blob_off, blob_len, {0}, {nf}, {0}, nf, nullptr, &cmp)) != FLO_OK) return rc;
        }
    } else {
        const uint64_t n_dec = cl[0].dec_frames * (uint64_t)ch;
        if (!d_dec.alloc(n_dec)) return fail(c, FLO_ERR_NOMEM, "fidelity decode scratch");
        if (n_dec) {
            LlWrapperList w;
            const uint64_t out_sf = file_ll_wrappers(f, w);
            if ((rc = ll_decode_device(c, w, out_sf, d_bytes.p, ch, d_dec.p, nullptr)) != FLO_OK) return rc;
        }
        HIPCHK(c, hipMemcpyAsync(d_cl.p, cl.data(), sizeof(FidClipDev), hipMemcpyHostToDevice, c->stream));
        if ((rc = compare_decoded(c, d_src.p, d_dec.p, d_cl.p, 1, ch, d_blk.p, dec_blocks)) != FLO_OK) return rc;
    }
    return finish(c, d_cl.p, 1, ch, d_blk.p, n_pub, out, blocks);
}
