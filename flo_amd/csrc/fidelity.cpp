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

#include "container.hpp"
#include "ctx_internal.hpp"
#include "devpool.hpp"
#include "fidelity_kernels.hpp"

static_assert(sizeof(FidTotal) == sizeof(flo_fidelity) && sizeof(FidPublicBlock) == sizeof(flo_fidelity_block),
              "device records mirror the C ABI's");

namespace {

template <class T>
struct DevBuf {   // one pool block, released when the call returns
    T *p = nullptr;
    ~DevBuf() {
        if (p) pool_free(p);
    }
    bool alloc(size_t n) { return pool_alloc(&p, (n ? n : 1) * sizeof(T)) == hipSuccess; }
};
// declared behind a call's DevBufs: the stream is idle before they go back to the pool, whichever way the call ends
struct Quiesce {
    flo_ctx *c;
    ~Quiesce() {
        if (c && c->stream) hipStreamSynchronize(c->stream);
    }
};

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
    Quiesce q{c};
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
    FidBatchView v;
    int rc = batch_fidelity_view(b, v);
    if (rc != FLO_OK) return rc;
    flo_ctx *c = v.ctx;
    const size_t n = v.src_off.size();
    const int ch = v.channels;
    std::vector<FidClipDev> cl(n);
    for (size_t i = 0; i < n; i++) {
        cl[i].src = v.src_off[i];
        cl[i].src_frames = v.src_frames[i];
        cl[i].dec_frames = v.dec_frames[i];
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
    Quiesce q{c};
    if (!d_cl.alloc(n) || !d_blk.alloc(dec_blocks * ch)) return fail(c, FLO_ERR_NOMEM, "fidelity records");
    if (v.lossy && !unfused()) {
        HIPCHK(c, hipMemcpyAsync(d_cl.p, cl.data(), n * sizeof(FidClipDev), hipMemcpyHostToDevice, c->stream));
        LossyCmpArgs cmp{v.pcm, d_cl.p, d_blk.p};
        if ((rc = batch_lossy_compare(b, cmp)) != FLO_OK) return rc;
    } else {
        uint64_t total = 0;
        for (size_t i = 0; i < n; i++) total += v.dec_frames[i] * (uint64_t)ch;
        if (!d_dec.alloc(total)) return fail(c, FLO_ERR_NOMEM, "fidelity decode scratch");
        std::vector<uint64_t> offs(n);
        if ((rc = flo_batch_decode(b, d_dec.p, total, offs.data())) != FLO_OK) return rc;
        for (size_t i = 0; i < n; i++) cl[i].dec = offs[i];
        HIPCHK(c, hipMemcpyAsync(d_cl.p, cl.data(), n * sizeof(FidClipDev), hipMemcpyHostToDevice, c->stream));
        if ((rc = compare_decoded(c, v.pcm, d_dec.p, d_cl.p, n, ch, d_blk.p, dec_blocks)) != FLO_OK) return rc;
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
    if (f.is_transform) {
        uint64_t nf = 0;
        for (const FrameDesc &fr : f.frames) nf += fr.n_channels ? 1 : 0;
        cl[0].dec_frames = nf > 1 ? (nf - 1) * 1024 : 0;
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
    Quiesce q{c};
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
        LossyCmpArgs cmp{d_src.p, d_cl.p, d_blk.p};
        if ((rc = file_lossy_compare(c, f, d_bytes.p, cmp)) != FLO_OK) return rc;
    } else {
        const uint64_t n_dec = cl[0].dec_frames * (uint64_t)ch;
        if (!d_dec.alloc(n_dec)) return fail(c, FLO_ERR_NOMEM, "fidelity decode scratch");
        if (n_dec && (rc = file_lossless_decode(c, f, d_bytes.p, d_dec.p)) != FLO_OK) return rc;
        HIPCHK(c, hipMemcpyAsync(d_cl.p, cl.data(), sizeof(FidClipDev), hipMemcpyHostToDevice, c->stream));
        if ((rc = compare_decoded(c, d_src.p, d_dec.p, d_cl.p, 1, ch, d_blk.p, dec_blocks)) != FLO_OK) return rc;
    }
    return finish(c, d_cl.p, 1, ch, d_blk.p, n_pub, out, blocks);
}
