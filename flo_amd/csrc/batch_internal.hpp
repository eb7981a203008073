// batch_internal.hpp — the device-resident batch (flo_batch_*, include/flo_hip.h) as the library's source files see it:
// batch.cpp makes, encodes and releases it; decode.cpp, fidelity.cpp, analysis.cpp, dist.cpp, stages.cpp, stream.cpp,
// rate.cpp, ladder.cpp and curve_pass.cpp read it; resample.cpp, normalize.cpp and edit.cpp make one from another, through
// the helpers at the end of this file. Not part of the C ABI.
#pragma once
#include <functional>
#include <vector>

#include "ctx_internal.hpp"
#include "encode_plan.hpp"
#include "lossless_kernels.hpp"

struct flo_batch {
    flo_ctx *ctx = nullptr;
    int mode = 0;
    size_t n_clips = 0;
    uint32_t sr = 0;
    uint8_t ch = 0;
    float qol = 0;
    uint8_t bit_depth = 16;
    TableSet *ts = nullptr;
    // plan (host)
    std::vector<uint64_t> n_il, clip_off, clip_nsf, clip_frame0, out_off, out_cap;
    std::vector<uint64_t> file_off, h_file_bytes;   // finished file = [file_off, file_off + head_bytes(frames) + DATA)
    std::vector<uint32_t> hops;
    uint64_t total_frames = 0, total_floats = 0, out_bytes = 0;
    // device
    float *d_pcm = nullptr;
    uint64_t *d_plan = nullptr;  // clip_off | clip_nsf | clip_frame0 | out_off
    uint32_t *d_hops = nullptr;
    uint8_t *d_out = nullptr;
    uint32_t *d_frame_size = nullptr;
    uint64_t *d_clip_bytes = nullptr;
    uint32_t *d_crc = nullptr, *d_part = nullptr, *d_next = nullptr;
    // stereo chain encode of many clips (form 5): the CRC in the launch's idle tail. d_next holds two sets of counters
    // (claim, done-queue tail and head), used by launches of alternating epoch parity; each launch zeroes the other set
    uint32_t *d_crc_ready = nullptr;          // [n_clips] epoch of the launch whose tail left the clip's slice registers
    unsigned long long *d_done_q = nullptr;   // [n_clips] done queue entries (epoch << 32 | clip)
    uint32_t epoch = 0;                       // of the last form-5 launch; the next is epoch + 1 (never 0)
    uint64_t *pin_sizes = nullptr;            // pinned [n_clips]: DATA sizes, copied behind finish_files (sizes_queued)
    bool sizes_queued = false;
    float *d_bmax = nullptr;   // band maxima of every frame (frame-parallel form: pass 1 -> pass 2)
    unsigned long long *d_inf_mark = nullptr;   // [n_clips][ch][32] first frame of a +inf level (LossyArgs::inf_mark), zeroed once
    uint32_t inf_tag = 0;                       // of the last frame-parallel launch sequence
    void *d_coef = nullptr;    // ... and, for a few long stereo clips, every frame's coefficients (8 KB per frame)
    float *d_at = nullptr, *d_sprev = nullptr;
    uint8_t *d_slots = nullptr;
    uint64_t *d_frame_off = nullptr;
    // analysis buffers (optional)
    float *d_dbg_coeffs = nullptr;
    short *d_dbg_q = nullptr;
    unsigned short *d_dbg_sfw = nullptr;
    const float *d_in_coeffs = nullptr;
    uint64_t *d_pack_plan = nullptr;
    uint64_t *pin_plan = nullptr;        // pinned: clip plan (4 n) | hops (n u32) | pack plan (3 n): read by asynchronous copies
    hipEvent_t ev_pack_plan = nullptr;
    unsigned long long *d_stamps = nullptr;
    int exact = 0;
    LossyPlan plan;   // of the last lossy flo_batch_encode
    // results (host, valid after sync)
    bool encoded = false, synced = false, encode_failed = false;
    bool pcm_written = false;   // an upload, a fill or a device pointer handed out: the batch holds PCM (flo_batch_size_curve)
    std::vector<uint64_t> h_clip_bytes;
    std::vector<uint32_t> h_frame_size;
    // lossless
    LosslessPlan *ll = nullptr;
    // a batch made from another by a launch that is only enqueued (flo_batch_resample, flo_batch_edit): that launch's work
    // block (work_block_get), device and pinned, kept until the batch goes
    void *d_work = nullptr, *pin_work = nullptr;
    // lossy clips of n_interleaved % ch != 0 uploaded from the host: the trailing partial sample-frame, which the encoder
    // drops (so it stays out of the device copy) but the analysis covers (flo_batch_analyze_all)
    std::vector<std::vector<float>> tail;
    void keep_tail(size_t clip, const float *pcm) {
        if (tail.size() != n_clips) tail.resize(n_clips);
        const uint64_t whole = clip_nsf[clip] * ch;
        if (mode == FLO_MODE_LOSSY && n_il[clip] > whole) tail[clip].assign(pcm + whole, pcm + n_il[clip]);
        else tail[clip].clear();
    }
};

// all clips of a batch from host buffers, through the pinned staging ring (batch.cpp)
int batch_upload_all(flo_batch *b, const float *const *pcm, hipStream_t stream = nullptr);

// ---- one batch made from another (resample.cpp, normalize.cpp, edit.cpp; all of these are batch.cpp's) -----------------
// A new batch of n_out clips of n_il[k] floats each at `sr` and `ch`, otherwise like src: its mode and quality (or level),
// its bit_depth and exact. The one place that knows what a derived batch inherits.
int batch_derive(const flo_batch *src, size_t n_out, const size_t *n_il, uint32_t sr, uint8_t ch, flo_batch **out);
// ... on its way to the caller: destroyed on scope exit (which waits for the stream first) unless released
struct BatchHold {
    flo_batch *b = nullptr;
    ~BatchHold() {
        if (b) flo_batch_destroy(b);
    }
    flo_batch *release() {
        flo_batch *r = b;
        b = nullptr;
        return r;
    }
};
// n_il[i] / ch of every clip, whole sample-frames: a kept partial frame (flo_batch::tail) is not carried over
std::vector<uint64_t> batch_whole_frames(const flo_batch *b);
// FLO_ERR_STATE with "<who>: the batch holds no PCM yet"
int batch_no_pcm(const flo_batch *b, const char *who);
// The work block of a launch that is only enqueued: `bytes` of pinned memory from the stager to fill, and a pool block to
// copy them into. Each is recorded in the caller's pair as soon as it exists, so the owner releases what there is: a batch
// passes its own pair (pin_work, d_work; flo_batch_destroy), flo_resample its locals. Pool errors read "<what>: <HIP's text>".
int work_block_get(flo_ctx *c, size_t bytes, const char *what, void *&pin, void *&dev);
// One host clip through a batch operation and back: a one-clip lossless batch of `n_il` floats is made and uploaded, op
// makes another from it, and clip 0 of that comes back as a malloc'd block of *n_out floats (n_out nullable). Both batches
// are gone on return. Device errors of the copy back read "<who>: <HIP's text>".
int batch_one_shot(flo_ctx *c, const char *who, const float *pcm, size_t n_il, uint32_t sr, uint8_t ch,
                   const std::function<int(flo_batch *, flo_batch **)> &op, float **out, size_t *n_out);

// One host clip and one host response through a convolution of batches and back (flo_convolve, flo_convolve_fft;
// convolve.cpp): both are uploaded, op makes the batch, clip 0 comes back malloc'd. Messages of `batch_who` read `who`.
typedef int (*ConvBatchOp)(flo_batch *, flo_batch *, size_t, const flo_conv_job *, flo_batch **);
int conv_one_clip(flo_ctx *c, const std::string &who, const std::string &batch_who, ConvBatchOp op, const float *pcm, size_t n_interleaved,
                  const float *ir, size_t ir_interleaved, uint32_t sample_rate, uint8_t channels, uint8_t ir_channels, const flo_conv_job *job,
                  float **out, size_t *n_out);

// The frame and clip tables of a synced lossy batch's decode, read from the encoder's own records: clip i's PCM at
// co[i] floats, `total` floats in all (decode.cpp: flo_batch_decode, and the fidelity reports' fused pass)
int batch_lossy_tables(flo_batch *b, std::vector<unsigned long long> &blob_off, std::vector<unsigned int> &blob_len,
                       std::vector<unsigned long long> &c0, std::vector<unsigned int> &cn, std::vector<unsigned long long> &co,
                       uint64_t &total, unsigned &max_hops);
