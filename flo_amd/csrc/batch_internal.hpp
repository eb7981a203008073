// batch_internal.hpp — the device-resident batch (flo_batch_*, include/flo_hip.h) as the library's source files see it:
// batch.cpp makes, encodes and releases it; decode.cpp, fidelity.cpp, analysis.cpp, dist.cpp, stages.cpp, stream.cpp,
// rate.cpp, ladder.cpp and curve_pass.cpp read it; resample.cpp, normalize.cpp and edit.cpp make one from another. Not part of the C ABI.
#pragma once
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
    // a batch made by flo_batch_resample (resample.cpp): the filter table and work list of the launch that fills it, device
    // and pinned, kept until the batch goes (the launch is only enqueued)
    void *d_resample = nullptr, *pin_resample = nullptr;
    // a batch made by flo_batch_edit (edit.cpp): the segments and tile prefix of the launch that fills it, kept likewise
    void *d_edit = nullptr, *pin_edit = nullptr;
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
// The frame and clip tables of a synced lossy batch's decode, read from the encoder's own records: clip i's PCM at
// co[i] floats, `total` floats in all (decode.cpp: flo_batch_decode, and the fidelity reports' fused pass)
int batch_lossy_tables(flo_batch *b, std::vector<unsigned long long> &blob_off, std::vector<unsigned int> &blob_len,
                       std::vector<unsigned long long> &c0, std::vector<unsigned int> &cn, std::vector<unsigned long long> &co,
                       uint64_t &total, unsigned &max_hops);
