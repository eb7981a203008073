// curve_pass.hpp — what the passes over candidate qualities share (flo_batch_size_curve, rate.cpp; flo_batch_encode_ladder,
// ladder.cpp): the per-candidate constants, the scratch of the frame-parallel level rows, and per group of clips
// (partition_clips, ladder_plan.hpp) pass 1 and the scan. Also the two pieces of a lossy batch's encode that those share
// with batch.cpp: the partial sample-frame in the padding and the finish arguments of a lossy file. Not part of the C ABI.
#pragma once
#include "batch_internal.hpp"
#include "container_kernels.hpp"
#include "devmem.hpp"
#include "ladder_plan.hpp"
#include "lossy_kernels.hpp"

// A caller who wrote all n_interleaved floats through flo_batch_clip_device_ptr left a partial sample-frame in the zero
// padding behind the clip: it is not part of the clip (encoder.rs:174). Enqueues the clears.
int batch_zero_partial_frames(flo_batch *b);

// Per-candidate constants: the tables an encode at that quality gets (get_tables -> build_lossy_tables). levels: null, or
// [n_q] the header's quality level of every candidate.
int curve_args_fill(flo_batch *b, size_t n_q, const float *qualities, CurveArgs &C, unsigned char *levels);

// The level rows of the largest group, the +inf marks of every clip (LossyArgs::inf_mark, a tag per group) and every clip's
// first frame inside its group. Declare it in front of the function's QuiesceOnExit.
struct LevelRows {
    DevBuf<float> d_at, d_sprev, d_bmax;   // d_bmax: stereo only
    DevBuf<unsigned long long> d_inf, d_rel;
    std::vector<uint64_t> rel;   // [n_clips] host copy of d_rel (kept: the upload reads it)
    uint64_t max_frames = 0;     // of the largest group
    bool alloc(const flo_batch *b, const std::vector<ClipGroup> &groups);
    int enqueue_clear(flo_batch *b);   // rel goes up, the marks are zeroed
};
// Group g's clips into C.A, then pass 1 and the scan under the two profile names
int level_rows_pass(flo_batch *b, CurveArgs &C, const LevelRows &R, const ClipGroup &g, const char *bands, const char *scan);

// header, TOC and CRC32 of lossy files (writer.rs:132-224; encoder.rs:229-238 parameters): frames of 1024 samples, 16 bits,
// level 5. crc_out, crc_ready and epoch are the caller's.
FinishArgs lossy_finish_args(const flo_batch *b, uint8_t *out, const unsigned long long *data_off, const unsigned long long *clip_bytes,
                             const unsigned long long *clip_frame0, const unsigned int *clip_frames, const unsigned int *frame_size,
                             size_t n_files, unsigned short flags, unsigned int *part_reg, unsigned int max_frames);
