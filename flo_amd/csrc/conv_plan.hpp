// conv_plan.hpp — FIR filtering and convolution of resident batches (flo_batch_convolve, flo_convolve, flo_conv_geometry;
// convolve.cpp, conv_kernels.hip): the checks of a list of jobs with their messages, the number of taps of a job, the tile
// prefix and the geometry. Plain C++: no HIP headers, so a host test builds it with g++ alone
// (tests/native/conv_plan_test.cpp); the geometry and the LDS index are inline here because the kernel uses the same functions.
//
// The definition: output clip k has T = frames frames of C channels; K = min(taps, P - min(ir_start, P));
// h[k, c] is frame ir_start + k of the response clip, channel (Ch == 1 ? 0 : c). Output sample (t, c): a = +0.0f, then for
// k = 0 .. K - 1 ascending, m = t + skip - k, xv = x[m, c] if 0 <= m < N else +0.0f, a = fmaf(h[k, c], xv, a).
//
// Geometry: a tile is kConvTileFrames consecutive output frames of one output clip from a multiple of it on; a lane owns
// kConvLaneOutputs consecutive frames of it; taps are staged kConvTapChunk at a time. Both kernel variants (stereo float2
// frames; planes of floats for every other channel count) share it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/flo_hip.h"

#if defined(__HIPCC__)
#define FLO_CV_HD __host__ __device__ inline
#else
#define FLO_CV_HD inline
#endif

namespace flo {

constexpr uint32_t kConvThreads = 256;
constexpr uint32_t kConvLaneOutputs = 8;                                 // the register window's length
constexpr uint32_t kConvTileFrames = kConvThreads * kConvLaneOutputs;    // 2048
constexpr uint32_t kConvTapChunk = 256;                                  // a multiple of kConvLaneOutputs
constexpr uint32_t kConvMaxChannels = 8;
constexpr uint32_t kConvStaged = kConvTileFrames + kConvTapChunk - 1;    // source frames one chunk of one tile touches

// staged frame s lies at this LDS element: one element of skew per kConvLaneOutputs frames, so that lanes, which read
// kConvLaneOutputs frames apart, are an odd number of elements apart (9: no two of 32 lanes share a bank, 4-byte elements on
// 32 banks and 8-byte elements on 64 alike)
FLO_CV_HD uint32_t conv_lds_index(uint32_t s) { return s + s / kConvLaneOutputs; }
constexpr uint32_t kConvLdsElems = (kConvStaged - 1) + (kConvStaged - 1) / kConvLaneOutputs + 1;

// one output clip as the kernel reads it (64 bytes)
struct ConvJob {
    const float *src;            // the source clip's first sample (d_pcm + clip_off of src)
    const float *ir;             // h[0, 0]: the response clip's frame ir_start (never read when taps == 0)
    unsigned long long n_src;    // N
    unsigned long long skip;     // min(skip, N + K): from N + K on every tap of every output meets +0.0 alike
    unsigned long long frames;   // T
    unsigned long long dst_off;  // floats: the output clip's first sample
    unsigned int taps;           // K
    unsigned int ir_channels;    // Ch
    unsigned int unused[2];
};
static_assert(sizeof(ConvJob) == 64, "ConvJob is 64 bytes");
static_assert(sizeof(flo_conv_job) == 40, "flo_conv_job is 40 bytes");

// K of a job against a response clip of P frames
FLO_CV_HD uint32_t conv_taps(uint32_t taps, uint64_t P, uint64_t ir_start) {
    const uint64_t left = P - (ir_start < P ? ir_start : P);
    return left < taps ? (uint32_t)left : taps;
}
// the skip the kernel works with (see ConvJob::skip); N + K does not wrap: N is a clip's frame count, K <= 65536
FLO_CV_HD uint64_t conv_skip(uint64_t skip, uint64_t N, uint32_t K) { return skip < N + K ? skip : N + K; }

// One batch as the checks see it.
struct ConvSource {
    bool present = false;          // the pointer is not NULL
    const void *ctx = nullptr;
    uint32_t rate = 0, channels = 0;
    size_t n_clips = 0;
    const uint64_t *clip_frames = nullptr;   // [n_clips] whole frames
};
// What differs between the callers of conv_check: the direct path's limits are the default; the partitioned FFT path
// (fftconv_plan.cpp) has a limit and a tile of its own.
struct ConvLimits {
    uint32_t max_taps = FLO_CONV_MAX_TAPS;
    const char *max_taps_name = "FLO_CONV_MAX_TAPS";
    uint64_t tile_frames = kConvTileFrames;
};
// The checks of flo_batch_convolve: K[k] of every job and pre, the tile prefix of clip_tiles(frames, n_out, lim.tile_frames);
// or false with a message that names the quantity.
bool conv_check(const ConvSource &src, const ConvSource &irs, size_t n_out, const flo_conv_job *jobs, std::vector<uint32_t> &K,
                std::vector<uint32_t> &pre, std::string &err, const ConvLimits &lim = ConvLimits());

// flo_fir_design without the C wrapping (fir_design.cpp): the table in f64, or false with a message
bool fir_design(uint32_t kind, uint32_t rate, double f_lo, double f_hi, uint32_t taps, double beta, std::vector<double> &h, std::string &err);

}  // namespace flo
