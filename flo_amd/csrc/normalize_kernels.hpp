// normalize_kernels.hpp — the launches of the normalisation kernels (normalize_kernels.hip) as normalize.cpp sees them.
#pragma once
#include <hip/hip_runtime.h>

#include "normalize_plan.hpp"

namespace flo {

struct NormArgs {
    const float *src = nullptr;   // interleaved f32: clip i's frames[i] sample-frames at src + src_off[i]
    float *dst = nullptr;         // clip i at dst + dst_off[i]; nothing else is written (unused by the peak launch)
    const float *table = nullptr; // h[4][64]
    const unsigned long long *src_off = nullptr, *dst_off = nullptr, *frames = nullptr;   // [n_clips]
    const unsigned int *pre = nullptr;     // [n_clips + 1] tiles in front of every clip (clip_tiles)
    const float *gain = nullptr;           // [n_clips]
    const unsigned int *copy = nullptr;    // [n_clips] non-zero: the clip is copied bit for bit
    unsigned long long *limited = nullptr; // [n_clips] frames with s < 2^24, from 0
    unsigned int *min_q = nullptr;         // [n_clips] the smallest s, from 2^24
    unsigned int *peak_bits = nullptr;     // [n_clips] the peak launch: max of the magnitudes' bit patterns, from 0
    unsigned int n_clips = 0, channels = 0, lookahead = 0, no_skip = 0;
    float ceiling = 0, bound = 0;
};

// Each: one workgroup per tile of the flat list (n_tiles = pre[n_clips] > 0); 0 or a hipError_t.
// peak_bits[i] = max over the clip's frames of the bits of p[n] with y = x; tiles of norm_tile_frames(0) frames
int launch_norm_peak(const NormArgs &a, unsigned int n_tiles, hipStream_t stream);
// dst = fl32(src * gain) or a copy; tiles of norm_tile_frames(0) frames
int launch_norm_gain(const NormArgs &a, unsigned int n_tiles, hipStream_t stream);
// the limiter; tiles of norm_tile_frames(lookahead) frames
int launch_norm_limit(const NormArgs &a, unsigned int n_tiles, hipStream_t stream);

}  // namespace flo
