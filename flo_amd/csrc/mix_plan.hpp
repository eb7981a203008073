// mix_plan.hpp — mixing and concatenation of resident batches (flo_batch_mix, flo_mix; mix.cpp, mix_kernels.hip): the checks
// of a list of parts with their messages, the per-clip prefix of parts, the tile prefix and the class of a part on a tile.
// Plain C++: no HIP headers, so a host test builds it with g++ alone (tests/native/mix_plan_test.cpp); the class is inline
// here because the kernel branches on the same function.
//
// The definition: output clip k has T_k frames of C channels. Part p of clip k is live on output frame t when
// at <= t < at + frames, t < T_k and start + (t - at) < N. With u = t - at and v = frames - 1 - u the fade weight is the edit
// stage's (w_in = fl32(u / fade_in) if u < fade_in, w_out = fl32(v / fade_out) if v < fade_out, w their product where both
// apply); the part's coefficient is k_p = gain where no fade applies, else fl32(gain * w). Output sample (t, c): a = +0.0f,
// then a = fmaf(k_p, x_p[start + u, c], a) for every live part of the clip in list order.
//
// Geometry: the edit stage's. A tile is F = edit_tile_frames(C) consecutive output frames of one output clip from a multiple
// of F on; F * C is a multiple of 4 floats and output clips start 16-byte aligned, so every tile does.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/flo_hip.h"
#include "edit_plan.hpp"

namespace flo {

constexpr uint32_t kMixThreads = kEditThreads;
constexpr uint32_t kMixNone = 0, kMixWhole = 1, kMixPartial = 2;

// one part as the kernel reads it (64 bytes)
struct MixPart {
    const float *src;           // the source clip's first sample (d_pcm + clip_off of its batch)
    unsigned long long n_src;   // N: whole sample-frames of the source clip
    unsigned long long start, frames, at;
    unsigned int fade_in, fade_out;
    float gain;
    unsigned int unused[3];
};
// one output clip as the kernel reads it (16 bytes)
struct MixClip {
    unsigned long long dst_off;   // floats: the output clip's first sample
    unsigned long long frames;    // T
};
static_assert(sizeof(MixPart) == 64, "MixPart is 64 bytes");
static_assert(sizeof(MixClip) == 16, "MixClip is 16 bytes");
static_assert(sizeof(flo_mix_part) == 48, "flo_mix_part is 48 bytes");

// frames of the part that have a source frame: min(frames, N - start), 0 from start >= N on
FLO_EP_HD unsigned long long mix_avail(const MixPart &p) {
    const unsigned long long left = p.start >= p.n_src ? 0ull : p.n_src - p.start;
    return p.frames < left ? p.frames : left;
}
// The class of a checked part on the tile of output frames [t0, t0 + nf) of a clip of T frames (nf >= 1, t0 + nf <= T):
// kMixNone: live on no frame of the tile; kMixWhole: live on every frame of the tile, none of them inside one of its fades;
// kMixPartial: anything else.
FLO_EP_HD uint32_t mix_part_in_tile(const MixPart &p, unsigned long long T, unsigned long long t0, uint32_t nf) {
    const unsigned long long t1 = t0 + nf, lo = p.at;
    unsigned long long hi = lo + mix_avail(p);   // (at + frames does not wrap: checked)
    hi = hi < T ? hi : T;
    if (hi <= lo || t1 <= lo || t0 >= hi) return kMixNone;
    if (t0 < lo || t1 > hi) return kMixPartial;
    const unsigned long long a = t0 - lo, b = t1 - lo;   // the part's frames [a, b) are the tile's
    if (a < p.fade_in) return kMixPartial;
    if (p.fade_out && b > p.frames - p.fade_out) return kMixPartial;
    return kMixWhole;
}

// One source batch as the checks see it.
struct MixSource {
    bool present = false;          // the pointer is not NULL
    const void *ctx = nullptr;
    uint32_t rate = 0, channels = 0;
    size_t n_clips = 0;
    const uint64_t *clip_frames = nullptr;   // [n_clips] N_i
};
// The checks of flo_batch_mix: ppre[k] = parts in front of output clip k (n_out + 1 entries) and pre, the tile prefix of
// clip_tiles(out_frames, n_out, edit_tile_frames(C)); or false with a message that names the quantity.
bool mix_check(const MixSource *srcs, size_t n_srcs, size_t n_out, const uint64_t *out_frames, size_t n_parts, const flo_mix_part *parts,
               std::vector<uint32_t> &ppre, std::vector<uint32_t> &pre, std::string &err);

}  // namespace flo
