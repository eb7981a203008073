// edit_plan.hpp — trimming, fades, padding and channel remixing of resident batches (flo_batch_edit, flo_batch_active_range,
// flo_edit, flo_edit_tile_frames; edit.cpp, edit_kernels.hip): the checks of a list of segments with their messages, the tile
// geometry and the class of a tile. Plain C++: no HIP headers, so a host test builds it with g++ alone
// (tests/native/edit_plan_test.cpp); the geometry and the class are inline here because the kernel uses the same functions.
//
// The definition: output clip k is T = pad_head + frames + pad_tail frames of Cout channels; output frame t with
// u = t - pad_head is +0.0 where u < 0, u >= frames or start + u >= N, else the mix of source frame start + u times the fade
// weights of u.
//
// Geometry: a tile is F = edit_tile_frames(Cout) consecutive output frames of one output clip from a multiple of F on; F * Cout
// is a multiple of 4 floats, and output clips start 16-byte aligned, so every tile does. A tile's class is a set of two bits:
// kEditEdge when it holds a frame of a pad or a frame whose source lies past the clip's end, kEditFaded when it holds a
// frame of the cut inside a fade; neither (kEditInterior): every frame is the plain mix of a source frame.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/flo_hip.h"

#if defined(__HIPCC__)
#define FLO_EP_HD __host__ __device__ inline
#else
#define FLO_EP_HD inline
#endif

namespace flo {

constexpr uint32_t kEditThreads = 256;
constexpr uint32_t kEditTileFloats = 4096;    // four 16-byte stores per lane
constexpr uint32_t kEditMaxMix = 8;           // channels on either side of a matrix
constexpr uint32_t kEditMaxFade = 1u << 24;   // fades stay below it: u and v convert to f32 exactly
constexpr uint32_t kEditInterior = 0, kEditEdge = 1, kEditFaded = 2;

// one output clip as the kernel reads it (64 bytes)
struct EditSeg {
    unsigned long long src_off;   // floats: the source clip's first sample
    unsigned long long n_src;     // N: whole sample-frames of the source clip
    unsigned long long start, frames;
    unsigned long long dst_off;   // floats: the output clip's first sample
    unsigned int pad_head, pad_tail, fade_in, fade_out;
    unsigned int unused[2];
};
static_assert(sizeof(EditSeg) == 64, "EditSeg is 64 bytes");
static_assert(sizeof(flo_edit_segment) == 40, "flo_edit_segment is 40 bytes");

// output frames of one tile (out_channels 1 .. 255): a multiple of 4, so F * Cout floats are whole 16-byte units
FLO_EP_HD uint32_t edit_tile_frames(uint32_t out_channels) { return (kEditTileFloats / out_channels) & ~3u; }
// T of a checked segment
FLO_EP_HD unsigned long long edit_out_frames(const EditSeg &s) { return (unsigned long long)s.pad_head + s.frames + s.pad_tail; }
// frames of the cut that have a source frame: min(frames, N - start), 0 from start >= N on
FLO_EP_HD unsigned long long edit_avail(const EditSeg &s) {
    const unsigned long long left = s.start >= s.n_src ? 0ull : s.n_src - s.start;
    return s.frames < left ? s.frames : left;
}
// the class of tile `tile` (of F frames) of a checked segment; the tile holds output frames [tile * F, min(.. + F, T))
FLO_EP_HD uint32_t edit_tile_class(const EditSeg &s, unsigned long long tile, uint32_t F) {
    const unsigned long long T = edit_out_frames(s), t0 = tile * F, t1 = t0 + F < T ? t0 + F : T;
    const unsigned long long lo = s.pad_head, hi = lo + s.frames;
    uint32_t cls = kEditInterior;
    if (t0 < lo || t1 > hi) cls |= kEditEdge;
    const unsigned long long a = (t0 > lo ? t0 : lo) - lo, b = (t1 < hi ? t1 : hi) - lo;   // the cut's frames [a, b) of the tile
    if (t1 > lo && t0 < hi && a < b) {
        if (b > edit_avail(s)) cls |= kEditEdge;
        if (a < s.fade_in) cls |= kEditFaded;
        if (s.fade_out && b > s.frames - s.fade_out) cls |= kEditFaded;
    }
    return cls;
}

// What a list of segments is cut from.
struct EditSource {
    size_t n_clips = 0;
    const uint64_t *clip_frames = nullptr;   // [n_clips] N_i
    uint32_t channels = 0;                   // Cin
    bool lossy = false;
};
// The checks of flo_batch_edit: T[k] of every segment, or false with a message that names the quantity.
bool edit_check(const EditSource &src, size_t n_out, const flo_edit_segment *segs, uint32_t out_channels, const float *matrix,
                std::vector<uint64_t> &T, std::string &err);
// threshold >= 0 and not NaN
bool edit_threshold(float threshold, std::string &err);
// (the flat work list of a launch: clip_tiles of every clip's frames in tiles of edit_tile_frames(Cout), clip_tiles.hpp)
// The matrix as the kernel takes it: rows of kEditMaxMix, zeros elsewhere (a checked matrix)
void edit_matrix_rows(const float *matrix, uint32_t in_channels, uint32_t out_channels, float (&rows)[kEditMaxMix * kEditMaxMix]);

}  // namespace flo
