// ladder_plan.hpp — how flo_batch_encode_ladder (ladder.cpp) cuts a batch into groups of consecutive clips whose device
// scratch stays under a limit, and where every finished file of the ladder comes to lie. Plain C++: no HIP headers, so a
// host test builds it with g++ alone (tests/native/ladder_plan_test.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace flo {

struct LadderGroup {
    size_t first = 0, count = 0;   // clips first .. first + count - 1
    uint64_t frames = 0;           // their frames in all
    uint32_t max_hops = 0;         // frames of the longest of them
};

// Scratch of one frame of a group: per rung a slot, a frame size and a frame offset; per channel the 32-float rows of the
// frame-parallel levels (a_t, s_prev, and the band maxima the stereo pass 1 leaves).
uint64_t ladder_frame_bytes(unsigned channels, size_t n_q, unsigned slot_bytes);

// Consecutive clips, in order, every clip in exactly one group: a group takes clips while (its frames + the next clip's)
// * bytes_per_frame <= limit; a clip that alone exceeds the limit is a group of its own. Clips of no frames cannot occur
// (a clip of no samples still has one frame), but a count of 0 would join the group at hand.
std::vector<LadderGroup> ladder_partition(const uint32_t *hops, size_t n_clips, uint64_t bytes_per_frame, uint64_t limit);

// The resident layout: rung-major, file (rung j, clip i) at offsets[j * n_clips + i], every offset a multiple of 16;
// returns the bytes in all. sizes: [n_q][n_clips] finished file bytes (header + TOC + DATA).
uint64_t ladder_layout(const uint64_t *sizes, size_t n_files, uint64_t *offsets);

}  // namespace flo
