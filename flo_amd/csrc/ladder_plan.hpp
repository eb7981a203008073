// ladder_plan.hpp — how the passes over candidate qualities (flo_batch_size_curve, rate.cpp; flo_batch_encode_ladder,
// ladder.cpp) cut a batch into groups of consecutive clips whose device scratch stays under a limit. Plain C++: no HIP
// headers, so a host test builds it with g++ alone (tests/native/ladder_plan_test.cpp). Where the finished files come to
// lie: file_layout.hpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace flo {

struct ClipGroup {
    size_t first = 0, count = 0;   // clips first .. first + count - 1
    uint64_t frames = 0;           // their frames in all
    uint32_t max_hops = 0;         // frames of the longest of them
};

// Scratch of one frame's level rows: per channel the 32-float rows of the frame-parallel levels (a_t, s_prev, and the band
// maxima the stereo pass 1 leaves). All the scratch of a size curve's frame.
uint64_t level_row_bytes(unsigned channels);
// Scratch of one frame of a ladder's group: per rung a slot, a frame size and a frame offset; and the level rows.
uint64_t ladder_frame_bytes(unsigned channels, size_t n_q, unsigned slot_bytes);

// Consecutive clips, in order, every clip in exactly one group: a group takes clips while (its frames + the next clip's)
// * bytes_per_frame <= limit; a clip that alone exceeds the limit is a group of its own. Clips of no frames cannot occur
// (a clip of no samples still has one frame), but a count of 0 would join the group at hand.
std::vector<ClipGroup> partition_clips(const uint32_t *hops, size_t n_clips, uint64_t bytes_per_frame, uint64_t limit);

}  // namespace flo
