// ladder_plan.cpp — see ladder_plan.hpp.
#include "ladder_plan.hpp"

namespace flo {

uint64_t level_row_bytes(unsigned channels) { return (uint64_t)channels * 32 * sizeof(float) * (channels == 2 ? 3 : 2); }

uint64_t ladder_frame_bytes(unsigned channels, size_t n_q, unsigned slot_bytes) {
    return (uint64_t)n_q * ((uint64_t)slot_bytes + 4 + 8) + level_row_bytes(channels);
}

std::vector<ClipGroup> partition_clips(const uint32_t *hops, size_t n_clips, uint64_t bytes_per_frame, uint64_t limit) {
    std::vector<ClipGroup> groups;
    // frames a group may hold (a division, so that frames * bytes_per_frame cannot overflow)
    const uint64_t cap = bytes_per_frame ? limit / bytes_per_frame : UINT64_MAX;
    for (size_t i = 0; i < n_clips;) {
        ClipGroup g;
        g.first = i;
        while (i < n_clips && (g.count == 0 || g.frames + hops[i] <= cap)) {
            g.frames += hops[i];
            g.max_hops = hops[i] > g.max_hops ? hops[i] : g.max_hops;
            g.count++;
            i++;
        }
        groups.push_back(g);
    }
    return groups;
}

}  // namespace flo
