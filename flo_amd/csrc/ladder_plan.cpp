// ladder_plan.cpp — see ladder_plan.hpp.
#include "ladder_plan.hpp"

namespace flo {

uint64_t ladder_frame_bytes(unsigned channels, size_t n_q, unsigned slot_bytes) {
    const uint64_t levels = (uint64_t)channels * 32 * sizeof(float) * (channels == 2 ? 3 : 2);
    return (uint64_t)n_q * ((uint64_t)slot_bytes + 4 + 8) + levels;
}

std::vector<LadderGroup> ladder_partition(const uint32_t *hops, size_t n_clips, uint64_t bytes_per_frame, uint64_t limit) {
    std::vector<LadderGroup> groups;
    // frames a group may hold (a division, so that frames * bytes_per_frame cannot overflow)
    const uint64_t cap = bytes_per_frame ? limit / bytes_per_frame : UINT64_MAX;
    for (size_t i = 0; i < n_clips;) {
        LadderGroup g;
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

uint64_t ladder_layout(const uint64_t *sizes, size_t n_files, uint64_t *offsets) {
    uint64_t pos = 0;
    for (size_t k = 0; k < n_files; k++) {
        offsets[k] = pos;
        pos += (sizes[k] + 15) & ~(uint64_t)15;
    }
    return pos;
}

}  // namespace flo
