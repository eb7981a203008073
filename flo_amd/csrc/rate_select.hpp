// rate_select.hpp — choosing a candidate quality from a size curve (flo_rate_pick, flo_encode_batch_to_size). Plain C++:
// no HIP headers, so a host test builds it with g++ alone.
#pragma once
#include <cstddef>
#include <cstdint>

namespace flo {

// a quality as the encoder takes it (get_tables): NaN -> 0, else clamped to [0, 1]
float rate_clamp_quality(float q);

struct RatePick {
    uint32_t index = 0;   // candidate chosen
    int fits = 0;         // 1: sizes[index] <= budget; 0: nothing fits, index is the candidate of the smallest quality
};
// The candidate of the LARGEST (clamped) quality value whose size is <= budget. Every candidate is looked at: nothing
// assumes that sizes grow with quality. Equal quality values: the lower index. None fits: the candidate of the smallest
// quality value (lower index on ties), fits = 0. n must be at least 1.
RatePick rate_pick(size_t n, const float *qualities, const uint64_t *sizes, uint64_t budget);

}  // namespace flo
