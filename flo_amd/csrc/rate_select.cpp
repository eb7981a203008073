// rate_select.cpp — see rate_select.hpp.
#include "rate_select.hpp"

namespace flo {

float rate_clamp_quality(float q) {
    if (q != q) return 0.0f;
    return q < 0.0f ? 0.0f : (q > 1.0f ? 1.0f : q);
}

RatePick rate_pick(size_t n, const float *qualities, const uint64_t *sizes, uint64_t budget) {
    RatePick best, lowest;
    bool have = false;
    float best_q = 0.0f, low_q = 0.0f;
    for (size_t j = 0; j < n; j++) {
        const float q = rate_clamp_quality(qualities[j]);
        if (j == 0 || q < low_q) {
            low_q = q;
            lowest.index = (uint32_t)j;
        }
        if (sizes[j] <= budget && (!have || q > best_q)) {
            have = true;
            best_q = q;
            best.index = (uint32_t)j;
            best.fits = 1;
        }
    }
    return have ? best : lowest;
}

}  // namespace flo
