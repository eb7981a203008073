// edit_plan.cpp — see edit_plan.hpp.
#include "edit_plan.hpp"

#include <cmath>

namespace flo {

bool edit_check(const EditSource &src, size_t n_out, const flo_edit_segment *segs, uint32_t out_channels, const float *matrix,
                std::vector<uint64_t> &T, std::string &err) {
    auto bad = [&](const std::string &m) {
        err = m;
        return false;
    };
    const uint32_t cin = src.channels, cout = out_channels;
    if (cout < 1) return bad("out_channels must be at least 1");
    if (!matrix && cout != cin)
        return bad("matrix is NULL but out_channels " + std::to_string(cout) + " differs from the source's " + std::to_string(cin) + " channels");
    if (matrix) {
        if (cin > kEditMaxMix) return bad("in_channels " + std::to_string(cin) + " is above the " + std::to_string(kEditMaxMix) + " a matrix supports");
        if (cout > kEditMaxMix) return bad("out_channels " + std::to_string(cout) + " is above the " + std::to_string(kEditMaxMix) + " a matrix supports");
        for (uint32_t i = 0; i < cin * cout; i++)
            if (!std::isfinite(matrix[i]))
                return bad("matrix entry [" + std::to_string(i / cin) + "][" + std::to_string(i % cin) + "] is not finite");
    }
    if (src.lossy && cout > 8) return bad("out_channels " + std::to_string(cout) + " is above the 8 a lossy batch supports");
    if (n_out && !segs) return bad("segments is NULL");
    T.assign(n_out, 0);
    const uint64_t most = (uint64_t)(SIZE_MAX / 8) / cout;   // what flo_batch_create lays out without overflow
    for (size_t k = 0; k < n_out; k++) {
        const flo_edit_segment &s = segs[k];
        const std::string at = " of segment " + std::to_string(k);
        if (s.clip >= src.n_clips) return bad("clip " + std::to_string(s.clip) + at + " is not below n_clips " + std::to_string(src.n_clips));
        if (s.reserved != 0) return bad("reserved" + at + " is " + std::to_string(s.reserved) + ", not 0");
        if (s.fade_in >= kEditMaxFade || s.fade_in > s.frames)
            return bad("fade_in " + std::to_string(s.fade_in) + at + " is longer than its " + std::to_string(s.frames) + " frames or not below 2^24");
        if (s.fade_out >= kEditMaxFade || s.fade_out > s.frames)
            return bad("fade_out " + std::to_string(s.fade_out) + at + " is longer than its " + std::to_string(s.frames) + " frames or not below 2^24");
        const uint64_t pads = (uint64_t)s.pad_head + s.pad_tail;
        if (s.frames > most || pads > most - s.frames)
            return bad("frames: pad_head + frames + pad_tail" + at + " times out_channels overflows");
        T[k] = pads + s.frames;
    }
    return true;
}

bool edit_threshold(float threshold, std::string &err) {
    if (!(threshold >= 0.0f)) {
        err = "threshold must be at least 0 and not NaN";
        return false;
    }
    return true;
}

void edit_matrix_rows(const float *matrix, uint32_t in_channels, uint32_t out_channels, float (&rows)[kEditMaxMix * kEditMaxMix]) {
    for (uint32_t i = 0; i < kEditMaxMix * kEditMaxMix; i++) rows[i] = 0.0f;
    if (!matrix) return;
    for (uint32_t j = 0; j < out_channels; j++)
        for (uint32_t i = 0; i < in_channels; i++) rows[j * kEditMaxMix + i] = matrix[j * in_channels + i];
}

}  // namespace flo
