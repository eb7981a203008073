// mix_plan.cpp — see mix_plan.hpp.
#include "mix_plan.hpp"

#include <cmath>

#include "clip_tiles.hpp"

namespace flo {

bool mix_check(const MixSource *srcs, size_t n_srcs, size_t n_out, const uint64_t *out_frames, size_t n_parts, const flo_mix_part *parts,
               std::vector<uint32_t> &ppre, std::vector<uint32_t> &pre, std::string &err) {
    auto bad = [&](const std::string &m) {
        err = m;
        return false;
    };
    if (!n_srcs || !srcs) return bad("n_srcs is 0: a mix needs at least one source batch");
    for (size_t i = 0; i < n_srcs; i++) {
        const std::string of = " of source " + std::to_string(i);
        if (!srcs[i].present) return bad("source " + std::to_string(i) + " is NULL");
        if (srcs[i].ctx != srcs[0].ctx) return bad("context" + of + " is not the context of source 0");
        if (srcs[i].rate != srcs[0].rate)
            return bad("sample_rate " + std::to_string(srcs[i].rate) + of + " differs from the " + std::to_string(srcs[0].rate) + " of source 0");
        if (srcs[i].channels != srcs[0].channels)
            return bad("channels " + std::to_string(srcs[i].channels) + of + " differ from the " + std::to_string(srcs[0].channels) + " of source 0");
    }
    const uint32_t ch = srcs[0].channels;
    if (ch < 1) return bad("channels must be at least 1");
    if (n_out && !out_frames) return bad("out_frames is NULL");
    if (n_parts && !parts) return bad("parts is NULL");
    if ((uint64_t)n_parts >= (1ull << 32)) return bad("n_parts " + std::to_string(n_parts) + " is not below 2^32");
    const uint64_t most = (uint64_t)(SIZE_MAX / 8) / ch;   // what flo_batch_create lays out without overflow
    for (size_t k = 0; k < n_out; k++)
        if (out_frames[k] > most) return bad("out_frames " + std::to_string(out_frames[k]) + " of output " + std::to_string(k) + " times channels overflows");
    if (!clip_tiles(out_frames, n_out, edit_tile_frames(ch), pre)) return bad("too many tiles for one launch");
    ppre.assign(n_out + 1, 0);
    uint32_t last = 0;
    for (size_t i = 0; i < n_parts; i++) {
        const flo_mix_part &p = parts[i];
        const std::string of = " of part " + std::to_string(i);
        if (p.out >= n_out) return bad("out " + std::to_string(p.out) + of + " is not below n_out " + std::to_string(n_out));
        if (p.out < last) return bad("out " + std::to_string(p.out) + of + " is below the " + std::to_string(last) + " of the part before it: out must not decrease");
        last = p.out;
        if (p.batch >= n_srcs) return bad("batch " + std::to_string(p.batch) + of + " is not below n_srcs " + std::to_string(n_srcs));
        if (p.clip >= srcs[p.batch].n_clips)
            return bad("clip " + std::to_string(p.clip) + of + " is not below n_clips " + std::to_string(srcs[p.batch].n_clips) + " of source " + std::to_string(p.batch));
        if (p.fade_in >= kEditMaxFade || p.fade_in > p.frames)
            return bad("fade_in " + std::to_string(p.fade_in) + of + " is longer than its " + std::to_string(p.frames) + " frames or not below 2^24");
        if (p.fade_out >= kEditMaxFade || p.fade_out > p.frames)
            return bad("fade_out " + std::to_string(p.fade_out) + of + " is longer than its " + std::to_string(p.frames) + " frames or not below 2^24");
        if (!std::isfinite(p.gain)) return bad("gain" + of + " is not finite");
        if (p.at + p.frames < p.at) return bad("at + frames" + of + " wraps 64 bits");
        if (p.start + p.frames < p.start) return bad("start + frames" + of + " wraps 64 bits");
        ppre[p.out + 1]++;
    }
    for (size_t k = 0; k < n_out; k++) ppre[k + 1] += ppre[k];
    return true;
}

}  // namespace flo
