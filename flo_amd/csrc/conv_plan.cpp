// conv_plan.cpp — see conv_plan.hpp.
#include "conv_plan.hpp"

#include "clip_tiles.hpp"

namespace flo {

bool conv_check(const ConvSource &src, const ConvSource &irs, size_t n_out, const flo_conv_job *jobs, std::vector<uint32_t> &K,
                std::vector<uint32_t> &pre, std::string &err, const ConvLimits &lim) {
    auto bad = [&](const std::string &m) {
        err = m;
        return false;
    };
    if (!src.present) return bad("src is NULL");
    if (!irs.present) return bad("irs is NULL");
    if (irs.ctx != src.ctx) return bad("context of irs is not the context of src");
    if (irs.rate != src.rate)
        return bad("sample_rate " + std::to_string(irs.rate) + " of irs differs from the " + std::to_string(src.rate) + " of src: resample one of them first");
    const uint32_t ch = src.channels;
    if (ch < 1 || ch > kConvMaxChannels) return bad("channels " + std::to_string(ch) + " of src are outside 1 .. " + std::to_string(kConvMaxChannels));
    if (irs.channels != 1 && irs.channels != ch)
        return bad("ir_channels " + std::to_string(irs.channels) + " of irs are neither 1 nor the " + std::to_string(ch) + " of src");
    if (n_out && !jobs) return bad("jobs is NULL");
    const uint64_t most = (uint64_t)(SIZE_MAX / 8) / ch;   // what flo_batch_create lays out without overflow
    K.assign(n_out, 0);
    std::vector<uint64_t> T(n_out);
    for (size_t k = 0; k < n_out; k++) {
        const flo_conv_job &j = jobs[k];
        const std::string of = " of job " + std::to_string(k);
        if (j.clip >= src.n_clips) return bad("clip " + std::to_string(j.clip) + of + " is not below n_clips " + std::to_string(src.n_clips) + " of src");
        if (j.ir >= irs.n_clips) return bad("ir " + std::to_string(j.ir) + of + " is not below n_clips " + std::to_string(irs.n_clips) + " of irs");
        if (j.reserved != 0) return bad("reserved" + of + " is not 0");
        K[k] = conv_taps(j.taps, irs.clip_frames[j.ir], j.ir_start);
        if (K[k] > lim.max_taps)
            return bad("taps" + of + ": " + std::to_string(K[k]) + " taps are above " + lim.max_taps_name + " " + std::to_string(lim.max_taps));
        if (j.frames + j.skip < j.frames) return bad("frames + skip" + of + " wraps 64 bits");
        if (j.frames > most) return bad("frames " + std::to_string(j.frames) + of + " times channels overflows");
        T[k] = j.frames;
    }
    if (!clip_tiles(T.data(), n_out, lim.tile_frames, pre)) return bad("too many tiles for one launch");
    return true;
}

extern "C" int flo_conv_geometry(uint8_t channels, uint8_t ir_channels, flo_conv_info *info) {
    if (!info || channels < 1 || channels > kConvMaxChannels || (ir_channels != 1 && ir_channels != channels)) return FLO_ERR_ARG;
    // (the stereo variant and the plane variant share one geometry)
    *info = flo_conv_info{kConvTileFrames, kConvTapChunk, kConvLaneOutputs};
    return FLO_OK;
}

}  // namespace flo
