// fftconv_plan.cpp — see fftconv_plan.hpp.
#include "fftconv_plan.hpp"

#include <algorithm>
#include <cmath>
#include <map>
#include <tuple>

#include "clip_tiles.hpp"

namespace flo {

namespace {
constexpr int64_t kB = kFcBlock, kLB = kFcLaneBlocks;
// ceil(a / B) of a signed a
int64_t ceil_blocks(int64_t a) { return a >= 0 ? (a + kB - 1) / kB : -((-a) / kB); }
}  // namespace

bool fftconv_plan(const ConvSource &src, const ConvSource &irs, size_t n_out, const flo_conv_job *jobs, uint64_t group_bytes, FcPlan &plan,
                  std::string &err) {
    plan = FcPlan();
    std::vector<uint32_t> K, pre;
    ConvLimits lim;
    lim.max_taps = FLO_CONV_FFT_MAX_TAPS;
    lim.max_taps_name = "FLO_CONV_FFT_MAX_TAPS";
    lim.tile_frames = kFcTileFrames;
    if (!conv_check(src, irs, n_out, jobs, K, pre, err, lim)) return false;
    const uint32_t C = src.channels, Ch = irs.channels;
    plan.channels = C;
    plan.ir_channels = Ch;
    // (a group's items stay far below 2^32 whatever the caller asks for)
    const uint64_t seg_bytes = fftconv_segment_elems(C) * 8;
    uint64_t cap_segs = std::min<uint64_t>(group_bytes, (uint64_t)1 << 38) / seg_bytes;

    std::map<std::tuple<uint32_t, uint64_t, uint32_t>, uint32_t> seen;
    plan.jobs.resize(n_out);
    for (size_t k = 0; k < n_out; k++) {
        const flo_conv_job &g = jobs[k];
        FcJob &j = plan.jobs[k];
        j.taps = K[k];
        j.parts = fftconv_parts(K[k]);
        // one response per distinct (ir, ir_start, K); every K == 0 is the same empty one
        const auto key = K[k] ? std::make_tuple(g.ir, g.ir_start, K[k]) : std::make_tuple(0u, (uint64_t)0, 0u);
        auto it = seen.find(key);
        if (it == seen.end()) {
            FcResponse r;
            r.ir = std::get<0>(key);
            r.ir_start = std::get<1>(key);
            r.taps = K[k];
            r.parts = j.parts;
            r.h_off = plan.h_elems;
            plan.h_elems += (uint64_t)r.parts * Ch * kFcBlock;
            it = seen.emplace(key, (uint32_t)plan.responses.size()).first;
            plan.responses.push_back(r);
        }
        j.response = it->second;
        const uint64_t N = src.clip_frames[g.clip];
        j.skip = conv_skip(g.skip, N, K[k]);
        j.blocks = g.frames / kFcBlock + (g.frames % kFcBlock != 0);
        if (N && K[k] && j.blocks) {
            // segment q meets the clip where (q + 1)B + skip > 0 and (q - 1)B + skip < N; a block uses q in [b - Pn + 1, b]
            const int64_t lo = -ceil_blocks((int64_t)j.skip), hi = ceil_blocks((int64_t)N - (int64_t)j.skip) + 1;
            j.q_lo = std::max<int64_t>(lo, -(int64_t)(j.parts - 1));
            j.q_hi = std::min<int64_t>(hi, (int64_t)j.blocks);
            if (j.q_hi <= j.q_lo) j.q_lo = j.q_hi = 0;
        }
    }

    // a cap far too small for the call is raised until about kFcMaxGroups groups hold its segments: a bad value in the
    // environment must not turn one call into millions of launches
    uint64_t all_segs = 0;
    for (const FcJob &j : plan.jobs) all_segs += (uint64_t)(j.q_hi - j.q_lo);
    cap_segs = std::max(cap_segs, all_segs / kFcMaxGroups + (all_segs % kFcMaxGroups != 0));
    // groups: jobs in order, each cut at tile boundaries where the cap asks for it
    FcGroup cur;
    uint64_t cur_segs = 0;
    auto close = [&] {
        cur.count = plan.entries.size() - cur.first;
        cur.x_elems = cur_segs * fftconv_segment_elems(C);
        plan.x_elems = std::max(plan.x_elems, cur.x_elems);
        plan.groups.push_back(cur);
        cur = FcGroup();
        cur.first = plan.entries.size();
        cur_segs = 0;
    };
    for (size_t k = 0; k < n_out; k++) {
        const FcJob &j = plan.jobs[k];
        uint64_t b0 = 0;
        while (b0 < j.blocks) {
            const int64_t s0 = std::max<int64_t>(j.q_lo, (int64_t)b0 - (int64_t)j.parts + 1);
            const uint64_t room = cap_segs > cur_segs ? cap_segs - cur_segs : 0;
            // the last block b1 with min(q_hi, b1) - s0 <= room
            uint64_t b1 = j.blocks;
            if (j.q_hi > s0 && (uint64_t)(j.q_hi - s0) > room) {
                const int64_t end = s0 + (int64_t)room;   // < q_hi <= blocks
                b1 = end <= (int64_t)b0 ? b0 : (uint64_t)end / kLB * kLB;
                if (b1 <= b0) {
                    if (plan.entries.size() > cur.first) {   // a fresh group has more room
                        close();
                        continue;
                    }
                    b1 = std::min<uint64_t>(b0 + kLB, j.blocks);   // one tile, whatever the cap
                }
            }
            FcEntry e;
            e.job = (uint32_t)k;
            e.b0 = b0;
            e.b1 = b1;
            e.s0 = s0;
            e.s1 = std::max<int64_t>(s0, std::min<int64_t>(j.q_hi, (int64_t)b1));
            if (j.q_hi <= j.q_lo) e.s0 = e.s1 = 0;
            e.x_off = cur_segs * fftconv_segment_elems(C);
            cur_segs += (uint64_t)(e.s1 - e.s0);
            plan.entries.push_back(e);
            b0 = b1;
        }
    }
    if (plan.entries.size() > cur.first) close();
    // every group's lists must fit a launch
    std::vector<uint32_t> a, b;
    for (const FcGroup &g : plan.groups)
        if (!fftconv_group_tiles(plan, g, a, b)) {
            err = "too many tiles for one launch";
            return false;
        }
    if (!fftconv_response_tiles(plan, a)) {
        err = "too many tiles for one launch";
        return false;
    }
    return true;
}

bool fftconv_group_tiles(const FcPlan &plan, const FcGroup &g, std::vector<uint32_t> &pre_spec, std::vector<uint32_t> &pre_mac) {
    std::vector<uint64_t> items(g.count), blocks(g.count);
    for (size_t i = 0; i < g.count; i++) {
        const FcEntry &e = plan.entries[g.first + i];
        items[i] = (uint64_t)(e.s1 - e.s0) * plan.channels;
        blocks[i] = e.b1 - e.b0;
        if (items[i] > 0xFFFFFFFFull) return false;
    }
    return clip_tiles(items.data(), g.count, kFcTogether, pre_spec) && clip_tiles(blocks.data(), g.count, kFcLaneBlocks, pre_mac);
}

bool fftconv_response_tiles(const FcPlan &plan, std::vector<uint32_t> &pre) {
    std::vector<uint64_t> items(plan.responses.size());
    for (size_t i = 0; i < items.size(); i++) items[i] = (uint64_t)plan.responses[i].parts * plan.ir_channels;
    return clip_tiles(items.data(), items.size(), kFcTogether, pre);
}

void fftconv_twiddles(std::vector<float> &tw) {
    tw.resize(2 * (size_t)kFcBlock);
    const double pi = 3.14159265358979323846264338327950288;
    for (uint32_t k = 0; k < kFcBlock; k++) {
        const double a = pi * (double)k / (double)kFcBlock;   // 2 pi k / F
        tw[2 * k] = (float)std::cos(a);
        tw[2 * k + 1] = (float)-std::sin(a);
    }
}

extern "C" int flo_conv_fft_geometry(uint8_t channels, uint8_t ir_channels, flo_conv_fft_info *info) {
    if (!info || channels < 1 || channels > kConvMaxChannels || (ir_channels != 1 && ir_channels != channels)) return FLO_ERR_ARG;
    *info = flo_conv_fft_info{kFcBlock, kFcLaneBlocks, FLO_CONV_FFT_MAX_TAPS, kFcCrossoverTaps};
    return FLO_OK;
}

}  // namespace flo
