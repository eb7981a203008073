// mix_kernels.hpp — the launch of the mixing kernel (mix_kernels.hip) as mix.cpp sees it.
#pragma once
#include <hip/hip_runtime.h>

#include "mix_plan.hpp"

namespace flo {

struct MixArgs {
    float *dst = nullptr;                 // output clip k at dst + clips[k].dst_off; nothing else is written
    const MixPart *parts = nullptr;       // [ppre[n_out]] in list order
    const MixClip *clips = nullptr;       // [n_out]
    const unsigned int *ppre = nullptr;   // [n_out + 1] parts in front of every output clip
    const unsigned int *pre = nullptr;    // [n_out + 1] tiles in front of every output clip (clip_tiles)
    unsigned int n_out = 0, channels = 0;
};

// One workgroup per tile of the flat list (n_tiles = pre[n_out] > 0); 0 or a hipError_t.
int launch_mix(const MixArgs &a, unsigned int n_tiles, hipStream_t stream);

}  // namespace flo
