// conv_kernels.hpp — the launch of the FIR kernel (conv_kernels.hip) as convolve.cpp sees it.
#pragma once
#include <hip/hip_runtime.h>

#include "conv_plan.hpp"

namespace flo {

struct ConvArgs {
    float *dst = nullptr;                // output clip k at dst + jobs[k].dst_off; nothing else is written
    const ConvJob *jobs = nullptr;       // [n_out]
    const unsigned int *pre = nullptr;   // [n_out + 1] tiles in front of every output clip (clip_tiles)
    unsigned int n_out = 0, channels = 0;
};

// One workgroup per tile of the flat list (n_tiles = pre[n_out] > 0); ir_channels (1 or a.channels) is every job's; 0 or a
// hipError_t.
int launch_convolve(const ConvArgs &a, unsigned int n_tiles, unsigned int ir_channels, hipStream_t stream);

}  // namespace flo
