// resample_kernels.hpp — the launch of the sample-rate conversion kernel (resample_kernels.hip) as resample.cpp sees it.
#pragma once
#include <hip/hip_runtime.h>

#include "resample_plan.hpp"

namespace flo {

struct ResampleArgs {
    const float *src = nullptr;   // interleaved f32: clip i's n_in[i] frames at src + src_off[i]
    float *dst = nullptr;         // clip i's n_out[i] frames at dst + dst_off[i]; nothing else is written
    const float *table = nullptr; // [L][taps]
    const unsigned long long *src_off = nullptr, *n_in = nullptr, *dst_off = nullptr, *n_out = nullptr;   // [n_clips]
    const unsigned int *pre = nullptr;   // [n_clips + 1] tiles in front of every clip (clip_tiles)
    unsigned int n_clips = 0, channels = 0;
    // ResamplePlan's fields (the plan's block is the kernel's own: kResampleBlock with one phase per wave, else 1)
    unsigned int L = 0, M = 0, taps = 0, slots = 0, lanes_per_phase = 0, phases_per_wave = 0, chunks = 0, units = 0;
    unsigned int shift = 31, span = 0, lds_elems = 0;
};

// one workgroup per tile of the flat list (n_tiles = pre[n_clips] > 0); 0 or a hipError_t
int launch_resample(const ResampleArgs &a, unsigned int n_tiles, unsigned int lds_bytes, hipStream_t stream);

}  // namespace flo
