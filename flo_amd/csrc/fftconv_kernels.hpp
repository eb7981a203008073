// fftconv_kernels.hpp — the launches of the partitioned FFT convolution (fftconv_kernels.hip) as fftconv.cpp sees them.
#pragma once
#include <hip/hip_runtime.h>

#include "fftconv_plan.hpp"

namespace flo {

// Spectra of the transforms of a list of signals (responses: profile name fftconv_ir; segments: fftconv_fwd)
struct FcSpecArgs {
    float2 *out = nullptr;               // every job's `out` counts complex elements from here
    const FcSpecJob *jobs = nullptr;     // [n_jobs]
    const unsigned int *pre = nullptr;   // [n_jobs + 1] tiles of kFcTogether items in front of every job (clip_tiles)
    const float2 *tw = nullptr;          // [kFcBlock] fftconv_twiddles
    unsigned int n_jobs = 0;
};
// The multiply stage and the inverse transform (fftconv_mac)
struct FcMacArgs {
    float *dst = nullptr;                // entry e's output clip at dst + jobs[e].dst_off; nothing else is written
    const float2 *x = nullptr, *h = nullptr;   // segment and response spectra
    const float2 *tw = nullptr;
    const FcMacJob *jobs = nullptr;      // [n_jobs]
    const unsigned int *pre = nullptr;   // [n_jobs + 1] tiles of kFcLaneBlocks blocks in front of every entry
    unsigned int n_jobs = 0, channels = 0;
};

// One workgroup per tile of the flat list (n_tiles = pre[n_jobs] > 0; the multiply stage: times channels); 0 or a hipError_t.
int launch_fftconv_spectra(const FcSpecArgs &a, unsigned int n_tiles, hipStream_t stream);
int launch_fftconv_mac(const FcMacArgs &a, unsigned int n_tiles, hipStream_t stream);

}  // namespace flo
