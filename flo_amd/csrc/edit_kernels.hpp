// edit_kernels.hpp — the launches of the editing kernels (edit_kernels.hip) as edit.cpp sees them.
#pragma once
#include <hip/hip_runtime.h>

#include "edit_plan.hpp"

namespace flo {

// which instantiation of edit_kernel makes a launch
enum EditForm : int { kEditCopy = 0, kEditTwoToOne = 1, kEditOneToTwo = 2, kEditGeneric = 3 };

struct EditArgs {
    const float *src = nullptr;   // interleaved f32: segment k's source clip at src + segs[k].src_off
    float *dst = nullptr;         // output clip k at dst + segs[k].dst_off; nothing else is written
    const EditSeg *segs = nullptr;       // [n_segs]
    const unsigned int *pre = nullptr;   // [n_segs + 1] tiles in front of every output clip (clip_tiles)
    unsigned int n_segs = 0, cin = 0, cout = 0;
    float m[kEditMaxMix * kEditMaxMix] = {};   // rows of kEditMaxMix (edit_matrix_rows); unused by the copy form
};

struct EditActiveArgs {
    const float *src = nullptr;
    const unsigned long long *src_off = nullptr, *frames = nullptr;   // [n_clips]
    const unsigned int *pre = nullptr;                                // [n_clips + 1] tiles of edit_tile_frames(channels)
    unsigned long long *first = nullptr;   // [n_clips] the smallest active frame, from ~0
    unsigned long long *end = nullptr;     // [n_clips] the largest active frame plus one, from 0
    unsigned int n_clips = 0, channels = 0;
    float threshold = 0;
};

// Each: one workgroup per tile of the flat list (n_tiles = pre[n] > 0); 0 or a hipError_t.
int launch_edit(const EditArgs &a, EditForm form, unsigned int n_tiles, hipStream_t stream);
int launch_edit_active(const EditActiveArgs &a, unsigned int n_tiles, hipStream_t stream);

}  // namespace flo
