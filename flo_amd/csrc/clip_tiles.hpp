// clip_tiles.hpp — what every batch-to-batch operation shares (resample, normalize, edit; the batched analysis uses the
// lookup): each clip is cut into tiles, the flat list of tiles is one launch, a workgroup finds its clip by binary search
// in the per-clip prefix, and the lists go up in one block. Header-only plain C++: the plan files and their host tests
// build it with g++ alone, the host files and the kernels with hipcc.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define FLO_CT_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define FLO_CT_HD inline __attribute__((always_inline))
#endif

namespace flo {

// The flat work list: pre[i] = tiles of clips 0 .. i - 1, clip i of count[i] items cut into tiles of per_tile (pre has
// n + 1 entries); false when a launch cannot hold them: more than 2^31 - 1 clips or tiles.
inline bool clip_tiles(const uint64_t *count, size_t n, uint64_t per_tile, std::vector<uint32_t> &pre) {
    if (n > 0x7FFFFFFFull) return false;
    pre.assign(n + 1, 0);
    uint64_t t = 0;
    for (size_t i = 0; i < n; i++) {
        pre[i] = (uint32_t)t;
        const uint64_t tiles = count[i] / per_tile + (count[i] % per_tile != 0);   // (count + per_tile - 1 can wrap)
        if (tiles > 0x7FFFFFFFull - t) return false;
        t += tiles;
    }
    pre[n] = (uint32_t)t;
    return true;
}

// pre[lo] <= b < pre[lo + 1]: the last such lo, a clip that has tiles (0 <= b < pre[n])
FLO_CT_HD unsigned tile_clip(const unsigned *pre, unsigned n, unsigned b) {
    unsigned lo = 0, hi = n;
    while (hi - lo > 1) {
        const unsigned mid = (lo + hi) >> 1;
        if (pre[mid] <= b) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Offsets of the regions of one block, each 16-byte aligned, in the order they are taken. It describes the block only: the
// memory (pinned, pageable or device) is the caller's, and the same offsets address the host copy and the device copy.
struct BlockLayout {
    size_t bytes = 0;
    size_t take(size_t b) {
        const size_t at = bytes;
        bytes += (b + 15) & ~(size_t)15;
        return at;
    }
    template <class T>
    static T *at(void *base, size_t off) {
        return reinterpret_cast<T *>(static_cast<char *>(base) + off);
    }
};

}  // namespace flo
