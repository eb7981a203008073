// mix_kernels.hip — sums of parts of the clips of resident batches, each at a gain and with linear fades (flo_batch_mix,
// flo_mix; mix.cpp). The definition and the class of a part on a tile are mix_plan.hpp's, the tile geometry the edit stage's.
//
// One workgroup per tile of the flat (output clip, tile) list; it finds its clip by binary search over the per-clip prefix,
// as the sample-rate conversion, the normalisation and the edit stage do. A lane owns the same 16 floats of the tile in
// every path: four 16-byte units, unit = tid + 256 j, accumulated in registers from +0.0 and written once at the end, so
// every output float is stored exactly once and a tile without a live part stores zeros.
//
// Each wave scans its clip's parts 64 at a time: a lane reads one part's placement and asks the plan's own function
// whether the part is live on the tile, the ballot's bits are walked lowest first (list order is summation order), the
// part's index is made uniform, so the part itself comes through scalar loads and the branch on its class is wave-uniform.
// The four waves scan redundantly: no LDS, no barrier. The scan is linear in the clip's parts.
//
// A whole part (live on every frame of the tile, none in a fade) is four 16-byte loads per lane at the 4-byte aligned
// source address and sixteen FMAs with the scalar gain; any other part, and any part on a last tile whose floats do not
// fill whole 16-byte units, goes float by float with every check of the definition. mx_coef holds a copy of the edit
// stage's fade-weight arithmetic (ed_weight, edit_kernels.hip).
// Compiled with -ffp-contract=off; the FMAs are explicit, the products single multiplications, the divisions IEEE.
#include "clip_tiles.hpp"
#include "mix_kernels.hpp"

namespace flo {

typedef float mx_v4f __attribute__((ext_vector_type(4)));
typedef const float __attribute__((address_space(1))) mx_gf;   // a part's pointer arrives through memory: say that it is global

// k_p of frame u of the part: gain where no fade applies, else fl32(gain * w)
__device__ __forceinline__ float mx_coef(unsigned long long u, const MixPart &p) {
    const unsigned long long v = p.frames - 1 - u;
    const bool in = u < p.fade_in, out = v < p.fade_out;
    if (!in && !out) return p.gain;
    const float w_in = in ? __fdiv_rn((float)(unsigned)u, (float)p.fade_in) : 0.f;
    const float w_out = out ? __fdiv_rn((float)(unsigned)v, (float)p.fade_out) : 0.f;
    const float w = in && out ? w_in * w_out : in ? w_in : w_out;
    return p.gain * w;
}

// a whole part on a tile of whole units (n a multiple of 4: a unit is full or has no float of the tile): the tile's n floats
// lie at sp (4-byte aligned) one after another. The four loads are issued before the first FMA; the accumulators of a unit
// without a float are never stored, so what the FMAs make of them does not matter
__device__ __forceinline__ void mx_whole(const mx_gf *__restrict__ sp, float g, unsigned n, unsigned tid, float (&acc)[16]) {
    mx_v4f v[4];
#pragma unroll
    for (unsigned j = 0; j < 4; j++) {
        const unsigned i = 4 * (tid + kMixThreads * j);
        v[j] = mx_v4f{0.f, 0.f, 0.f, 0.f};
        if (i < n) __builtin_memcpy(&v[j], sp + i, 16);   // one 16-byte load at a 4-byte aligned address
    }
#pragma unroll
    for (unsigned j = 0; j < 4; j++)
#pragma unroll
        for (unsigned e = 0; e < 4; e++) acc[4 * j + e] = __builtin_fmaf(g, v[j][e], acc[4 * j + e]);
}

// any part: the lane's sixteen floats one by one
__device__ __forceinline__ void mx_partial(const MixPart &p, unsigned long long t0, unsigned n, unsigned ch, unsigned tid, float (&acc)[16]) {
    const unsigned long long avail = mix_avail(p);
    const mx_gf *__restrict__ src = (const mx_gf *)p.src;
#pragma unroll
    for (unsigned j = 0; j < 4; j++) {
        const unsigned i = 4 * (tid + kMixThreads * j);
        unsigned f = i / ch, c = i - f * ch;
#pragma unroll
        for (unsigned e = 0; e < 4; e++) {
            const unsigned long long t = t0 + f;
            if (i + e < n && t >= p.at && t - p.at < avail) {
                const unsigned long long u = t - p.at;
                acc[4 * j + e] = __builtin_fmaf(mx_coef(u, p), src[(p.start + u) * ch + c], acc[4 * j + e]);
            }
            if (++c == ch) {
                c = 0;
                f++;
            }
        }
    }
}

__global__ __launch_bounds__(kMixThreads) void mix_kernel(const MixArgs A) {
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    const unsigned k = tile_clip(A.pre, A.n_out, blockIdx.x);
    const unsigned tile = blockIdx.x - A.pre[k];
    const MixClip *__restrict__ clips = A.clips;
    const MixPart *__restrict__ parts = A.parts;
    const MixClip oc = clips[k];
    const unsigned ch = A.channels, F = edit_tile_frames(ch);
    const unsigned long long T = oc.frames, t0 = (unsigned long long)tile * F;
    const unsigned nf = T - t0 < F ? (unsigned)(T - t0) : F, n = nf * ch;
    const unsigned long long p0 = A.ppre[k], p1 = A.ppre[k + 1];
    float acc[16];
#pragma unroll
    for (unsigned i = 0; i < 16; i++) acc[i] = 0.f;
    for (unsigned long long base = p0; base < p1; base += 64) {
        const unsigned long long idx = base + lane;
        bool live = false;
        if (idx < p1) live = mix_part_in_tile(parts[idx], T, t0, nf) != kMixNone;
        unsigned long long mask = __ballot(live);
        while (mask) {
            const unsigned bit = (unsigned)__builtin_ctzll(mask);
            mask &= mask - 1;
            const unsigned pi = __builtin_amdgcn_readfirstlane((unsigned)(base + bit));
            const MixPart p = parts[pi];
            // (a whole part on a last tile whose floats do not fill whole units goes float by float as well)
            if (mix_part_in_tile(p, T, t0, nf) == kMixWhole && (n & 3u) == 0)
                mx_whole((const mx_gf *)p.src + (p.start + (t0 - p.at)) * ch, p.gain, n, tid, acc);
            else mx_partial(p, t0, n, ch, tid, acc);
        }
    }
    float *__restrict__ dp = A.dst + oc.dst_off + t0 * ch;   // 16-byte aligned: the clip is, and so are F * ch floats
#pragma unroll
    for (unsigned j = 0; j < 4; j++) {
        const unsigned i = 4 * (tid + kMixThreads * j);
        if (i + 4 <= n) {
            *reinterpret_cast<mx_v4f *>(dp + i) = mx_v4f{acc[4 * j], acc[4 * j + 1], acc[4 * j + 2], acc[4 * j + 3]};
        } else {
#pragma unroll
            for (unsigned e = 0; e < 4; e++)
                if (i + e < n) dp[i + e] = acc[4 * j + e];
        }
    }
}

int launch_mix(const MixArgs &a, unsigned int n_tiles, hipStream_t stream) {
    if (!n_tiles) return 0;
    mix_kernel<<<dim3(n_tiles), dim3(kMixThreads), 0, stream>>>(a);
    return (int)hipGetLastError();
}

}  // namespace flo
