// resample_kernels.hip — sample-rate conversion of every clip of a batch in one launch (flo_batch_resample, flo_resample;
// resample.cpp). The filter, the index arithmetic and the geometry are resample_plan.hpp's.
//
// One workgroup per tile of the flat (clip, tile) list; it finds its clip by binary search over the per-clip prefix, as the
// batch analysis does. A tile is Q * L consecutive outputs from a multiple of L on: output q * L + r has the coefficient
// row p_r = (r * M) mod L whatever q is, and starts reading at staged frame q * M + floor(r * M / L). The workgroup stages
// the tile's input span once (zeros outside the clip); then every wave takes (r, 64 slots) units in turn: the phase is
// wave-uniform, so h[p_r][k] is a scalar operand from scalar loads, and the only LDS traffic is one read of x per lane and
// tap. A lane then makes kResampleBlock consecutive phases r, r + 1, ... of its slot in one pass: their windows start
// floor(M / L) or one more frame apart, so every x it reads feeds that many accumulators (and that many independent FMA
// chains). The lanes of a wave read M frames apart; resample_lds_index spreads an even M over the banks. Stereo keeps float2
// frames in LDS (one 8-byte read and two FMAs per tap); other channel counts keep planes of floats and go through the
// tile's LDS two channels at a time. Where 64 slots of input exceed the LDS budget (large M), a tile has fewer than 64
// slots and a wave takes several phases side by side (UNIFORM = false: the coefficients come through vector loads).
//
// Every output is sum_k fma(h[p][k], x[i + k - T/2 + 1], acc) for k = 0 .. T - 1 in that order, from acc = 0: the result of
// a clip does not depend on the batch around it, on where its tiles fall or on the kernel variant. Only outputs
// j < n_out of a clip are stored. Compiled with -ffp-contract=off; the FMAs are explicit.
#include <mutex>
#include <set>
#include <type_traits>
#include <utility>

#include "resample_kernels.hpp"

namespace flo {

typedef float rs_v2f __attribute__((ext_vector_type(2)));

extern __shared__ __attribute__((aligned(16))) char rs_smem[];

__device__ __forceinline__ float rs_fma(float h, float x, float acc) { return __builtin_fmaf(h, x, acc); }
__device__ __forceinline__ rs_v2f rs_fma(float h, rs_v2f x, rs_v2f acc) {
    const rs_v2f hh = {h, h};
    return __builtin_elementwise_fma(hh, x, acc);
}
__device__ __forceinline__ float rs_first(float v) { return v; }
__device__ __forceinline__ float rs_first(rs_v2f v) { return v.x; }
__device__ __forceinline__ float rs_second(float v) { return v; }
__device__ __forceinline__ float rs_second(rs_v2f v) { return v.y; }
// four stereo frames in a row: 32 bytes at the 8-byte alignment of a stereo frame
struct __attribute__((packed, aligned(8))) rs_run4 {
    float v[8];
};

template <bool STEREO, bool UNIFORM>
__global__ __launch_bounds__(kResampleThreads) void resample_kernel(const float *__restrict__ src_all, float *__restrict__ dst_all,
                                                                    const float *__restrict__ table, const ResampleArgs A) {
    typedef typename std::conditional<STEREO, rs_v2f, float>::type V;   // one staged frame of a plane
    const unsigned tid = threadIdx.x, lane = tid & 63u;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), n_waves = blockDim.x >> 6;
    // pre[lo] <= blockIdx.x < pre[lo + 1]: the last such lo, a clip that has tiles. This is tile_clip (clip_tiles.hpp) written
    // out: called as a function, its loop reaches this kernel already rotated and the compiler emits hi + lo for lo + hi;
    // written out, the code object is the one this kernel has always had
    const unsigned b = blockIdx.x;
    unsigned lo = 0, hi = A.n_clips;
    while (hi - lo > 1) {
        const unsigned mid = (lo + hi) >> 1;
        if (A.pre[mid] <= b) lo = mid;
        else hi = mid;
    }
    const unsigned tile = b - A.pre[lo];
    const unsigned long long n_in = A.n_in[lo], n_out = A.n_out[lo];
    const float *__restrict__ src = src_all + A.src_off[lo];
    float *__restrict__ dst = dst_all + A.dst_off[lo];
    const unsigned L = A.L, M = A.M, taps = A.taps, shift = A.shift, ch = A.channels;
    const unsigned long long j0 = (unsigned long long)tile * ((unsigned long long)A.slots * L);
    uint64_t i0;
    uint32_t p0;   // 0: j0 is a multiple of L
    resample_pos(j0, L, M, i0, p0);
    const long long start = (long long)i0 - (long long)(taps / 2 - 1);   // the clip's frame behind staged frame 0
    const unsigned stride = M + (M >> shift);   // LDS elements between the slots of neighbouring lanes
    const unsigned pass = STEREO ? 2u : (ch >= 2 ? 2u : 1u);

    for (unsigned c0 = 0; c0 < ch; c0 += pass) {
        const unsigned nc = ch - c0 < pass ? ch - c0 : pass;
        if (c0) __syncthreads();
        // (a tile belongs to a clip with outputs, so n_in >= 1.) Every load is unconditional at a clamped frame and zeroed
        // afterwards where the frame lies outside the clip: several loads of a thread are in flight at a time
        const unsigned long long last = n_in - 1;
        if (STEREO) {
            rs_v2f *x2 = reinterpret_cast<rs_v2f *>(rs_smem);
            const rs_v2f *s2 = reinterpret_cast<const rs_v2f *>(src);
#pragma unroll 8
            for (unsigned f = tid; f < A.span; f += kResampleThreads) {
                const long long sf = start + (long long)f;
                const bool in = sf >= 0 && (unsigned long long)sf <= last;
                const rs_v2f v = s2[sf < 0 ? 0ull : ((unsigned long long)sf > last ? last : (unsigned long long)sf)];
                x2[resample_lds_index(f, shift)] = in ? v : rs_v2f(0.f);
            }
        } else {
            float *x1 = reinterpret_cast<float *>(rs_smem);
#pragma unroll 8
            for (unsigned e = tid; e < A.span * nc; e += kResampleThreads) {
                const unsigned f = nc == 2 ? e >> 1 : e, c = nc == 2 ? e & 1u : 0u;
                const long long sf = start + (long long)f;
                const bool in = sf >= 0 && (unsigned long long)sf <= last;
                const float v = src[(sf < 0 ? 0ull : ((unsigned long long)sf > last ? last : (unsigned long long)sf)) * ch + c0 + c];
                x1[c * A.lds_elems + resample_lds_index(f, shift)] = in ? v : 0.f;
            }
        }
        __syncthreads();
        for (unsigned unit = wave; unit < A.units; unit += n_waves) {
            constexpr unsigned R = UNIFORM ? kResampleBlock : 1u;
            const ResampleLane ln = resample_lane(unit, lane, L, A.slots, A.lanes_per_phase, A.phases_per_wave, A.chunks, R);
            // idle lanes read inside the staged span and store nothing; with one phase per wave, r is lane 0's
            unsigned r0 = ln.r < L ? ln.r : L - 1;
            if (UNIFORM) r0 = (unsigned)__builtin_amdgcn_readfirstlane((int)r0);
            const unsigned q = ln.q < A.slots ? ln.q : A.slots - 1;
            const unsigned lanebase = q * stride;
            const unsigned long long j = j0 + (unsigned long long)q * L + r0;
            // outputs r0 .. r0 + R - 1 (as far as they stay below L; the rest repeats the last and is dropped): window starts
            // e[0] <= e[1] <= ..., less than a window apart, and coefficient rows
            unsigned e[R];
            const float *__restrict__ hrow[R];
#pragma unroll
            for (unsigned i = 0; i < R; i++) {
                const unsigned r = r0 + i < L ? r0 + i : L - 1;
                unsigned p;
                resample_phase(r, L, M, e[i], p);
                hrow[i] = table + (unsigned long long)p * taps;
            }
            for (unsigned c = 0; c < (STEREO ? 1u : nc); c++) {
                const V *x = reinterpret_cast<const V *>(rs_smem) + c * A.lds_elems + lanebase;
                V acc[R];
#pragma unroll
                for (unsigned i = 0; i < R; i++) acc[i] = V(0.f);
                unsigned o = e[0];
                if (R > 1) {   // before the last window starts: the outputs whose window has (uniform branches)
                    for (; o < e[R - 1]; o++) {
                        const V xv = x[o + (o >> shift)];
#pragma unroll
                        for (unsigned i = 0; i < R; i++)
                            if (o >= e[i]) acc[i] = rs_fma(hrow[i][o - e[i]], xv, acc[i]);
                    }
                }
                // every window holds o: one read of x, R FMAs, each output's taps in ascending order (counted from 0, so
                // that the coefficients of eight taps come in one scalar load per output)
                const unsigned n_all = e[0] + taps - o;
                const float *__restrict__ hp[R];
#pragma unroll
                for (unsigned i = 0; i < R; i++) hp[i] = hrow[i] + (o - e[i]);
#pragma unroll 8
                for (unsigned t = 0; t < n_all; t++) {
                    const unsigned oo = o + t;
                    const V xv = x[oo + (oo >> shift)];
#pragma unroll
                    for (unsigned i = 0; i < R; i++) acc[i] = rs_fma(hp[i][t], xv, acc[i]);
                }
                o += n_all;
                if (R > 1) {   // behind the first window's end
                    for (; o < e[R - 1] + taps; o++) {
                        const V xv = x[o + (o >> shift)];
#pragma unroll
                        for (unsigned i = 0; i < R; i++)
                            if (o >= e[i] && o - e[i] < taps) acc[i] = rs_fma(hrow[i][o - e[i]], xv, acc[i]);
                    }
                }
                // a lane's R outputs are neighbours in the clip: one store of the run where all of them exist
                if (STEREO && R == 4 && ln.active && r0 + R <= L && j + R <= n_out) {
                    rs_run4 run;
#pragma unroll
                    for (unsigned i = 0; i < R; i++) run.v[2 * i] = rs_first(acc[i]), run.v[2 * i + 1] = rs_second(acc[i]);
                    *reinterpret_cast<rs_run4 *>(dst + 2 * j) = run;
                } else {
#pragma unroll
                    for (unsigned i = 0; i < R; i++) {
                        if (ln.active && r0 + i < L && j + i < n_out) {
                            if (STEREO) reinterpret_cast<V *>(dst)[j + i] = acc[i];
                            else dst[(j + i) * ch + c0 + c] = rs_first(acc[i]);
                        }
                    }
                }
            }
        }
    }
}

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-device property of a kernel: set once per (device, kernel) under a
// lock, from whichever thread launches first on that device
static int rs_allow_lds(const void *fn) {
    static std::mutex mu;
    static std::set<std::pair<int, const void *>> done;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return (int)e;
    std::lock_guard<std::mutex> g(mu);
    if (done.count({dev, fn})) return 0;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kResampleLdsBytes);
    if (e != hipSuccess) return (int)e;
    done.insert({dev, fn});
    return 0;
}

template <bool STEREO, bool UNIFORM>
static int rs_launch(const ResampleArgs &a, unsigned n_tiles, unsigned lds_bytes, hipStream_t stream) {
    if (int rc = rs_allow_lds(reinterpret_cast<const void *>(&resample_kernel<STEREO, UNIFORM>))) return rc;
    resample_kernel<STEREO, UNIFORM><<<dim3(n_tiles), dim3(kResampleThreads), lds_bytes, stream>>>(a.src, a.dst, a.table, a);
    return (int)hipGetLastError();
}

int launch_resample(const ResampleArgs &a, unsigned int n_tiles, unsigned int lds_bytes, hipStream_t stream) {
    if (!n_tiles) return 0;
    if (lds_bytes > kResampleLdsBytes) return (int)hipErrorInvalidValue;
    const bool uniform = a.phases_per_wave == 1;
    if (a.channels == 2) return uniform ? rs_launch<true, true>(a, n_tiles, lds_bytes, stream) : rs_launch<true, false>(a, n_tiles, lds_bytes, stream);
    return uniform ? rs_launch<false, true>(a, n_tiles, lds_bytes, stream) : rs_launch<false, false>(a, n_tiles, lds_bytes, stream);
}

}  // namespace flo
