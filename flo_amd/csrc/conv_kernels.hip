// conv_kernels.hip — direct-form FIR of the clips of a resident batch by the clips of another (flo_batch_convolve,
// flo_convolve; convolve.cpp). The definition, the geometry and the LDS index are conv_plan.hpp's.
//
// One workgroup per tile of the flat (output clip, tile) list; it finds its clip by binary search over the per-clip prefix,
// as the other batch-to-batch stages do. A tile is kConvTileFrames output frames; a lane owns kConvLaneOutputs (LO)
// consecutive ones, whose accumulators stay in registers from +0.0 to the single store.
//
// Taps are taken in chunks of kConvTapChunk (KC), chunks and the taps inside them in ascending k, so every output's chain is
// the definition's whatever the chunking. For the chunk from tap k0 on the workgroup stages the source frames it touches:
// staged frame s is source frame t0 + skip - k0 - (KC - 1) + s, s < kConvTileFrames + KC - 1, +0.0 where that lies outside
// [0, N); every load is unconditional at a clamped frame (none at all for a clip of no frames). Output j of a lane meets tap
// k0 + kk at staged frame lane * LO + j + KC - 1 - kk. The lane keeps a window of LO staged frames in registers: each tap
// costs one LDS read (the frame that enters the window) and LO FMAs. The tap loop is unrolled by LO, so the window is a ring
// that rotates by name. The tap is wave-uniform and comes through scalar loads from the response clip in global memory.
// Lanes read LO frames apart; conv_lds_index skews that to 9 elements, odd in banks.
//
// Stereo keeps float2 frames (one 8-byte read and LO packed FMAs per tap, the tap pair either (h, h) or the response's two
// channels); every other channel count goes through the tile one channel at a time as a plane of floats. Stores are 16-byte
// units where a lane's frames all exist and its floats are contiguous (stereo, mono); float by float on a clip's ragged last
// tile and for the planes of three and more channels.
// Compiled with -ffp-contract=off; the FMAs are explicit.
#include <type_traits>

#include "clip_tiles.hpp"
#include "conv_kernels.hpp"

namespace flo {

typedef float cv_v2f __attribute__((ext_vector_type(2)));
typedef float cv_v4f __attribute__((ext_vector_type(4)));
typedef const float __attribute__((address_space(1))) cv_gf;      // a job's pointers arrive through memory: say that they are global
typedef const cv_v2f __attribute__((address_space(1))) cv_g2f;

constexpr unsigned kCvLO = kConvLaneOutputs, kCvKC = kConvTapChunk;
static_assert(kCvLO == 8 && kCvKC % kCvLO == 0, "the ring below is written for a window of 8");

__device__ __forceinline__ float cv_fma(float h, float x, float a) { return __builtin_fmaf(h, x, a); }
__device__ __forceinline__ cv_v2f cv_fma(cv_v2f h, cv_v2f x, cv_v2f a) { return __builtin_elementwise_fma(h, x, a); }
__device__ __forceinline__ float cv_first(float v) { return v; }
__device__ __forceinline__ float cv_first(cv_v2f v) { return v.x; }
__device__ __forceinline__ float cv_second(float v) { return v; }
__device__ __forceinline__ float cv_second(cv_v2f v) { return v.y; }

// tap k (uniform) as a frame's worth of coefficients. Planes: element k * hs + hc of the response
template <bool STEREO, bool PERCH>
__device__ __forceinline__ typename std::conditional<STEREO, cv_v2f, float>::type cv_tap(const cv_gf *__restrict__ hp, unsigned k, unsigned hs, unsigned hc) {
    if constexpr (STEREO) {
        if constexpr (PERCH) return cv_v2f{hp[2 * k], hp[2 * k + 1]};
        else return cv_v2f{hp[k], hp[k]};
    } else {
        return hp[k * hs + hc];
    }
}

// LO taps from k on (the first `rem` of them where GUARD): xr[7 - u] is the staged frame that enters the window at step u.
// Before step 0, w[j] holds the frame output j meets at tap k for j = 1 .. LO - 1; step u puts the entering frame into
// w[(LO - u) % LO], and output j then reads w[(j - u) mod LO]. After LO steps the ring is back where it began, LO frames on.
template <bool STEREO, bool PERCH, bool GUARD, class V>
__device__ __forceinline__ void cv_round(const V *xr, const cv_gf *__restrict__ hp, unsigned k, unsigned hs, unsigned hc, unsigned rem, V (&w)[kCvLO],
                                         V (&acc)[kCvLO]) {
#pragma unroll
    for (unsigned u = 0; u < kCvLO; u++) {
        if (GUARD && u >= rem) break;   // (uniform)
        w[(kCvLO - u) % kCvLO] = xr[kCvLO - 1 - u];
        const V h = cv_tap<STEREO, PERCH>(hp, k + u, hs, hc);
#pragma unroll
        for (unsigned j = 0; j < kCvLO; j++) acc[j] = cv_fma(h, w[(j + kCvLO - u) % kCvLO], acc[j]);
    }
}

template <bool STEREO, bool PERCH>
__global__ __launch_bounds__(kConvThreads) void conv_kernel(const ConvArgs A) {
    typedef typename std::conditional<STEREO, cv_v2f, float>::type V;
    constexpr unsigned LO = kCvLO, KC = kCvKC, TF = kConvTileFrames;
    __shared__ V lds[kConvLdsElems];
    const unsigned tid = threadIdx.x;
    const unsigned clip = tile_clip(A.pre, A.n_out, blockIdx.x);
    const unsigned tile = blockIdx.x - A.pre[clip];
    const ConvJob *__restrict__ jobs = A.jobs;
    const ConvJob J = jobs[clip];
    const unsigned ch = STEREO ? 2u : A.channels;
    const unsigned long long T = J.frames, N = J.n_src, t0 = (unsigned long long)tile * TF;
    const unsigned nf = T - t0 < TF ? (unsigned)(T - t0) : TF;   // >= 1: the tile exists
    const unsigned nf_up = (nf + LO - 1) & ~(LO - 1);            // the frames of the lanes that own one
    const unsigned K = J.taps;
    const cv_gf *__restrict__ src = (const cv_gf *)J.src;
    const cv_gf *__restrict__ hp = (const cv_gf *)J.ir;
    const unsigned hs = J.ir_channels;
    const bool active = tid * LO < nf;
    const V *x = lds + tid * (LO + 1);   // conv_lds_index(tid * LO + s) = tid * (LO + 1) + conv_lds_index(s)
    float *__restrict__ dp = A.dst + J.dst_off + t0 * ch;   // 16-byte aligned: the clip is, and so are TF * ch floats

    for (unsigned c = 0; c < (STEREO ? 1u : ch); c++) {
        const unsigned hc = hs == 1 ? 0u : c;
        V acc[LO];
#pragma unroll
        for (unsigned j = 0; j < LO; j++) acc[j] = V(0.f);
        for (unsigned k0 = 0; k0 < K; k0 += KC) {
            const unsigned nc = K - k0 < KC ? K - k0 : KC;
            // (t0 + skip stays far below 2^63: both are bounded by frame counts, conv_skip)
            const long long base = (long long)(t0 + J.skip) - (long long)(k0 + KC - 1);
            __syncthreads();   // the chunk or the plane before has been read
            // the staged frames this chunk reads: from KC - nc (tap k0 + nc - 1 of output 0) to nf_up + KC - 2 (tap k0 of the last)
            if (N) {
                const unsigned long long last = N - 1;
#pragma unroll 4
                for (unsigned s = KC - nc + tid; s < nf_up + KC - 1; s += kConvThreads) {
                    const long long m = base + (long long)s;
                    const bool in = m >= 0 && (unsigned long long)m <= last;
                    const unsigned long long cm = m < 0 ? 0ull : ((unsigned long long)m > last ? last : (unsigned long long)m);
                    V v;
                    if constexpr (STEREO) v = ((const cv_g2f *)J.src)[cm];
                    else v = src[cm * ch + c];
                    lds[conv_lds_index(s)] = in ? v : V(0.f);
                }
            } else {
                for (unsigned s = KC - nc + tid; s < nf_up + KC - 1; s += kConvThreads) lds[conv_lds_index(s)] = V(0.f);
            }
            __syncthreads();
            if (active) {
                V w[LO];
                w[0] = V(0.f);   // (entered at step 0)
#pragma unroll
                for (unsigned j = 1; j < LO; j++) w[j] = x[conv_lds_index(KC - 1 + j)];
                unsigned kk = 0;
                for (; kk + LO <= nc; kk += LO)
                    cv_round<STEREO, PERCH, false>(x + (KC - LO - kk) / LO * (LO + 1), hp, k0 + kk, hs, hc, LO, w, acc);
                if (kk < nc) cv_round<STEREO, PERCH, true>(x + (KC - LO - kk) / LO * (LO + 1), hp, k0 + kk, hs, hc, nc - kk, w, acc);
            }
        }
        if (!active) continue;
        const unsigned f0 = tid * LO;
        if (STEREO) {
            if (f0 + LO <= nf) {
#pragma unroll
                for (unsigned j = 0; j < LO; j += 2)
                    *reinterpret_cast<cv_v4f *>(dp + 2 * (f0 + j)) = cv_v4f{cv_first(acc[j]), cv_second(acc[j]),
                                                                            cv_first(acc[j + 1]), cv_second(acc[j + 1])};
            } else {
#pragma unroll
                for (unsigned j = 0; j < LO; j++)
                    if (f0 + j < nf) {
                        dp[2 * (f0 + j)] = cv_first(acc[j]);
                        dp[2 * (f0 + j) + 1] = cv_second(acc[j]);
                    }
            }
        } else if (ch == 1 && f0 + LO <= nf) {
#pragma unroll
            for (unsigned j = 0; j < LO; j += 4)
                *reinterpret_cast<cv_v4f *>(dp + f0 + j) = cv_v4f{cv_first(acc[j]), cv_first(acc[j + 1]), cv_first(acc[j + 2]),
                                                                  cv_first(acc[j + 3])};
        } else {
#pragma unroll
            for (unsigned j = 0; j < LO; j++)
                if (f0 + j < nf) dp[(unsigned long long)(f0 + j) * ch + c] = cv_first(acc[j]);
        }
    }
}

int launch_convolve(const ConvArgs &a, unsigned int n_tiles, unsigned int ir_channels, hipStream_t stream) {
    if (!n_tiles) return 0;
    const dim3 grid(n_tiles), block(kConvThreads);
    if (a.channels != 2) conv_kernel<false, false><<<grid, block, 0, stream>>>(a);
    else if (ir_channels == 2) conv_kernel<true, true><<<grid, block, 0, stream>>>(a);
    else conv_kernel<true, false><<<grid, block, 0, stream>>>(a);
    return (int)hipGetLastError();
}

}  // namespace flo
