// normalize_kernels.hip — the 4x oversampled peak of every clip of a batch, and the batch at a new level under a true-peak
// ceiling (flo_batch_true_peak, flo_batch_normalize, flo_normalize; normalize.cpp). The definition, the skip bound and the
// tile geometry are normalize_plan.hpp's.
//
// One workgroup per tile of the flat (clip, tile) list; it finds its clip by binary search over the per-clip prefix, as the
// sample-rate conversion does. The envelope is that conversion's arithmetic at L = 4, M = 1: a lane reads a frame's 64 taps
// from the staged plane (neighbouring lanes one element apart: no bank conflicts) and feeds each into the four rows' FMA
// chains; h[q][k] is wave-uniform, so it comes through scalar loads; a thread makes four frames, 512 apart, side by side
// (np_envelope_bits). One channel is staged at a time, p gathers
// the maximum over the channels in a second plane (a thread owns the same frames in every pass).
//
// The limiter's tile, long path: y of channel c -> plane 0; p (bit patterns: magnitudes order like unsigned integers) ->
// plane 1; r in place; the sliding minimum over 2A + 1 by doubling, ping-pong between the planes (log2 steps); m split
// into 12-bit halves whose inclusive prefix sums (below 2^26 each) replace m and fill the other plane; then
// S[n] = P[n + A] - P[n - A - 1], s = S div (2A + 1) and the stores. Everything behind p is integer arithmetic, so the order
// of the scans does not matter. Short path: when max |y| over the staged span times the bound B is at most C, every r is
// 2^24 and the tile stores y. The test is made on a value every wave reads from LDS: a wave-uniform branch.
//
// Compiled with -ffp-contract=off; the FMAs are explicit, x * g and y * scale are single multiplications.
#include <mutex>
#include <set>
#include <utility>

#include "clip_tiles.hpp"
#include "normalize_kernels.hpp"

namespace flo {

extern __shared__ __attribute__((aligned(16))) char np_smem[];

typedef float np_v4f __attribute__((ext_vector_type(4)));
typedef unsigned int np_v4u __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned np_abs_bits(float v) { return __float_as_uint(v) & 0x7FFFFFFFu; }
__device__ __forceinline__ unsigned np_umax(unsigned a, unsigned b) { return a > b ? a : b; }
__device__ __forceinline__ unsigned np_umin(unsigned a, unsigned b) { return a < b ? a : b; }

// bits[j] = the bits of max(|y|, max_q |e_q|) of the frame whose 64 taps start at plane[f[j]], for kNormGroup frames side
// by side, eight taps of the four rows at a time: 32 coefficients are live in scalar registers, not 256 (which the compiler
// hoists out of the frame loop and spills into VGPR lanes: that form of the peak kernel took 16.7 ms where this one takes
// 8.0), and every coefficient loaded feeds kNormGroup frames. Each chain still runs over k = 0 .. 63 in that order.
constexpr unsigned kNormGroup = 4;
__device__ __forceinline__ void np_envelope_bits(const float *plane, const unsigned (&f)[kNormGroup], const float *__restrict__ h,
                                                 unsigned (&bits)[kNormGroup]) {
    float acc[kNormGroup][kNormPhases];
#pragma unroll
    for (unsigned j = 0; j < kNormGroup; j++)
#pragma unroll
        for (unsigned q = 0; q < kNormPhases; q++) acc[j][q] = 0.f;
#pragma unroll 1
    for (unsigned kb = 0; kb < kNormTaps; kb += 8) {
#pragma unroll
        for (unsigned i = 0; i < 8; i++) {
            const unsigned k = kb + i;
#pragma unroll
            for (unsigned j = 0; j < kNormGroup; j++) {
                const float v = plane[f[j] + k];
#pragma unroll
                for (unsigned q = 0; q < kNormPhases; q++) acc[j][q] = __builtin_fmaf(h[q * kNormTaps + k], v, acc[j][q]);
            }
        }
    }
#pragma unroll
    for (unsigned j = 0; j < kNormGroup; j++) {
        unsigned m = np_abs_bits(plane[f[j] + kNormBefore]);
#pragma unroll
        for (unsigned q = 0; q < kNormPhases; q++) m = np_umax(m, np_abs_bits(acc[j][q]));
        bits[j] = m;
    }
}

// plane[f] = g * (channel c of frame y0 + f), zero outside the clip's n frames
__device__ __forceinline__ void np_stage(float *plane, unsigned span, const float *__restrict__ src, long long y0, unsigned long long n,
                                         unsigned ch, unsigned c, float g, unsigned tid) {
    for (unsigned f = tid; f < span; f += kNormThreads) {
        const long long sf = y0 + (long long)f;
        float v = 0.f;
        if (sf >= 0 && (unsigned long long)sf < n) v = src[(unsigned long long)sf * ch + c] * g;
        plane[f] = v;
    }
}

// the maximum of v over the workgroup, in every thread (red: 8 words; two barriers)
__device__ __forceinline__ unsigned np_block_umax(unsigned v, unsigned *red, unsigned tid) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = np_umax(v, (unsigned)__shfl_xor((int)v, o));
    __syncthreads();   // (red may still be read from an earlier use)
    if ((tid & 63u) == 0) red[tid >> 6] = v;
    __syncthreads();
    unsigned m = red[0];
#pragma unroll
    for (unsigned w = 1; w < kNormThreads / 64; w++) m = np_umax(m, red[w]);
    return m;
}

// n floats of a tile from src to dst, both 16-byte aligned: copied bit for bit, or multiplied by g
__device__ __forceinline__ void np_store_tile(const float *__restrict__ src, float *__restrict__ dst, unsigned n, float g, bool copy, unsigned tid) {
    const unsigned n4 = n >> 2;
    if (copy) {
        const np_v4u *s4 = reinterpret_cast<const np_v4u *>(src);
        np_v4u *d4 = reinterpret_cast<np_v4u *>(dst);
        for (unsigned i = tid; i < n4; i += kNormThreads) d4[i] = s4[i];
        const unsigned *s1 = reinterpret_cast<const unsigned *>(src);
        unsigned *d1 = reinterpret_cast<unsigned *>(dst);
        for (unsigned i = 4 * n4 + tid; i < n; i += kNormThreads) d1[i] = s1[i];
    } else {
        const np_v4f *s4 = reinterpret_cast<const np_v4f *>(src);
        np_v4f *d4 = reinterpret_cast<np_v4f *>(dst);
        for (unsigned i = tid; i < n4; i += kNormThreads) d4[i] = s4[i] * g;
        for (unsigned i = 4 * n4 + tid; i < n; i += kNormThreads) dst[i] = src[i] * g;
    }
}

__global__ __launch_bounds__(kNormThreads) void norm_peak_kernel(const NormArgs A) {
    __shared__ unsigned red[kNormThreads / 64];
    const unsigned tid = threadIdx.x;
    const unsigned clip = tile_clip(A.pre, A.n_clips, blockIdx.x);
    const unsigned tile = blockIdx.x - A.pre[clip];
    const unsigned long long n = A.frames[clip];
    const float *__restrict__ src = A.src + A.src_off[clip];
    const unsigned ch = A.channels, F = norm_tile_frames(0), span = norm_span(0);
    static_assert(kNormGroup * kNormThreads == kNormMinTile, "a thread of the peak kernel makes one group of frames of its tile");
    const unsigned long long t0 = (unsigned long long)tile * F;
    const unsigned nf = n - t0 < F ? (unsigned)(n - t0) : F;
    float *plane = reinterpret_cast<float *>(np_smem);
    unsigned best = 0;
    for (unsigned c = 0; c < ch; c++) {
        if (c) __syncthreads();
        np_stage(plane, span, src, norm_y0(tile, 0), n, ch, c, 1.0f, tid);
        __syncthreads();
        unsigned f[kNormGroup], bits[kNormGroup];   // (a tile of the peak kernel is one group per thread; frames at or beyond nf read inside the plane)
#pragma unroll
        for (unsigned j = 0; j < kNormGroup; j++) f[j] = tid + j * kNormThreads;
        np_envelope_bits(plane, f, A.table, bits);
#pragma unroll
        for (unsigned j = 0; j < kNormGroup; j++)
            if (f[j] < nf) best = np_umax(best, bits[j]);
    }
    best = np_block_umax(best, red, tid);
    if (tid == 0 && best) atomicMax(A.peak_bits + clip, best);
}

__global__ __launch_bounds__(kNormThreads) void norm_gain_kernel(const NormArgs A) {
    const unsigned clip = tile_clip(A.pre, A.n_clips, blockIdx.x);
    const unsigned tile = blockIdx.x - A.pre[clip];
    const unsigned long long n = A.frames[clip];
    const unsigned ch = A.channels, F = norm_tile_frames(0);
    const unsigned long long t0 = (unsigned long long)tile * F;
    const unsigned nf = n - t0 < F ? (unsigned)(n - t0) : F;
    np_store_tile(A.src + A.src_off[clip] + t0 * ch, A.dst + A.dst_off[clip] + t0 * ch, nf * ch, A.gain[clip], A.copy[clip] != 0, threadIdx.x);
}

__global__ __launch_bounds__(kNormThreads) void norm_limit_kernel(const NormArgs A) {
    __shared__ unsigned red[kNormThreads / 64];
    __shared__ unsigned long long wsum[kNormThreads / 64];
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const unsigned clip = tile_clip(A.pre, A.n_clips, blockIdx.x);
    const unsigned tile = blockIdx.x - A.pre[clip];
    const unsigned long long n = A.frames[clip];
    const float *__restrict__ src = A.src + A.src_off[clip];
    float *__restrict__ dst = A.dst + A.dst_off[clip];
    const unsigned ch = A.channels, la = A.lookahead, F = norm_tile_frames(la), span = norm_span(la);
    const unsigned long long t0 = (unsigned long long)tile * F;
    const unsigned nf = n - t0 < F ? (unsigned)(n - t0) : F;
    const float g = A.gain[clip];
    if (A.copy[clip]) {
        np_store_tile(src + t0 * ch, dst + t0 * ch, nf * ch, g, true, tid);
        return;
    }
    // max |y| over the staged span, every channel: the clip's frames [lo, hi)
    const long long y0 = norm_y0(tile, la);
    const unsigned long long lo = y0 < 0 ? 0ull : (unsigned long long)y0;
    const unsigned long long hi = (unsigned long long)(y0 + (long long)span) < n ? (unsigned long long)(y0 + (long long)span) : n;
    unsigned peak = 0;
    {
        const float *__restrict__ s = src + lo * ch;
        const unsigned cnt = (unsigned)((hi - lo) * ch);
        for (unsigned i = tid; i < cnt; i += kNormThreads) peak = np_umax(peak, np_abs_bits(s[i] * g));
    }
    peak = np_block_umax(peak, red, tid);
    if (!A.no_skip && __uint_as_float(peak) * A.bound <= A.ceiling) {
        np_store_tile(src + t0 * ch, dst + t0 * ch, nf * ch, g, false, tid);
        return;
    }
    unsigned *pa = reinterpret_cast<unsigned *>(np_smem);   // plane 0
    unsigned *pb = pa + span;                               // plane 1
    const unsigned lr = norm_r_len(la), lm = norm_m_len(la);
    const long long r0 = norm_r0(tile, la);
    for (unsigned c = 0; c < ch; c++) {
        if (c) __syncthreads();
        np_stage(reinterpret_cast<float *>(pa), span, src, y0, n, ch, c, g, tid);
        __syncthreads();
        for (unsigned base = 0; base < lr; base += kNormGroup * kNormThreads) {   // (uniform: every wave makes every group)
            unsigned f[kNormGroup], bits[kNormGroup];
#pragma unroll
            for (unsigned j = 0; j < kNormGroup; j++) {   // frames beyond r's last read the last one's taps and are dropped
                const unsigned fj = base + tid + j * kNormThreads;
                f[j] = fj < lr ? fj : lr - 1;
            }
            np_envelope_bits(reinterpret_cast<const float *>(pa), f, A.table, bits);
#pragma unroll
            for (unsigned j = 0; j < kNormGroup; j++) {
                const unsigned fj = base + tid + j * kNormThreads;
                const long long sf = r0 + (long long)fj;
                if (fj < lr && sf >= 0 && (unsigned long long)sf < n) pb[fj] = c ? np_umax(pb[fj], bits[j]) : bits[j];
            }
        }
    }
    // r in place (the same thread made p[f])
    for (unsigned f = tid; f < lr; f += kNormThreads) {
        const long long sf = r0 + (long long)f;
        unsigned r = kNormUnity;
        if (sf >= 0 && (unsigned long long)sf < n) {
            const float p = __uint_as_float(pb[f]);
            if (!(p <= A.ceiling)) r = (unsigned)(__fdiv_rn(A.ceiling, p) * 16777216.0f);
        }
        pb[f] = r;
    }
    __syncthreads();
    // a[i] = min r[i .. i + j - 1] (as far as r reaches), j doubling up to the largest power of two in the window
    unsigned *a = pb, *b = pa;
    const unsigned pw = norm_min_pow2(la);
    for (unsigned j = 1; j < pw; j *= 2) {
        for (unsigned f = tid; f < lr; f += kNormThreads) b[f] = np_umin(a[f], f + j < lr ? a[f + j] : kNormUnity);
        __syncthreads();
        unsigned *t = a;
        a = b;
        b = t;
    }
    // m[i] = min r[i .. i + 2A]: two windows of pw
    const unsigned shift = 2 * la + 1 - pw;
    for (unsigned i = tid; i < lm; i += kNormThreads) b[i] = np_umin(a[i], a[i + shift]);
    __syncthreads();
    unsigned *m = b, *lows = a;
    // inclusive prefix sums of m's halves: hi = m >> 12 in the upper word, lo = m & 4095 in the lower, each sum below 2^26
    const unsigned chunk = norm_scan_chunk(la);
    const unsigned c0 = tid * chunk, c1 = c0 + chunk < lm ? c0 + chunk : lm;
    unsigned long long run = 0;
    for (unsigned i = c0; i < c1; i++) run += ((unsigned long long)(m[i] >> 12) << 32) | (m[i] & 4095u);
    unsigned long long incl = run;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long up = __shfl_up(incl, o);
        if ((int)lane >= o) incl += up;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    unsigned long long acc = incl - run;
    for (unsigned w = 0; w < wave; w++) acc += wsum[w];
    for (unsigned i = c0; i < c1; i++) {
        const unsigned v = m[i];
        acc += ((unsigned long long)(v >> 12) << 32) | (v & 4095u);
        m[i] = (unsigned)(acc >> 32);
        lows[i] = (unsigned)acc;
    }
    __syncthreads();
    // S[t0 + j] = sum m[j .. j + 2A]
    const unsigned w = 2 * la + 1;
    unsigned long long limited = 0;
    unsigned least = kNormUnity;
    for (unsigned j = tid; j < nf; j += kNormThreads) {
        const unsigned shi = m[j + 2 * la] - (j ? m[j - 1] : 0u), slo = lows[j + 2 * la] - (j ? lows[j - 1] : 0u);
        const unsigned long long S = (unsigned long long)shi * 4096ull + slo;
        const unsigned s = (unsigned)(S / w);
        const float scale = (float)s * 0x1p-24f;
        const unsigned long long e = (t0 + j) * ch;
        for (unsigned c = 0; c < ch; c++) dst[e + c] = (src[e + c] * g) * scale;
        limited += s < kNormUnity;
        least = np_umin(least, s);
    }
    // the report words: one pair of atomics per tile that limited anything
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) limited += __shfl_xor(limited, o);
    __syncthreads();   // (wsum was read above)
    if (lane == 0) wsum[wave] = limited;
    least = ~np_block_umax(~least, red, tid);
    if (tid == 0) {
        unsigned long long total = 0;
        for (unsigned v = 0; v < kNormThreads / 64; v++) total += wsum[v];
        if (total) {
            atomicAdd(A.limited + clip, total);
            atomicMin(A.min_q + clip, least);
        }
    }
}

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-device property of a kernel: set once per device under a lock
static int np_allow_lds(const void *fn) {
    static std::mutex mu;
    static std::set<std::pair<int, const void *>> done;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return (int)e;
    std::lock_guard<std::mutex> g(mu);
    if (done.count({dev, fn})) return 0;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kNormLdsBytes);
    if (e != hipSuccess) return (int)e;
    done.insert({dev, fn});
    return 0;
}

int launch_norm_peak(const NormArgs &a, unsigned int n_tiles, hipStream_t stream) {
    if (!n_tiles) return 0;
    norm_peak_kernel<<<dim3(n_tiles), dim3(kNormThreads), norm_span(0) * 4, stream>>>(a);
    return (int)hipGetLastError();
}

int launch_norm_gain(const NormArgs &a, unsigned int n_tiles, hipStream_t stream) {
    if (!n_tiles) return 0;
    norm_gain_kernel<<<dim3(n_tiles), dim3(kNormThreads), 0, stream>>>(a);
    return (int)hipGetLastError();
}

int launch_norm_limit(const NormArgs &a, unsigned int n_tiles, hipStream_t stream) {
    if (!n_tiles) return 0;
    const unsigned lds = norm_lds_bytes(a.lookahead);
    if (a.lookahead < 1 || a.lookahead > kNormMaxLookahead || lds > kNormLdsBytes) return (int)hipErrorInvalidValue;
    if (int rc = np_allow_lds(reinterpret_cast<const void *>(&norm_limit_kernel))) return rc;
    norm_limit_kernel<<<dim3(n_tiles), dim3(kNormThreads), lds, stream>>>(a);
    return (int)hipGetLastError();
}

}  // namespace flo
