// fftconv_kernels.hip — uniformly partitioned overlap-save convolution of the clips of a resident batch
// (flo_batch_convolve_fft, flo_convolve_fft; fftconv.cpp). The definition, the descriptors and the geometry are
// fftconv_plan.hpp's: B = kFcBlock frames a block, F = 2B points a transform, spectra of B complex f32 with (DC, Nyquist) in bin 0.
//
// The transform. F real points are B complex ones, z[n] = x[2n] + i x[2n+1]; a radix-2 Stockham FFT of B points runs in LDS
// between two buffers (log2 B stages, B / 2 butterflies each, one barrier a stage; kFcTogether transforms side by side so
// that every lane has a butterfly), and the real spectrum comes out of Z[k] and Z[B-k] with one twiddle W_F^k. The inverse
// undoes this in the opposite order with the conjugate twiddles. Butterfly j of a stage of stride s reads elements j and
// j + B/2 (8-byte units, consecutive lanes consecutive: no bank conflict) and writes 2j - (j mod s) and that plus s: runs of
// s consecutive elements, so the first stage writes 16 bytes apart (two lanes a bank pair, a 2-way conflict), the second
// 8-byte pairs, and from s = 4 on whole runs. The twiddles W_F^k, k < B, are read from an LDS copy of the host's table.
//
// fc_spectra_kernel: one workgroup per kFcTogether transforms of one signal (a response's partitions, a job's segments):
// loads at clamped frames, the padding and everything outside the signal zeroed in registers, transform, store.
//
// fc_mac_kernel: one workgroup per (tile of kFcLaneBlocks output blocks, channel). A lane owns the bins tid + i * 256. It
// keeps kFcLaneBlocks accumulators per bin in registers and walks p in ascending order: block b0 + j meets partition p at
// segment b0 + j - p, so going from p to p + 1 every block takes over its lower neighbour's segment and one segment enters.
// The window of segment spectra is a ring that rotates by name (the loop is unrolled by kFcLaneBlocks): each p costs one
// 8-byte load of X and one of H_p per bin, and 4 FMAs per block. Segments outside the job's stored range are zero and are
// skipped (a uniform branch), and p runs only over the partitions that meet a stored segment. Then the blocks go through the
// inverse transform in LDS, kFcTogether at a time, and the last B values of each are stored.
// No atomics; nothing depends on the launch's other workgroups. Compiled with -ffp-contract=off; the FMAs are explicit.
#include "clip_tiles.hpp"
#include "fftconv_kernels.hpp"

namespace flo {

typedef float fc_v2 __attribute__((ext_vector_type(2)));
typedef const float __attribute__((address_space(1))) fc_gf;
typedef const fc_v2 __attribute__((address_space(1))) fc_g2;

constexpr unsigned kB = kFcBlock, kLB = kFcLaneBlocks, kTG = kFcTogether, kTH = kFcThreads, kBPL = kFcBinsPerLane;

__device__ __forceinline__ fc_v2 fc_cmul(fc_v2 a, fc_v2 w) { return fc_v2{a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x}; }

// nt transforms of kB points, transform t at a[t * kB ..); the buffer that holds the result is returned (a barrier behind it)
template <bool INV>
__device__ __forceinline__ fc_v2 *fc_fft(fc_v2 *a, fc_v2 *b, const fc_v2 *tw, unsigned nt, unsigned tid) {
#pragma unroll
    for (unsigned s = 1; s < kB; s <<= 1) {
        for (unsigned i = tid; i < nt * (kB / 2); i += kTH) {
            const unsigned t = i / (kB / 2), j = i % (kB / 2), q = j & (s - 1);
            const fc_v2 u = a[t * kB + j], v = a[t * kB + j + kB / 2];
            fc_v2 w = tw[2 * (j - q)];   // W_B^(j - q)
            if (INV) w.y = -w.y;
            b[t * kB + 2 * j - q] = u + v;
            b[t * kB + 2 * j - q + s] = fc_cmul(u - v, w);
        }
        __syncthreads();
        fc_v2 *const o = a;
        a = b;
        b = o;
    }
    return a;
}

__global__ __launch_bounds__(kFcThreads) void fc_spectra_kernel(const FcSpecArgs A) {
    __shared__ fc_v2 la[kTG * kB], lb[kTG * kB], ltw[kB];
    const unsigned tid = threadIdx.x;
    const unsigned job = tile_clip(A.pre, A.n_jobs, blockIdx.x);
    const unsigned first = (blockIdx.x - A.pre[job]) * kTG;
    const FcSpecJob J = A.jobs[job];
    const unsigned nt = J.items - first < kTG ? J.items - first : kTG;   // >= 1: the tile exists
    fc_gf *__restrict__ base = (fc_gf *)J.base;
    for (unsigned i = tid; i < kB; i += kTH) ltw[i] = ((fc_g2 *)A.tw)[i];
    for (unsigned i = tid; i < nt * kB; i += kTH) {
        const unsigned t = i / kB, n = i % kB, item = first + t, tr = item / J.channels, c = item % J.channels;
        fc_v2 v = fc_v2{0.f, 0.f};
        if (J.len && 2 * n < J.live) {   // (live is even: a pair is inside it or outside)
            const long long m = J.start + (long long)tr * (long long)kB + 2 * n;
            const unsigned long long last = J.len - 1;
            const unsigned long long c0 = m < 0 ? 0ull : ((unsigned long long)m > last ? last : (unsigned long long)m);
            const unsigned long long c1 = m + 1 < 0 ? 0ull : ((unsigned long long)(m + 1) > last ? last : (unsigned long long)(m + 1));
            const float v0 = base[c0 * J.channels + c], v1 = base[c1 * J.channels + c];
            v.x = (m >= 0 && (unsigned long long)m <= last) ? v0 : 0.f;
            v.y = (m + 1 >= 0 && (unsigned long long)(m + 1) <= last) ? v1 : 0.f;
        }
        la[i] = v;
    }
    __syncthreads();
    const fc_v2 *z = fc_fft<false>(la, lb, ltw, nt, tid);
    for (unsigned i = tid; i < nt * kB; i += kTH) {
        const unsigned t = i / kB, k = i % kB;
        const fc_v2 zk = z[i], zm = z[t * kB + ((kB - k) & (kB - 1))];
        fc_v2 y;
        if (k == 0) {
            y = fc_v2{zk.x + zk.y, zk.x - zk.y};
        } else {
            const fc_v2 ye = fc_v2{0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y)};   // (Z[k] + conj Z[B-k]) / 2
            const fc_v2 yo = fc_v2{0.5f * (zk.y + zm.y), -0.5f * (zk.x - zm.x)};  // (Z[k] - conj Z[B-k]) / 2i
            y = ye + fc_cmul(yo, ltw[k]);
        }
        A.out[J.out + (unsigned long long)(first + t) * kB + k] = float2{y.x, y.y};
    }
}

__device__ __forceinline__ fc_v2 fc_mac(fc_v2 x, float hx, float hb, float hd, fc_v2 a) {
    a.x = __builtin_fmaf(x.x, hx, a.x);
    a.x = __builtin_fmaf(-x.y, hb, a.x);
    a.y = __builtin_fmaf(x.x, hb, a.y);
    a.y = __builtin_fmaf(x.y, hd, a.y);
    return a;
}

// kLB partitions from p on (the first `rem` of them where GUARD). Before step 0, w[j] holds segment b0 + j - p for
// j = 1 .. kLB - 1; step u puts segment b0 - p - u into w[(kLB - u) % kLB], and block j then reads w[(j - u) mod kLB].
template <bool GUARD>
__device__ __forceinline__ void fc_round(fc_g2 *__restrict__ X, fc_g2 *__restrict__ H, long long q0, long long s0, long long s1, unsigned long long x_step,
                                         unsigned long long h_step, unsigned p, unsigned rem, unsigned tid, fc_v2 (&w)[kLB][kBPL],
                                         fc_v2 (&acc)[kLB][kBPL]) {
#pragma unroll
    for (unsigned u = 0; u < kLB; u++) {
        if (GUARD && u >= rem) break;   // (uniform)
        const long long q = q0 - (long long)u;
        const bool in = q >= s0 && q < s1;   // (uniform)
#pragma unroll
        for (unsigned i = 0; i < kBPL; i++) {
            fc_v2 x = fc_v2{0.f, 0.f};
            if (in) x = X[(unsigned long long)(q - s0) * x_step + tid + i * kTH];
            w[(kLB - u) % kLB][i] = x;
        }
#pragma unroll
        for (unsigned i = 0; i < kBPL; i++) {
            const fc_v2 h = H[(unsigned long long)(p + u) * h_step + tid + i * kTH];
            const bool packed = i == 0 && tid == 0;   // bin 0: (DC, Nyquist), two real products
            const float hb = packed ? 0.f : h.y, hd = packed ? h.y : h.x;
#pragma unroll
            for (unsigned j = 0; j < kLB; j++) acc[j][i] = fc_mac(w[(j + kLB - u) % kLB][i], h.x, hb, hd, acc[j][i]);
        }
    }
}

__global__ __launch_bounds__(kFcThreads) void fc_mac_kernel(const FcMacArgs A) {
    __shared__ fc_v2 la[kTG * kB], lb[kTG * kB], ltw[kB];
    const unsigned tid = threadIdx.x;
    const unsigned entry = tile_clip(A.pre, A.n_jobs, blockIdx.x);
    const unsigned tile = blockIdx.x - A.pre[entry];
    const FcMacJob J = A.jobs[entry];
    const unsigned C = A.channels, c = blockIdx.y, hs = J.ir_channels, hc = hs == 1 ? 0u : c;
    const long long b0 = (long long)(J.b0 + (unsigned long long)tile * kLB);
    for (unsigned i = tid; i < kB; i += kTH) ltw[i] = ((fc_g2 *)A.tw)[i];

    fc_v2 acc[kLB][kBPL];
#pragma unroll
    for (unsigned j = 0; j < kLB; j++)
#pragma unroll
        for (unsigned i = 0; i < kBPL; i++) acc[j][i] = fc_v2{0.f, 0.f};

    // partitions that meet a stored segment: b0 + kLB - 1 - p >= s0 and b0 - p <= s1 - 1
    const long long lo = b0 - (J.s1 - 1), hi = b0 + (long long)kLB - J.s0;
    const unsigned p_lo = lo > 0 ? (unsigned)(lo < (long long)J.parts ? lo : (long long)J.parts) : 0u;
    const unsigned p_hi = hi < (long long)J.parts ? (hi > 0 ? (unsigned)hi : 0u) : J.parts;
    if (J.s1 > J.s0 && p_hi > p_lo) {
        fc_g2 *__restrict__ X = (fc_g2 *)A.x + J.x_off + (unsigned long long)c * kB;
        fc_g2 *__restrict__ H = (fc_g2 *)A.h + J.h_off + (unsigned long long)hc * kB;
        const unsigned long long x_step = (unsigned long long)C * kB, h_step = (unsigned long long)hs * kB;
        fc_v2 w[kLB][kBPL];
#pragma unroll
        for (unsigned j = 0; j < kLB; j++) {
            const long long q = b0 + (long long)j - (long long)p_lo;
            const bool in = j > 0 && q >= J.s0 && q < J.s1;   // (w[0] is entered at step 0)
#pragma unroll
            for (unsigned i = 0; i < kBPL; i++) {
                fc_v2 x = fc_v2{0.f, 0.f};
                if (in) x = X[(unsigned long long)(q - J.s0) * x_step + tid + i * kTH];
                w[j][i] = x;
            }
        }
        unsigned p = p_lo;
        for (; p + kLB <= p_hi; p += kLB) fc_round<false>(X, H, b0 - (long long)p, J.s0, J.s1, x_step, h_step, p, kLB, tid, w, acc);
        if (p < p_hi) fc_round<true>(X, H, b0 - (long long)p, J.s0, J.s1, x_step, h_step, p, p_hi - p, tid, w, acc);
    }

    float *__restrict__ dp = A.dst + J.dst_off;
    const unsigned long long T = J.frames;
    const float scale = 1.f / (float)(2 * kB);   // a power of two
#pragma unroll
    for (unsigned j0 = 0; j0 < kLB; j0 += kTG) {
        __syncthreads();   // the twiddles are there; the round before has been read
#pragma unroll
        for (unsigned t = 0; t < kTG; t++)
#pragma unroll
            for (unsigned i = 0; i < kBPL; i++) lb[t * kB + tid + i * kTH] = j0 + t < kLB ? acc[(j0 + t) % kLB][i] : fc_v2{0.f, 0.f};
        __syncthreads();
#pragma unroll
        for (unsigned t = 0; t < kTG; t++)
#pragma unroll
            for (unsigned i = 0; i < kBPL; i++) {
                const unsigned k = tid + i * kTH;
                const fc_v2 yk = lb[t * kB + k], ym = lb[t * kB + ((kB - k) & (kB - 1))];
                fc_v2 z;
                if (k == 0) {
                    z = fc_v2{yk.x + yk.y, yk.x - yk.y};
                } else {
                    const fc_v2 s = fc_v2{yk.x + ym.x, yk.y - ym.y};   // Y[k] + conj Y[B-k]
                    fc_v2 wk = ltw[k];
                    wk.y = -wk.y;
                    const fc_v2 yo = fc_cmul(fc_v2{yk.x - ym.x, yk.y + ym.y}, wk);   // (Y[k] - conj Y[B-k]) W_F^-k
                    z = fc_v2{s.x - yo.y, s.y + yo.x};
                }
                la[t * kB + k] = z;
            }
        __syncthreads();
        const fc_v2 *z = fc_fft<true>(la, lb, ltw, kTG, tid);
        // the last B values of a block: points B/2 .. B-1 of its transform, two frames each
        for (unsigned i = tid; i < kTG * (kB / 2); i += kTH) {
            const unsigned t = i / (kB / 2), n = i % (kB / 2);
            if (j0 + t >= kLB) continue;
            const unsigned long long f = (unsigned long long)(b0 + j0 + t) * kB + 2 * n;
            const fc_v2 v = z[t * kB + kB / 2 + n] * scale;
            if (f + 1 < T && C == 1) {
                *reinterpret_cast<fc_v2 *>(dp + f) = v;   // 8-byte aligned: the clip is 16-byte aligned and f is even
            } else {
                if (f < T) dp[f * C + c] = v.x;
                if (f + 1 < T) dp[(f + 1) * C + c] = v.y;
            }
        }
    }
}

int launch_fftconv_spectra(const FcSpecArgs &a, unsigned int n_tiles, hipStream_t stream) {
    if (!n_tiles) return 0;
    fc_spectra_kernel<<<dim3(n_tiles), dim3(kFcThreads), 0, stream>>>(a);
    return (int)hipGetLastError();
}

int launch_fftconv_mac(const FcMacArgs &a, unsigned int n_tiles, hipStream_t stream) {
    if (!n_tiles) return 0;
    fc_mac_kernel<<<dim3(n_tiles, a.channels), dim3(kFcThreads), 0, stream>>>(a);
    return (int)hipGetLastError();
}

}  // namespace flo
