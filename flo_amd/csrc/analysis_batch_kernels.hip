// analysis_batch_kernels.hip — the analysis of every clip of a batch in one device pass (flo_batch_analyze_all).
//
// The kernels of analysis_kernels.hip, one launch per kernel for a whole group of clips instead of one per clip: the same
// bodies (analysis_device.hpp) or, for the K-weighting passes and the true-peak FIR, the same arithmetic in the same order
// with the data staged for thousands of clips at once - every clip gets bit for bit what the per-clip path gives.
// A grid is a flat work list of (clip, item) over the group (AnBatchArgs, analysis_kernels.hpp); each workgroup finds its
// clip by binary search over the list's per-clip prefix, reads that clip's AnalysisArgs from the descriptor array and
// takes an_batch_per_wg items of it in turn.
// What one workgroup walks alone for one clip - the hash tree, the prefix and chain of the sum of squares, the
// K-weighting scan, the peak reduce - is one workgroup per clip in one launch: thousands of clips side by side where the
// per-clip path left the GPU all but idle. One kernel is new: an_block_energy builds the 400 ms block energies on the
// device, in the host's order of additions, so that only O(blocks + peaks) per clip comes back.
// Compiled with -ffp-contract=off.
#include "analysis_device.hpp"
#include "clip_tiles.hpp"
#include "stream_delay.hpp"

namespace flo {

#define AN_LAUNCH_CHECK()                      \
    do {                                       \
        hipError_t e_ = hipGetLastError();     \
        if (e_ != hipSuccess) return (int)e_;  \
    } while (0)

// Kernel parameters: the group's descriptors, the work lists' prefixes, the number of clips (AnBatchArgs). As kernel
// parameters with __restrict__ the descriptors are known not to change under the kernels' stores: their fields load once.
#define AN_BATCH_PARAMS const AnalysisArgs *__restrict__ clips, const unsigned int *__restrict__ pre, unsigned int n_clips

// the clip of this workgroup in list L and the workgroup's index within that clip. pre[0] = 0 <= blockIdx.x < pre[n]:
// at most log2(n) + 1 steps, every one uniform (scalar loads)
__device__ __forceinline__ const AnalysisArgs &an_clip(const AnalysisArgs *__restrict__ clips, const unsigned int *__restrict__ pre,
                                                       unsigned n_clips, int L, unsigned &wg) {
    const unsigned *p = pre + (unsigned long long)L * (n_clips + 1u);
    const unsigned b = blockIdx.x, lo = tile_clip(p, n_clips, b);
    wg = b - p[lo];
    return clips[lo];
}
// the items [wg * per, (wg + 1) * per) of list L of the clip, one after the other (LDS is reused: a barrier between)
template <int L, class F>
__device__ __forceinline__ void an_items(const AnalysisArgs &A, unsigned wg, F &&f) {
    unsigned long long it[kAnlCount];
    an_batch_items(A, it);
    constexpr unsigned per = an_batch_per_wg(L);
    const unsigned long long i0 = (unsigned long long)wg * per, i1 = i0 + per < it[L] ? i0 + per : it[L];
    for (unsigned long long i = i0; i < i1; i++) {
        if (i > i0) __syncthreads();
        f((unsigned)i);
    }
}

__global__ __launch_bounds__(64) void anb_peaks_kernel(AN_BATCH_PARAMS) {
    unsigned wg;
    const AnalysisArgs &A = an_clip(clips, pre, n_clips, kAnlPeaks, wg);
    an_items<kAnlPeaks>(A, wg, [&](unsigned it) { an_peaks_body(A, it); });
}
__global__ __launch_bounds__(128) void anb_loud_kernel(AN_BATCH_PARAMS) {
    unsigned it;
    const AnalysisArgs &A = an_clip(clips, pre, n_clips, kAnlLoud, it);
    an_loud_body(A, it % A.n_seg, it / A.n_seg);
}

// K-weighting passes 1 and 2 (an_kw_pass_body: one lane walks one segment of kseg_frames frames). In the per-clip kernel
// the 64 lanes of a wave read 64 segments straight from memory, 64 cache lines per load - a few dozen waves keep their lines
// in the caches, the tens of thousands of a batch do not (the passes ran at a sixteenth of the bandwidth). Here the
// workgroup stages kKwStep frames of its 64 segments through LDS with whole-line loads, and every lane walks its own row.
// The arithmetic of every frame, and its order, is that of an_kw_pass_body.
constexpr int kKwStep = 32;
template <int PASS>
__global__ __launch_bounds__(64) void anb_kw_pass_kernel(AN_BATCH_PARAMS) {
    __shared__ float xs[64][kKwStep + 1];   // (+1: the lanes' rows fall in different banks)
    unsigned it;
    const AnalysisArgs &A = an_clip(clips, pre, n_clips, kAnlKw, it);
    const unsigned ch = A.channels, per = (A.n_kseg + 63) / 64, c = it / per, sblk = it % per, lane = threadIdx.x;
    const unsigned L = A.kseg_frames;
    const unsigned long long frames = A.n / ch, seg0 = (unsigned long long)sblk * 64;
    const unsigned long long s = seg0 + lane;
    const bool have = s < A.n_kseg;
    const unsigned long long f0 = s * L;
    const unsigned cnt = have ? (unsigned)(f0 + L < frames ? L : frames - f0) : 0u;   // frames of this segment
    double *st = A.kstate + ((unsigned long long)c * A.n_kseg + s) * 4;
    double s1 = 0, s2 = 0, h1 = 0, h2 = 0;
    if (PASS >= 2 && have) s1 = st[0], s2 = st[1], h1 = st[2], h2 = st[3];
    const double b0 = A.shelf[0], b1 = A.shelf[1], b2 = A.shelf[2], a1 = A.shelf[3], a2 = A.shelf[4];
    const double c0 = A.hp[0], c1 = A.hp[1], c2 = A.hp[2], d1 = A.hp[3], d2 = A.hp[4];
    const unsigned hop = A.hop;
    double acc = 0.0;
    unsigned slot = 0;
    unsigned edge = hop ? (unsigned)((f0 / hop + 1) * (unsigned long long)hop - f0) : 0xFFFFFFFFu;
    double *qp = A.kqpart + ((unsigned long long)c * A.n_kseg + s) * A.kq;
    const float *pcm = A.pcm;
    for (unsigned t0 = 0; t0 < L; t0 += kKwStep) {
        __syncthreads();
        for (unsigned e = lane; e < 64u * kKwStep; e += 64) {   // row j, frame t0 + i: consecutive lanes, consecutive frames
            const unsigned j = e / kKwStep, i = e % kKwStep;
            const unsigned long long f = (seg0 + j) * L + t0 + i;
            xs[j][i] = (seg0 + j < A.n_kseg && t0 + i < L && f < frames) ? pcm[f * ch + c] : 0.f;
        }
        __syncthreads();
        for (unsigned k = 0; k < kKwStep; k++) {
            const unsigned i = t0 + k;
            if (i >= cnt) break;
            const double x = (double)xs[lane][k];
            const double y = b0 * x + s1;
            s1 = b1 * x - a1 * y + s2;
            s2 = b2 * x - a2 * y;
            const double y2 = c0 * y + h1;
            h1 = c1 * y - d1 * y2 + h2;
            h2 = c2 * y - d2 * y2;
            if (PASS == 2) {
                if (i == edge) {   // a quantum ends with the previous frame
                    qp[slot++] = acc;
                    acc = 0.0;
                    edge += hop;
                }
                const double e2 = y2 * y2;
                acc += e2;
            }
        }
    }
    if (!have) return;
    if (PASS == 1) st[0] = s1, st[1] = s2, st[2] = h1, st[3] = h2;
    else if (PASS == 3) {   // the refinement walk's end state (an_kw_scan_body)
        double *st2 = A.kstate2 + ((unsigned long long)c * A.n_kseg + s) * 4;
        st2[0] = s1, st2[1] = s2, st2[2] = h1, st2[3] = h2;
    } else if (cnt) qp[slot] = acc;
}
template <bool REFINE>
__global__ __launch_bounds__(64) void anb_kw_scan_kernel(AN_BATCH_PARAMS) {
    unsigned it;
    const AnalysisArgs &A = an_clip(clips, pre, n_clips, kAnlKScan, it);
    an_kw_scan_body<REFINE>(A, it);
}
__device__ __forceinline__ unsigned an_tiles(const AnalysisArgs &A) {
    const unsigned long long longest = (A.n + A.channels - 1) / A.channels;
    return (unsigned)((longest + kAnTile - 1) / kAnTile);
}

// Sample peak and true-peak FIR of one tile (an_peak_body's outputs and arithmetic: every output adds its 49 taps in
// ascending order). an_peak_body gives a thread eight outputs and a window of 56 doubles in registers (228 VGPRs, two
// waves per SIMD, the lanes' windows 64 bytes apart in the same LDS banks): at the scale of a batch, tens of thousands of
// tiles, it ran at a fraction of the LDS and FMA rates. Here lane t of the workgroup makes outputs t, t + 256, ...: every
// tap is one conflict-free LDS read of 64 consecutive doubles, and the kernel fits in a few dozen registers.
constexpr int kFirSpan = kAnTile + 2 * kAnHalo;
__global__ __launch_bounds__(256) void anb_peak_kernel(AN_BATCH_PARAMS) {
    __shared__ double xt[kFirSpan];
    __shared__ double taps[49];
    __shared__ double wmax[2][4];
    unsigned wg;
    const AnalysisArgs &A = an_clip(clips, pre, n_clips, kAnlTile, wg);
    const unsigned ch = A.channels, tid = threadIdx.x, tiles = an_tiles(A);
    const unsigned long long frames = A.n / ch;
    if (tid < 49) taps[tid] = A.tp_coef[tid];
    const float *pcm = A.pcm;
    unsigned long long it[kAnlCount];
    an_batch_items(A, it);
    constexpr unsigned per = an_batch_per_wg(kAnlTile);
    const unsigned i0 = wg * per, i1 = i0 + per < it[kAnlTile] ? i0 + per : (unsigned)it[kAnlTile];
    for (unsigned item = i0; item < i1; item++) {
        const unsigned c = item / tiles, tile = item % tiles;
        const unsigned long long n_ch = A.n > c ? (A.n - c + ch - 1) / ch : 0;
        const unsigned long long t0 = (unsigned long long)tile * kAnTile;
        if (t0 >= n_ch) {           // (uniform) a shorter channel's empty last tile: the reduction reads every pair
            if (tid < 2) A.peak_part[2ull * ((unsigned long long)c * tiles + tile) + tid] = 0.0;
            continue;
        }
        __syncthreads();            // (the previous tile's readers are done with xt and wmax)
        for (unsigned i = tid; i < kFirSpan; i += 256) {
            const long long f = (long long)t0 - kAnHalo + (long long)i;
            xt[i] = (f >= 0 && (unsigned long long)f < n_ch) ? (double)pcm[(unsigned long long)f * ch + c] : 0.0;
        }
        __syncthreads();
        const unsigned long long t1 = t0 + kAnTile < n_ch ? t0 + kAnTile : n_ch;
        double peak_x = 0.0, peak_fir = 0.0;
        for (unsigned o = tid; o < kAnTile; o += 256) {
            const unsigned long long i = t0 + o;
            if (i >= t1) break;
            double a2 = 0.0;
#pragma unroll 7
            for (int k = 0; k < 49; k++) a2 += xt[o + k] * taps[k];   // taps outside the channel meet zeros: +-0, no change
            if (i < frames) {
                const double a = fabs(xt[o + kAnHalo]);
                if (a > peak_x) peak_x = a;   // (a NaN sample never wins, as with f64::max)
            }
            const double f = fabs(a2);
            if (f > peak_fir) peak_fir = f;
        }
        for (int sh = 32; sh; sh >>= 1) {
            const double px = __shfl_xor(peak_x, sh), pf = __shfl_xor(peak_fir, sh);
            peak_x = px > peak_x ? px : peak_x;
            peak_fir = pf > peak_fir ? pf : peak_fir;
        }
        if ((tid & 63) == 0) wmax[0][tid >> 6] = peak_x, wmax[1][tid >> 6] = peak_fir;
        __syncthreads();
        if (tid < 2) {
            double m = wmax[tid][0];
            for (int k = 1; k < 4; k++) m = wmax[tid][k] > m ? wmax[tid][k] : m;
            A.peak_part[2ull * ((unsigned long long)c * tiles + tile) + tid] = m;
        }
    }
}
__global__ __launch_bounds__(256) void anb_peak_reduce_kernel(AN_BATCH_PARAMS) {
    unsigned it;
    const AnalysisArgs &A = an_clip(clips, pre, n_clips, kAnlFast1, it);
    an_peak_reduce_body(A, (unsigned long long)an_tiles(A) * A.channels);
}
__global__ __launch_bounds__(64) void anb_sq_dsum_kernel(AN_BATCH_PARAMS) {
    unsigned wg;
    const AnalysisArgs &A = an_clip(clips, pre, n_clips, kAnlSqChunk, wg);
    an_items<kAnlSqChunk>(A, wg, [&](unsigned it) { an_sq_dsum_body(A, it); });
}
__global__ __launch_bounds__(256) void anb_sq_prefix_kernel(AN_BATCH_PARAMS) {
    unsigned it;
    const AnalysisArgs &A = an_clip(clips, pre, n_clips, kAnlSq1, it);
    an_sq_prefix_body(A);
}
__global__ __launch_bounds__(64) void anb_sq_terms_kernel(AN_BATCH_PARAMS) {
    unsigned wg;
    const AnalysisArgs &A = an_clip(clips, pre, n_clips, kAnlSqChunk, wg);
    an_items<kAnlSqChunk>(A, wg, [&](unsigned it) { an_sq_terms_body(A, it); });
}
__global__ __launch_bounds__(64) void anb_sq_chain_kernel(AN_BATCH_PARAMS) {
    unsigned it;
    const AnalysisArgs &A = an_clip(clips, pre, n_clips, kAnlSq1, it);
    an_sq_chain_body(A);
}
__global__ __launch_bounds__(64) void anb_sumsq_kernel(AN_BATCH_PARAMS) {
    unsigned it;
    const AnalysisArgs &A = an_clip(clips, pre, n_clips, kAnlSumsq, it);
    an_sumsq_body(A, it);
}
__global__ __launch_bounds__(128) void anb_blake3_chunks_kernel(AN_BATCH_PARAMS) {
    unsigned wg;
    const AnalysisArgs &A = an_clip(clips, pre, n_clips, kAnlB3, wg);
    an_items<kAnlB3>(A, wg, [&](unsigned it) { an_blake3_chunks_body(A, (unsigned long long)it * 128 + threadIdx.x); });
}
__global__ __launch_bounds__(256) void anb_blake3_tree_kernel(AN_BATCH_PARAMS) {
    unsigned it;
    const AnalysisArgs &A = an_clip(clips, pre, n_clips, kAnlClip, it);
    an_blake3_tree_body(A);
    // the root next to the clip's other results (the thread that wrote it behind the two buffers reads it back)
    if (threadIdx.x < 8) A.root[threadIdx.x] = A.cvs[2 * A.n_chunks * 8 + threadIdx.x];
}
__global__ __launch_bounds__(128) void anb_fft_kernel(AN_BATCH_PARAMS) {
    unsigned it;
    const AnalysisArgs &A = an_clip(clips, pre, n_clips, kAnlFft, it);
    an_fft_body(A, it);
}

// The energy of every 400 ms block, summed over the channels and divided by the block's length: what the per-clip path
// does on the host from the read-back partial sums (flo_api.cpp, analyze_impl), with the same additions in the same
// order - a quantum is 0.0 plus the segments' shares in segment order, a block 0.0 plus its four quanta, the clip's
// energy 0.0 plus (part[0] + part[1]) / len over the channels. Adds and one division, nothing to fuse: bit for bit.
__global__ __launch_bounds__(64) void anb_block_energy_kernel(AN_BATCH_PARAMS) {
    unsigned it;
    const AnalysisArgs &A = an_clip(clips, pre, n_clips, kAnlClip, it);
    const unsigned ch = A.channels, hop = A.hop;
    const unsigned long long frames = A.n / ch, L = A.kseg_frames;
    const unsigned long long nq = hop ? (frames + hop - 1) / hop : 0;
    // Warm-up segments (the host's rule, analyze_impl): the first segment of a channel that wrote a share that is not finite
    // - a sample that is not finite, a filter that has overflowed: the sequential recurrence never recovers - makes every
    // share a later segment wrote NaN (those restarted their filters from zero and forgot it).
    __shared__ unsigned first_bad[256];   // per channel (channels is a byte); ~0u: none
    const bool warm = !A.fast && A.n_seg > 1;   // (uniform)
    if (warm) {
        for (unsigned cc = 0; cc < ch; cc++) {
            unsigned first = 0xFFFFFFFFu;
            const double *pc = A.block_part + (unsigned long long)cc * A.n_blocks * 2;
            for (unsigned k = threadIdx.x; k < A.n_blocks; k += 64)
                for (unsigned slot = 0; slot < 2; slot++) {
                    const double v = pc[2ull * k + slot];
                    const unsigned sg = (unsigned)((unsigned long long)k * hop / A.seg_frames) + slot;
                    if (!(fabs(v) <= 1.7976931348623157e308) && sg < first) first = sg;
                }
            for (int o = 32; o; o >>= 1) {
                const unsigned other = (unsigned)__shfl_xor((int)first, o);
                first = other < first ? other : first;
            }
            if (threadIdx.x == 0) first_bad[cc] = first;
        }
        __syncthreads();
    }
    for (unsigned k = threadIdx.x; k < A.n_blocks; k += 64) {
        const unsigned long long start = (unsigned long long)k * hop;
        const unsigned long long end = start + 4ull * hop < frames ? start + 4ull * hop : frames;
        double e = 0.0;
        for (unsigned cc = 0; cc < ch; cc++) {
            double p0, p1;
            if (A.fast) {
                double blk = 0.0;
                for (unsigned long long q = k; q < (unsigned long long)k + 4 && q < nq; q++) {
                    // the segments that overlap quantum q's frames [q hop, (q + 1) hop), in order (all start inside the clip)
                    const unsigned long long qf0 = q * hop, qf1 = (q + 1) * hop < frames ? (q + 1) * hop : frames;
                    double quantum = 0.0;
                    for (unsigned long long sg = qf0 / L; sg * L < qf1; sg++)
                        quantum += A.kqpart[((unsigned long long)cc * A.n_kseg + sg) * A.kq + (q - sg * L / hop)];
                    blk += quantum;
                }
                p0 = blk;
                p1 = 0.0;
            } else {
                const double *pp = A.block_part + ((unsigned long long)cc * A.n_blocks + k) * 2;
                p0 = pp[0];
                p1 = pp[1];
                if (warm && first_bad[cc] != 0xFFFFFFFFu) {
                    const unsigned long long behind = (first_bad[cc] + 1ull) * A.seg_frames;   // the first frame of the segments that forgot
                    const double nan = __longlong_as_double(0x7FF8000000000000ll);
                    if (end > behind) {
                        if (start >= behind) p0 = nan;
                        else p1 = nan;
                    }
                }
            }
            e += (p0 + p1) / (double)(end - start);
        }
        A.block_energy[k] = e;
    }
}

int launch_analysis_batch(const AnBatchArgs &G, const unsigned long long (&total)[kAnlCount], hipStream_t s, const AnalysisSide *side) {
    // the chains and streams of launch_analysis: s0 peaks of the waveform + K-weighting + block energies; s1 true / sample
    // peak; s2 sum of squares; s3 BLAKE3 + spectrum
    if (!G.n_clips || !total[kAnlClip]) return 0;
    hipStream_t s1 = s, s2 = s, s3 = s;
    if (side) {
        if (hipEventRecord(side->fork, s) != hipSuccess) return -1;
        for (int i = 0; i < 3; i++)
            if (hipStreamWaitEvent(side->st[i], side->fork, 0) != hipSuccess || stream_delay(side->st[i]) != hipSuccess) return -1;
        s1 = side->st[0], s2 = side->st[1], s3 = side->st[2];
    }
    auto grid = [&](int L) { return dim3((unsigned)total[L]); };
    if (total[kAnlPeaks]) {
        hipLaunchKernelGGL(anb_peaks_kernel, grid(kAnlPeaks), dim3(64), 0, s, G.clips, G.pre, G.n_clips);
        AN_LAUNCH_CHECK();
    }
    if (total[kAnlLoud]) {
        hipLaunchKernelGGL(anb_loud_kernel, grid(kAnlLoud), dim3(128), 0, s, G.clips, G.pre, G.n_clips);
        AN_LAUNCH_CHECK();
    }
    if (total[kAnlKw]) {
        hipLaunchKernelGGL(anb_kw_pass_kernel<1>, grid(kAnlKw), dim3(64), 0, s, G.clips, G.pre, G.n_clips);
        AN_LAUNCH_CHECK();
        hipLaunchKernelGGL(anb_kw_scan_kernel<false>, grid(kAnlKScan), dim3(64), 0, s, G.clips, G.pre, G.n_clips);
        AN_LAUNCH_CHECK();
        hipLaunchKernelGGL(anb_kw_pass_kernel<3>, grid(kAnlKw), dim3(64), 0, s, G.clips, G.pre, G.n_clips);
        AN_LAUNCH_CHECK();
        hipLaunchKernelGGL(anb_kw_scan_kernel<true>, grid(kAnlKScan), dim3(64), 0, s, G.clips, G.pre, G.n_clips);
        AN_LAUNCH_CHECK();
        hipLaunchKernelGGL(anb_kw_pass_kernel<2>, grid(kAnlKw), dim3(64), 0, s, G.clips, G.pre, G.n_clips);
        AN_LAUNCH_CHECK();
        hipLaunchKernelGGL(anb_peak_kernel, grid(kAnlTile), dim3(256), 0, s1, G.clips, G.pre, G.n_clips);
        AN_LAUNCH_CHECK();
        hipLaunchKernelGGL(anb_peak_reduce_kernel, grid(kAnlFast1), dim3(256), 0, s1, G.clips, G.pre, G.n_clips);
        AN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(anb_block_energy_kernel, grid(kAnlClip), dim3(64), 0, s, G.clips, G.pre, G.n_clips);
    AN_LAUNCH_CHECK();
    if (total[kAnlSqChunk]) {
        hipLaunchKernelGGL(anb_sq_dsum_kernel, grid(kAnlSqChunk), dim3(64), 0, s2, G.clips, G.pre, G.n_clips);
        AN_LAUNCH_CHECK();
        hipLaunchKernelGGL(anb_sq_prefix_kernel, grid(kAnlSq1), dim3(256), 0, s2, G.clips, G.pre, G.n_clips);
        AN_LAUNCH_CHECK();
        hipLaunchKernelGGL(anb_sq_terms_kernel, grid(kAnlSqChunk), dim3(64), 0, s2, G.clips, G.pre, G.n_clips);
        AN_LAUNCH_CHECK();
        hipLaunchKernelGGL(anb_sq_chain_kernel, grid(kAnlSq1), dim3(64), 0, s2, G.clips, G.pre, G.n_clips);
        AN_LAUNCH_CHECK();
    }
    if (total[kAnlSumsq]) {
        hipLaunchKernelGGL(anb_sumsq_kernel, grid(kAnlSumsq), dim3(64), 0, s2, G.clips, G.pre, G.n_clips);
        AN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(anb_blake3_chunks_kernel, grid(kAnlB3), dim3(128), 0, s3, G.clips, G.pre, G.n_clips);
    AN_LAUNCH_CHECK();
    hipLaunchKernelGGL(anb_blake3_tree_kernel, grid(kAnlClip), dim3(256), 0, s3, G.clips, G.pre, G.n_clips);
    AN_LAUNCH_CHECK();
    hipLaunchKernelGGL(anb_fft_kernel, grid(kAnlFft), dim3(128), 0, s3, G.clips, G.pre, G.n_clips);
    AN_LAUNCH_CHECK();
    if (side)
        for (int i = 0; i < 3; i++)
            if (hipEventRecord(side->join[i], side->st[i]) != hipSuccess || hipStreamWaitEvent(s, side->join[i], 0) != hipSuccess) return -1;
    if (side && stream_delay(s) != hipSuccess) return -1;   // behind the joins (flo_debug_stream_delay)
    return 0;
}

}  // namespace flo
