// analysis_kernels.hip — gfx950 kernels behind flo_analysis_metadata (see analysis_kernels.hpp).
//
// Reference behaviour replaced (files under /root/reference/libflo/src):
//   extract_waveform_peaks ............. core/analysis.rs:38-115      an_peaks_kernel (one wave per peak window)
//   extract_spectral_fingerprint ....... core/analysis.rs:223-357     an_blake3_chunks / an_blake3_tree (the hash; BLAKE3
//                                        is a tree of 1 KiB chunks, so chunks hash in parallel), an_fft_kernel (the three
//                                        256-point sections), the f32 sum of squares in an_sumsq_kernel
//   compute_ebu_r128_loudness .......... core/ebu_r128.rs:112-266      an_loud_kernel: K-weighting (two biquads, f64), the
//                                        400 ms block sums, the sample peak and the true-peak FIR
// Everything the reference accumulates sequentially is accumulated in the same order here (the sums feed truncating
// casts to u8 and an f32 cast of the loudness, so the order matters for byte equality) - exactly so for clips up to one
// segment (65 536 frames; 65 536 interleaved samples for the sum of squares), in segments with a filter warm-up beyond (see "order-bound scans" below); only order-free work
// (maxima, the hash tree, butterflies, the FIR outputs) is spread over lanes. Compiled with -ffp-contract=off.
#include "analysis_device.hpp"
#include "stream_delay.hpp"

namespace flo {

#define AN_LAUNCH_CHECK()                      \
    do {                                       \
        hipError_t e_ = hipGetLastError();     \
        if (e_ != hipSuccess) return (int)e_;  \
    } while (0)

// ------------------------------------------------------------------------------------------------ kernels (one clip)
// (the bodies, their reasoning and the reference lines they restate: analysis_device.hpp)
__global__ __launch_bounds__(64) void an_peaks_kernel(AnalysisArgs A) { an_peaks_body(A, blockIdx.x); }
__global__ __launch_bounds__(128) void an_loud_kernel(AnalysisArgs A) { an_loud_body(A, blockIdx.x, blockIdx.y); }
template <int PASS>
__global__ __launch_bounds__(64) void an_kw_pass_kernel(AnalysisArgs A) { an_kw_pass_body<PASS>(A, blockIdx.x, blockIdx.y); }
template <bool REFINE>
__global__ __launch_bounds__(64) void an_kw_scan_kernel(AnalysisArgs A) { an_kw_scan_body<REFINE>(A, blockIdx.x); }
__global__ __launch_bounds__(256) void an_peak_kernel(AnalysisArgs A) { an_peak_body(A, blockIdx.x, blockIdx.y, gridDim.x); }
__global__ __launch_bounds__(256) void an_peak_reduce_kernel(AnalysisArgs A, unsigned long long n_part) { an_peak_reduce_body(A, n_part); }
__global__ __launch_bounds__(64) void an_sq_dsum_kernel(AnalysisArgs A) { an_sq_dsum_body(A, blockIdx.x); }
__global__ __launch_bounds__(256) void an_sq_prefix_kernel(AnalysisArgs A) { an_sq_prefix_body(A); }
__global__ __launch_bounds__(64) void an_sq_terms_kernel(AnalysisArgs A) { an_sq_terms_body(A, blockIdx.x); }
__global__ __launch_bounds__(64) void an_sq_chain_kernel(AnalysisArgs A) { an_sq_chain_body(A); }
__global__ __launch_bounds__(64) void an_sumsq_kernel(AnalysisArgs A) { an_sumsq_body(A, blockIdx.x); }
__global__ void an_blake3_chunks_kernel(AnalysisArgs A) { an_blake3_chunks_body(A, (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x); }
__global__ __launch_bounds__(256) void an_blake3_tree_kernel(AnalysisArgs A) { an_blake3_tree_body(A); }
__global__ __launch_bounds__(128) void an_fft_kernel(AnalysisArgs A) { an_fft_body(A, blockIdx.x); }

int launch_analysis(const AnalysisArgs &A, hipStream_t s, const AnalysisSide *side) {
    // s0: peaks of the waveform + K-weighting; s1: true / sample peak; s2: sum of squares; s3: BLAKE3 + spectrum
    hipStream_t s1 = s, s2 = s, s3 = s;
    if (side && A.n) {
        if (hipEventRecord(side->fork, s) != hipSuccess) return -1;
        for (int i = 0; i < 3; i++)
            if (hipStreamWaitEvent(side->st[i], side->fork, 0) != hipSuccess || stream_delay(side->st[i]) != hipSuccess) return -1;
        s1 = side->st[0], s2 = side->st[1], s3 = side->st[2];
    }
    if (A.n_peaks) {
        hipLaunchKernelGGL(an_peaks_kernel, dim3(A.n_peaks), dim3(64), 0, s, A);
        AN_LAUNCH_CHECK();
    }
    if (A.n) {
        if (A.fast) {
            hipLaunchKernelGGL(an_kw_pass_kernel<1>, dim3((A.n_kseg + 63) / 64, A.channels), dim3(64), 0, s, A);
            AN_LAUNCH_CHECK();
            hipLaunchKernelGGL(an_kw_scan_kernel<false>, dim3(A.channels), dim3(64), 0, s, A);
            AN_LAUNCH_CHECK();
            // one refinement of the start states (an_kw_scan_body)
            hipLaunchKernelGGL(an_kw_pass_kernel<3>, dim3((A.n_kseg + 63) / 64, A.channels), dim3(64), 0, s, A);
            AN_LAUNCH_CHECK();
            hipLaunchKernelGGL(an_kw_scan_kernel<true>, dim3(A.channels), dim3(64), 0, s, A);
            AN_LAUNCH_CHECK();
            hipLaunchKernelGGL(an_kw_pass_kernel<2>, dim3((A.n_kseg + 63) / 64, A.channels), dim3(64), 0, s, A);
            AN_LAUNCH_CHECK();
            const unsigned long long longest = (A.n + A.channels - 1) / A.channels;
            const unsigned tiles = (unsigned)((longest + kAnTile - 1) / kAnTile);
            hipLaunchKernelGGL(an_peak_kernel, dim3(tiles, A.channels), dim3(256), 0, s1, A);
            AN_LAUNCH_CHECK();
            hipLaunchKernelGGL(an_peak_reduce_kernel, dim3(1), dim3(256), 0, s1, A, (unsigned long long)tiles * A.channels);
            AN_LAUNCH_CHECK();
        } else {
            hipLaunchKernelGGL(an_loud_kernel, dim3(A.n_seg, A.channels), dim3(128), 0, s, A);
            AN_LAUNCH_CHECK();
        }
        if (A.sq_exact) {
            hipLaunchKernelGGL(an_sq_dsum_kernel, dim3((unsigned)A.n_sq_chunks), dim3(64), 0, s2, A);
            AN_LAUNCH_CHECK();
            hipLaunchKernelGGL(an_sq_prefix_kernel, dim3(1), dim3(256), 0, s2, A);
            AN_LAUNCH_CHECK();
            hipLaunchKernelGGL(an_sq_terms_kernel, dim3((unsigned)A.n_sq_chunks), dim3(64), 0, s2, A);
            AN_LAUNCH_CHECK();
            hipLaunchKernelGGL(an_sq_chain_kernel, dim3(1), dim3(64), 0, s2, A);
            AN_LAUNCH_CHECK();
        } else {
            hipLaunchKernelGGL(an_sumsq_kernel, dim3(A.n_sq_seg), dim3(64), 0, s2, A);
            AN_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(an_blake3_chunks_kernel, dim3((unsigned)((A.n_chunks + 127) / 128)), dim3(128), 0, s3, A);
        AN_LAUNCH_CHECK();
        hipLaunchKernelGGL(an_blake3_tree_kernel, dim3(1), dim3(256), 0, s3, A);
        AN_LAUNCH_CHECK();
        hipLaunchKernelGGL(an_fft_kernel, dim3(3), dim3(128), 0, s3, A);
        AN_LAUNCH_CHECK();
    }
    if (side && A.n)
        for (int i = 0; i < 3; i++)
            if (hipEventRecord(side->join[i], side->st[i]) != hipSuccess || hipStreamWaitEvent(s, side->join[i], 0) != hipSuccess) return -1;
    if (side && A.n && stream_delay(s) != hipSuccess) return -1;   // behind the joins (flo_debug_stream_delay)
    return 0;
}

}  // namespace flo
