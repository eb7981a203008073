// analysis_plan.hpp — the geometry of one clip's analysis: everything flo_analyze and flo_batch_analyze_all (analysis.cpp)
// decide from (samples, sample rate, channels, peaks per second) alone, before a buffer exists - the peak windows, the
// K-weighting and true-peak coefficients, the block, segment, tile and chunk counts and which path each scan takes - and
// the items of the batched path's work lists. No HIP in here: the host test builds it with g++ alone
// (tests/native/analysis_plan_test.cpp), and the kernels' AnalysisArgs (analysis_kernels.hpp) is filled from it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define FLO_PLAN_HD __host__ __device__
#else
#define FLO_PLAN_HD
#endif

namespace flo {

struct AnalysisPlan {
    unsigned long long n = 0;    // interleaved samples
    unsigned int sample_rate = 0, channels = 0;
    double samples_per_peak = 0;
    unsigned int n_peaks = 0;
    double shelf[5] = {}, hp[5] = {};   // b0 b1 b2 a1 a2
    unsigned int hop = 0, n_blocks = 0;
    unsigned int seg_frames = 0, warm_frames = 0, n_seg = 0;
    unsigned int sq_seg = 0, n_sq_seg = 0;
    unsigned int fast = 0;
    unsigned int kseg_frames = 0, n_kseg = 0, kq = 0;
    double kpow[16] = {};
    unsigned int sq_exact = 0;
    unsigned long long n_sq_chunks = 0;
    double tp_coef[49] = {};
    unsigned long long n_chunks = 0;
    unsigned long long points[3] = {};
    unsigned int point_ok[3] = {};
};

// K-weighting of a clip beyond one exact segment: two passes over short segments with the filter state handed over
// exactly (analysis_kernels.hip, "K-weighting, long clips"); FLO_ANALYSIS_EXACT=1 keeps the one-lane walk (diagnostic)
bool analysis_fast_path(uint64_t frames, unsigned hop, unsigned ch);
// a clip's geometry: everything launch_analysis needs but its buffers, for the per-clip and the batched path alike
// (block_len: the lengths of the 400 ms blocks, when asked for). Nothing but n_peaks for an empty clip, or when
// peaks_only. `like`: a clip of the same rate whose geometry is made - its filter coefficients (and its M^L, for the same
// segment length) are copied rather than computed again (the same values: the batched path's clips share one rate).
void analysis_plan(AnalysisPlan &A, size_t n, uint32_t sr, uint8_t ch, uint32_t pps, std::vector<uint64_t> *block_len_out,
                   bool peaks_only = false, const AnalysisPlan *like = nullptr);

// ------------------------------------------------------------------------------------------------ batched analysis
constexpr int kAnTile = 2048;   // frames per tile (an_loud, an_peak)
enum AnList : int {
    kAnlPeaks,     // n_peaks: one wave per peak window
    kAnlLoud,      // clips of at most one exact segment: n_seg x channels
    kAnlKw,        // longer clips: ceil(n_kseg / 64) x channels (K-weighting passes 1 and 2)
    kAnlKScan,     // longer clips: channels
    kAnlTile,      // longer clips: true / sample peak tiles x channels
    kAnlFast1,     // longer clips: 1 (peak reduce)
    kAnlSqChunk,   // sum of squares beyond one segment: n_sq_chunks
    kAnlSq1,       // sum of squares beyond one segment: 1 (prefix, chain)
    kAnlSumsq,     // sum of squares within one segment: n_sq_seg
    kAnlB3,        // BLAKE3 chunks: ceil(n_chunks / 128)
    kAnlClip,      // every clip with samples: 1 (hash tree, block energies)
    kAnlFft,       // every clip with samples: 3
    kAnlCount
};
// items of every list for one clip (host and device agree on the geometry through this one function; G: the plan, or the
// kernels' AnalysisArgs filled from it)
template <class G>
FLO_PLAN_HD inline void an_batch_items(const G &A, unsigned long long (&it)[kAnlCount]) {
    for (int k = 0; k < kAnlCount; k++) it[k] = 0;
    if (!A.n) return;
    const unsigned long long ch = A.channels, longest = (A.n + ch - 1) / ch;
    it[kAnlPeaks] = A.n_peaks;
    if (A.fast) {
        it[kAnlKw] = (A.n_kseg + 63ull) / 64ull * ch;
        it[kAnlKScan] = ch;
        it[kAnlTile] = (longest + kAnTile - 1) / kAnTile * ch;
        it[kAnlFast1] = 1;
    } else {
        it[kAnlLoud] = (unsigned long long)A.n_seg * ch;
    }
    if (A.sq_exact) {
        it[kAnlSqChunk] = A.n_sq_chunks;
        it[kAnlSq1] = 1;
    } else {
        it[kAnlSumsq] = A.n_sq_seg;
    }
    it[kAnlB3] = (A.n_chunks + 127ull) / 128ull;
    it[kAnlClip] = 1;
    it[kAnlFft] = 3;
}
// items one workgroup takes in turn (one clip lookup for all of them); a list's prefix counts these workgroups
FLO_PLAN_HD constexpr unsigned an_batch_per_wg(int L) {
    return L == kAnlPeaks ? 8u : L == kAnlTile ? 4u : L == kAnlSqChunk ? 16u : L == kAnlB3 ? 4u : 1u;
}

}  // namespace flo
