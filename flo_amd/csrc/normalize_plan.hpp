// normalize_plan.hpp — loudness normalisation and true-peak limiting (flo_batch_normalize, flo_normalize, flo_batch_true_peak,
// flo_normalize_gain; normalize.cpp, normalize_kernels.hip): the gain of a clip from its measurements, the look-ahead, the
// skip bound and the tile geometry. Plain C++: no HIP headers, so a host test builds it with g++ alone
// (tests/native/normalize_plan_test.cpp); the geometry is inline here because the kernel uses the same functions.
//
// The measure: h = the 1 -> 4 interpolator of the sample-rate conversion (resample_plan: L = 4, M = 1, 64 taps),
// e_q[n, c] = the FMA chain over k = 0 .. 63 of h[q][k] * y[n + k - 31, c] from 0, y zero outside the clip, and
// p[n] = max over c of max(|y[n, c]|, max_q |e_q[n, c]|). The limiter, A = look-ahead frames, C = the ceiling, all channels
// linked: r[n] = 2^24 where p[n] <= C, else (uint32)((C / p[n]) * 2^24) (r outside the clip is 2^24);
// m[k] = min r[k - A .. k + A]; S[n] = sum m[n - A .. n + A]; s[n] = S[n] div (2A + 1); z[n, c] = y[n, c] * ((float)s[n] * 2^-24).
//
// Geometry: a tile is F = norm_tile_frames(A) consecutive frames of one clip from a multiple of F on. Its s needs m over
// F + 2A frames, r and p over F + 4A, y over F + 4A + 63: one channel of that span is staged at a time (so the geometry
// does not depend on the channel count), p is gathered in a second plane of the same size, and the sliding stages
// ping-pong between the two planes.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/flo_hip.h"

#if defined(__HIPCC__)
#define FLO_NP_HD __host__ __device__ inline
#else
#define FLO_NP_HD inline
#endif

namespace flo {

constexpr uint32_t kNormMaxLookahead = 1024;
constexpr uint32_t kNormThreads = 512;
constexpr uint32_t kNormPhases = 4, kNormTaps = 64, kNormBefore = 31, kNormAfter = 32;   // taps reach n - 31 .. n + 32
constexpr uint32_t kNormUnity = 1u << 24;
constexpr uint32_t kNormMinTile = 2048;
constexpr uint32_t kNormLdsBytes = 100 * 1024;   // one workgroup of 8 waves per CU at the longest look-ahead
// LIMIT mode keeps true_peak * g at or below this, so that no sample, partial sum or envelope value overflows
constexpr double kNormMaxScaledPeak = 0x1p100;
// GAIN mode keeps true_peak * g at or below C times this, so that the OUTPUT's own true peak stays at or below C: y is within
// 2^-24 relative of x * g, and the chain over x and the chain over y are each within 2^-18 of sum |h x|, which is at most
// 2.2525 true_peak: the output's peak is at most true_peak * g * (1 + 2.2525 * (2^-17 + 2^-23))
constexpr double kNormGainMargin = 1.0 - 0x1p-15;

// frames of one tile: at least eight look-aheads, so that the halo of 4A frames costs at most half as much again
FLO_NP_HD uint32_t norm_tile_frames(uint32_t A) { return 8 * A > kNormMinTile ? 8 * A : kNormMinTile; }
// elements of r (and p), of m, and frames of y a tile holds
FLO_NP_HD uint32_t norm_r_len(uint32_t A) { return norm_tile_frames(A) + 4 * A; }
FLO_NP_HD uint32_t norm_m_len(uint32_t A) { return norm_tile_frames(A) + 2 * A; }
FLO_NP_HD uint32_t norm_span(uint32_t A) { return norm_r_len(A) + kNormTaps - 1; }
// two planes of norm_span elements of 4 bytes
FLO_NP_HD uint32_t norm_lds_bytes(uint32_t A) { return 2 * 4 * norm_span(A); }
// the clip's frame behind staged frame 0, behind r[0] and behind m[0] of tile t
FLO_NP_HD long long norm_y0(unsigned long long t, uint32_t A) {
    return (long long)(t * norm_tile_frames(A)) - 2 * (long long)A - (long long)kNormBefore;
}
FLO_NP_HD long long norm_r0(unsigned long long t, uint32_t A) { return (long long)(t * norm_tile_frames(A)) - 2 * (long long)A; }
FLO_NP_HD long long norm_m0(unsigned long long t, uint32_t A) { return (long long)(t * norm_tile_frames(A)) - (long long)A; }
// the sliding minimum over 2A + 1 elements by doubling: the largest power of two at or below the window
FLO_NP_HD uint32_t norm_min_pow2(uint32_t A) {
    uint32_t p = 1;
    while (2 * p <= 2 * A + 1) p *= 2;
    return p;
}
// consecutive elements of m one thread sums in the block-wide prefix sum (odd: its lanes then fall on different LDS banks)
FLO_NP_HD uint32_t norm_scan_chunk(uint32_t A) { return ((norm_m_len(A) + kNormThreads - 1) / kNormThreads) | 1u; }

// 0 .. kNormMaxLookahead frames asked for at `rate`: 0 means max(1, round(0.0015 * rate)); false with a message that names
// the quantity
bool normalize_lookahead(uint32_t rate, uint32_t asked, uint32_t &frames, std::string &err);
// the options with NULL meaning the defaults, checked; false with a message that names the quantity
bool normalize_opts(const flo_normalize_opts *in, flo_normalize_opts &out, std::string &err);
// C = (float)10^(ceiling / 20)
float normalize_ceiling(const flo_normalize_opts &o);
// The gain of one clip (o: checked options): the report's input fields, gain, gain_db, ceiling_reduction_db and status. A
// clip with a status is copied (gain 1).
void normalize_gain(double integrated_lufs, double sample_peak_dbfs, float true_peak, const flo_normalize_opts &o, flo_normalize_report &rep);
// h[4][64] of the 1 -> 4 interpolator, and the skip bound B: no |e_q[n, c]| and no |y[n, c]| exceeds B * max |y| over the
// taps' reach (the largest row l1 norm of h times 1 + 2^-16, rounded up: the chain's rounding stays below 2^-17 relative
// to sum |h y|, the rounding of the product B * max |y| below 2^-23)
std::vector<float> normalize_table();
float normalize_skip_bound(const std::vector<float> &h);
// (the flat work list of a launch: clip_tiles of every clip's frames in tiles of norm_tile_frames(A), clip_tiles.hpp)

}  // namespace flo
