// fftconv_plan.hpp — partitioned FFT convolution of resident batches (flo_batch_convolve_fft, flo_convolve_fft,
// flo_conv_fft_geometry; fftconv.cpp, fftconv_kernels.hip): the checks (conv_check with this path's limits), the
// deduplicated responses, every job's segments and blocks, the groups the scratch is cut into, the work lists of a group, the
// twiddle table and the geometry. Plain C++: no HIP headers, so a host test builds it with g++ alone
// (tests/native/fftconv_plan_test.cpp).
//
// The definition: B = kFcBlock, F = 2B, Pn = ceil(K / B). Partition p is taps [pB, min((p+1)B, K)) zero-padded
// to F; segment q of a job is source frames [(q-1)B + skip, (q+1)B + skip), +0.0 outside [0, N); block b is output frames
// [bB, (b+1)B): Y_b = sum over p ascending of X_{b-p} H_p from zero, and the last B values of irfft(Y_b) are the block.
//
// A spectrum of F real points is stored as B complex f32: bin 0 holds (DC, Nyquist), both real; bins 1 .. B-1 as they are.
// Scratch, in complex elements: segments [entry][segment][channel][bin], responses [response][p][channel][bin].
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "conv_plan.hpp"

#ifndef FLO_FFTCONV_BLOCK
#define FLO_FFTCONV_BLOCK 512
#endif
#ifndef FLO_FFTCONV_LANE_BLOCKS
#define FLO_FFTCONV_LANE_BLOCKS 8
#endif

namespace flo {

constexpr uint32_t kFcThreads = 256;
constexpr uint32_t kFcBlock = FLO_FFTCONV_BLOCK;                  // B: one per build
constexpr uint32_t kFcLaneBlocks = FLO_FFTCONV_LANE_BLOCKS;       // output blocks a lane accumulates side by side
constexpr uint32_t kFcTileFrames = kFcBlock * kFcLaneBlocks;      // a tile of the multiply stage's work list
constexpr uint32_t kFcBinsPerLane = kFcBlock / kFcThreads;        // a lane owns bins tid + i * kFcThreads
// transforms a workgroup runs side by side: a transform of B complex points has B / 2 butterflies per stage
constexpr uint32_t kFcTogether = kFcBlock <= 512 ? 512 / kFcBlock : 1;
constexpr uint32_t kFcCrossoverTaps = 1024;                       // measured: DESIGN 4.19
constexpr uint64_t kFcGroupBytes = (uint64_t)1 << 30;             // FLO_CONV_FFT_GROUP_BYTES' default
constexpr uint64_t kFcMaxGroups = 1024;                           // a smaller cap than the call's segments / this is raised to it
static_assert(kFcBlock == 256 || kFcBlock == 512 || kFcBlock == 1024, "B is 256, 512 or 1024");
static_assert(kFcLaneBlocks >= 1 && kFcLaneBlocks <= 16, "lane_blocks");

// One real signal cut into transforms, as the spectrum kernel reads it (64 bytes). Transform i covers samples
// [start + iB, start + iB + 2B) of every channel; of those the first `live` (B for a response: the rest is the padding;
// 2B for a source) are taken from the signal where they lie in [0, len), everything else is +0.0. The spectrum of
// (transform i, channel c) goes to complex element out + (i * channels + c) * B.
struct FcSpecJob {
    const float *base;          // sample 0, channel 0 (never read when len == 0)
    long long start;
    unsigned long long len;
    unsigned long long out;
    unsigned int channels;      // of the signal: its stride
    unsigned int live;
    unsigned int items;         // transforms * channels
    unsigned int unused[5];
};
static_assert(sizeof(FcSpecJob) == 64, "FcSpecJob is 64 bytes");

// One entry (a job's blocks [b0, b1) inside one group) as the multiply kernel reads it (64 bytes)
struct FcMacJob {
    unsigned long long x_off;     // complex elements: segment s0, channel 0
    unsigned long long h_off;     // complex elements: partition 0, response channel 0
    unsigned long long dst_off;   // floats: the output clip's first sample
    unsigned long long frames;    // T
    long long s0, s1;             // the segments stored for this entry: [s0, s1)
    unsigned long long b0;        // a multiple of kFcLaneBlocks
    unsigned int parts;           // Pn
    unsigned int ir_channels;     // Ch
};
static_assert(sizeof(FcMacJob) == 64, "FcMacJob is 64 bytes");

struct FcResponse {
    uint32_t ir = 0;            // clip of irs
    uint64_t ir_start = 0;      // below P unless taps == 0
    uint32_t taps = 0, parts = 0;   // K, Pn
    uint64_t h_off = 0;         // complex elements
};
struct FcJob {
    uint32_t taps = 0, parts = 0, response = 0;
    uint64_t skip = 0;          // conv_skip
    int64_t q_lo = 0, q_hi = 0; // segments that are not zero and that some block uses: [q_lo, q_hi)
    uint64_t blocks = 0;        // ceil(T / B)
};
struct FcEntry {
    uint32_t job = 0;
    uint64_t b0 = 0, b1 = 0;    // blocks; b0 a multiple of kFcLaneBlocks, b1 one too or the job's last
    int64_t s0 = 0, s1 = 0;     // segments stored: [max(q_lo, b0 - Pn + 1), min(q_hi, b1))
    uint64_t x_off = 0;         // complex elements inside the group's scratch
};
struct FcGroup {
    size_t first = 0, count = 0;   // entries
    uint64_t x_elems = 0;
};
struct FcPlan {
    uint32_t channels = 0, ir_channels = 0;
    std::vector<FcResponse> responses;
    std::vector<FcJob> jobs;
    std::vector<FcEntry> entries;
    std::vector<FcGroup> groups;
    uint64_t h_elems = 0;       // the responses' spectra
    uint64_t x_elems = 0;       // the largest group's segment spectra
};

inline uint32_t fftconv_parts(uint32_t K) { return K / kFcBlock + (K % kFcBlock != 0); }
// complex elements of one segment of every channel
inline uint64_t fftconv_segment_elems(uint32_t channels) { return (uint64_t)channels * kFcBlock; }

// The plan of one call, or false with a message that names the quantity. group_bytes caps a group's segment spectra; an
// entry is never smaller than one tile, whatever the cap, and the cap is never below 1 / kFcMaxGroups of the call's segments.
bool fftconv_plan(const ConvSource &src, const ConvSource &irs, size_t n_out, const flo_conv_job *jobs, uint64_t group_bytes, FcPlan &plan,
                  std::string &err);
// The two flat work lists of a group through clip_tiles: transforms of its entries' segments (kFcTogether items a tile) and
// block groups (kFcLaneBlocks blocks a tile); false when a launch cannot hold them.
bool fftconv_group_tiles(const FcPlan &plan, const FcGroup &g, std::vector<uint32_t> &pre_spec, std::vector<uint32_t> &pre_mac);
// ... and of the responses (Pn * Ch items each)
bool fftconv_response_tiles(const FcPlan &plan, std::vector<uint32_t> &pre);
// tw[2k], tw[2k + 1] = cos, -sin of 2 pi k / F for k < B: made in f64, rounded once
void fftconv_twiddles(std::vector<float> &tw);

}  // namespace flo
