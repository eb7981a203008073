// resample_plan.hpp — sample-rate conversion (flo_batch_resample, flo_resample; resample.cpp, resample_kernels.hip): the
// filter of a rate pair, the index arithmetic that places every output, and the launch geometry. Plain C++: no HIP headers,
// so a host test builds it with g++ alone (tests/native/resample_plan_test.cpp); the index arithmetic and the LDS
// addressing are inline here because the kernel uses the same functions.
//
// in_rate -> out_rate, g = gcd: L = out_rate / g phases, M = in_rate / g. Output frame j of a clip sits at input time
// j * M / L: i = floor(j * M / L), p = (j * M) mod L, and y[j] = sum_k h[p][k] * x[i + k - T/2 + 1] (x zero outside the
// clip), k = 0 .. T - 1 in that order. With c = min(1, L / M) and W = 32 / c, T = 2 * ceil(W), and before normalisation
// h[p][k] = rho c sinc(rho c d) I0(beta sqrt(1 - (d/W)^2)) / I0(beta) for |d| <= W, d = (k - T/2 + 1) - p / L, rho = 0.91,
// beta = 9; every row is divided by its own sum in f64, then rounded to f32.
//
// Geometry (phase-stationary): a tile is Q * L consecutive outputs starting at a multiple of L, output q * L + r of it
// (slot q, phase index r) has the coefficient row p_r = (r * M) mod L and reads the tile's staged input from frame
// q * M + floor(r * M / L) on. A wave takes one r for 64 slots at a time, so its coefficients are wave-uniform (scalar
// loads) and only x comes from LDS, the lanes M frames apart; a lane makes kResampleBlock consecutive r from each x it
// reads. Where 64 slots of input do not fit the LDS budget, a tile
// has fewer slots and a wave takes 64 / Q phases side by side (coefficients then come through vector loads).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define FLO_RS_HD __host__ __device__ inline
#else
#define FLO_RS_HD inline
#endif

namespace flo {

constexpr uint32_t kResampleMaxRate = 384000, kResampleMaxPhases = 1024, kResampleMaxTaps = 2048;
constexpr uint32_t kResampleMaxTableBytes = 1u << 20;
constexpr double kResampleRho = 0.91, kResampleBeta = 9.0, kResampleZeroCrossings = 32.0;
// Workgroups of the kernel and the LDS one of them may hold: two workgroups of 8 waves share a CU's 160 KiB, four waves per
// SIMD. A tile is sized at 8 bytes per staged frame (one float2 plane, or two float planes) whatever the channel count:
// clips of more channels go through the tile's LDS two channels at a time, so the geometry depends on the rates alone.
constexpr uint32_t kResampleThreads = 512, kResampleLdsBytes = 80 * 1024, kResampleFrameBytes = 8;
// phases of work a tile should hold for every 64 slots at least, where the LDS budget allows
constexpr uint32_t kResampleTargetUnits = 128;
// With one phase per wave a lane makes this many consecutive outputs r, r + 1, ... of its slot in one pass: their windows
// start floor(M / L) or one more frame apart, so every x it reads from LDS feeds that many accumulators.
constexpr uint32_t kResampleBlock = 4;

// Where output frame j lies: i = floor(j * M / L), p = (j * M) mod L. u64 throughout: j < 2^44, M < 2^19.
FLO_RS_HD void resample_pos(uint64_t j, uint32_t L, uint32_t M, uint64_t &i, uint32_t &p) {
    const uint64_t t = j * (uint64_t)M;
    i = t / L;
    p = (uint32_t)(t % L);
}
// The LDS element of staged frame f (f counts from the tile's first staged frame). Lanes read M frames apart: an even M
// would put them on few banks, so frame f is moved up by f >> ctz(M) and the lanes' stride becomes M + (M >> ctz(M)), which
// is odd. shift is 31 for an odd M (nothing moves: f < 2^31).
FLO_RS_HD uint32_t resample_lds_index(uint32_t f, uint32_t shift) { return f + (f >> shift); }

// Which outputs of its tile a lane makes in wave-unit `unit`: slot q, phase indices r .. r + block - 1 as far as they stay
// below L (outputs q * L + r ... of the tile), or none. A unit is one 64-slot piece of `block` consecutive phases
// (phases_per_wave = 1: r is the same in every active lane), or phases_per_wave phases of lanes_per_phase = Q slots each,
// side by side (block = 1).
struct ResampleLane {
    uint32_t q, r;
    bool active;
};
FLO_RS_HD ResampleLane resample_lane(uint32_t unit, uint32_t lane, uint32_t L, uint32_t slots, uint32_t lanes_per_phase,
                                     uint32_t phases_per_wave, uint32_t chunks, uint32_t block) {
    const uint32_t grp = lane / lanes_per_phase, ql = lane - grp * lanes_per_phase;
    const uint32_t rb = unit / chunks, chunk = unit - rb * chunks;
    ResampleLane o;
    o.r = (rb * phases_per_wave + grp) * block;
    o.q = chunk * 64 + ql;
    o.active = grp < phases_per_wave && o.r < L && o.q < slots;
    return o;
}
// Output q * L + r of a tile: its coefficient row p and the staged frame e0 + q * M its first tap reads (r < 1024, M <= 384000)
FLO_RS_HD void resample_phase(uint32_t r, uint32_t L, uint32_t M, uint32_t &e0, uint32_t &p) {
    const uint32_t rm = r * M;
    e0 = rm / L;
    p = rm - e0 * L;
}

struct ResamplePlan {
    uint32_t in_rate = 0, out_rate = 0;
    uint32_t L = 1, M = 1, taps = 0;
    double W = 0, cutoff = 1;          // W = 32 / c, c = min(1, L / M)
    // geometry
    uint32_t slots = 0;                // Q
    uint32_t tile_outputs = 0;         // Q * L
    uint32_t lanes_per_phase = 0;      // min(Q, 64)
    uint32_t phases_per_wave = 0;      // 64 / lanes_per_phase: 1 = wave-uniform coefficients
    uint32_t chunks = 0;               // ceil(Q / 64): 64-slot pieces of one phase
    uint32_t block = 1;                // consecutive phases a lane makes from one pass over its x (kResampleBlock, or 1)
    uint32_t units = 0;                // wave-units of a tile: chunks * ceil(L / (phases_per_wave * block))
    uint32_t shift = 31;               // resample_lds_index
    uint32_t span = 0;                 // frames a tile stages: from (tile * Q * M) - (T/2 - 1) on
    uint32_t lds_elems = 0;            // elements of one staged plane: resample_lds_index(span - 1) + 1
    bool identity() const { return L == 1 && M == 1; }
};

// frames a tile of q slots stages, and the LDS elements they take
uint32_t resample_span(uint32_t L, uint32_t M, uint32_t taps, uint32_t q);
// The plan of a rate pair; false with a message that names the offending quantity.
bool resample_plan(uint32_t in_rate, uint32_t out_rate, ResamplePlan &out, std::string &err);
// h[L][taps], f32
std::vector<float> resample_table(const ResamplePlan &p);
// ceil(n_in * L / M); false when it does not fit 2^63
bool resample_out_frames(const ResamplePlan &p, uint64_t n_in, uint64_t &n_out);
// channels a tile stages at a time (1, or 2) and the dynamic LDS that takes
uint32_t resample_pass_channels(uint32_t channels);
uint32_t resample_lds_bytes(const ResamplePlan &p, uint32_t channels);
// (the flat work list of a launch: clip_tiles of every clip's n_out in tiles of tile_outputs, clip_tiles.hpp)

}  // namespace flo
