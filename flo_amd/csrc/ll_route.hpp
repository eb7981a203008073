// ll_route.hpp — which kernels take a lossless channel wrapper, and the per-call wrapper list (see decode_plan.hpp, which
// adds what drives the device). Plain C++: no HIP headers, so a host test builds ll_route.cpp with g++ alone
// (tests/native/decode_plan_test.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace flo {

// One ALPC / raw / silent channel wrapper of one frame = one thread.
struct LlChannelDev {
    unsigned long long off;           // payload offset
    unsigned long long out_off;       // int32 offset of this channel-frame in the planar scratch
    unsigned int len;                 // payload bytes
    unsigned int samples;             // frame_samples
    unsigned char n_coeffs, shift_bits, rice_k, pad;
    int coeffs[12];
};

// Parallel form of the ALPC decode (lldec_kernels.hip). A Rice stream is cut into tiles of kRiceTileBits bits.
constexpr int kRiceTileBits = 1024;
constexpr int kRiceStates = 16;       // entry states of a tile: skip 0..k bits (k <= 14), or "inside a unary run" (k + 1)
constexpr int kRiceMaxK = kRiceStates - 2;

// Per frame: mid/side, interleave, int -> float.
struct LlFrameDev {
    unsigned long long out_off;       // sample-frame offset of the frame in the output
    unsigned long long scratch_off[2];  // first two channel wrappers (mid/side needs exactly two)
    unsigned int first_channel, n_channels;
    unsigned int samples;
    unsigned int mid_side;
};

}  // namespace flo

using flo::kRiceMaxK;
using flo::kRiceTileBits;
using flo::LlChannelDev;
using flo::LlFrameDev;

// Which kernels take one channel wrapper. This mirrors the limits of lldec_kernels.hip: its tile tables have room for
// Rice parameters k <= kRiceMaxK only; the tile stages put a wrapper's tiles (four per workgroup at least) in gridDim.y
// (<= 65535); the f64 LPC recurrence is exact only for sum |coef| < 2^21 and shift <= 20 (it holds
// r * 2^shift + sum c * s, |r|, |s| < 2^31, in 53 bits). A wrapper outside them goes to the serial kernel. Wrappers that
// are no LPC recurrence ll_predict's row form takes (fixed predictors, raw, silent, too short) are "others".
struct LlRoute {
    uint32_t tiles = 0;   // Rice tiles of the parallel form (0: none, or serial)
    uint8_t serial = 0, other = 0;
};
LlRoute ll_route(const LlChannelDev &d, bool force_serial);

// A wrapper's descriptor; samples and out_off are set when it joins a list.
LlChannelDev ll_channel(uint64_t off, uint32_t len, uint8_t n_coeffs, uint8_t shift_bits, uint8_t rice_k, const int32_t *coeffs);

// The wrappers of one call in the order the kernels see them, with what the wrapper stage needs besides: the running
// tile count, the serial flags and the "others". Each wrapper's samples get the next run of the int32 scratch
// (out_off). clear() keeps the capacity.
struct LlWrapperList {
    std::vector<LlChannelDev> chs;
    std::vector<unsigned int> tile0{0u};   // [chs + 1]
    std::vector<int> serial;
    std::vector<unsigned int> others;
    std::vector<LlFrameDev> frs;           // the frames appended by add_frame
    uint64_t scratch = 0;                  // ints of scratch the wrappers take
    unsigned max_tiles = 0, max_samples = 0;

    void clear();
    unsigned tiles() const { return tile0.back(); }
    // append one wrapper, routed already; returns its index
    unsigned push(const LlChannelDev &d, const LlRoute &r);
    // append a frame of n wrappers, wrapper(k) giving wrapper k's descriptor, each routed here
    template <class F>
    void add_frame(uint64_t out_off, uint32_t samples, bool mid_side, unsigned n, bool force_serial, F &&wrapper) {
        LlFrameDev fd{};
        fd.out_off = out_off;
        fd.first_channel = (unsigned)chs.size();
        fd.n_channels = n;
        fd.samples = samples;
        fd.mid_side = mid_side ? 1u : 0u;
        for (unsigned k = 0; k < n; k++) {
            LlChannelDev d = wrapper(k);
            d.samples = samples;
            if (k < 2) fd.scratch_off[k] = scratch;
            push(d, ll_route(d, force_serial));
        }
        if (samples > max_samples) max_samples = samples;
        frs.push_back(fd);
    }
};
