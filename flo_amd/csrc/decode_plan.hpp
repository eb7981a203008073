// decode_plan.hpp — the host side of the device decode path, shared by every entry point that drives the decode kernels:
// flo_decode, flo_batch_decode and flo_decode_frame_at (flo_api.cpp), the corpus windows (corpus.cpp) and the streaming
// decoders (sdec.cpp). Which kernel takes a lossless channel wrapper, the per-call wrapper list, the descriptor block that
// carries a call's host arrays to the device in one copy, the pinned staging ring of the calls that never synchronise the
// host, and the launches of the wrapper stage. What differs between the callers (how device scratch grows, which finish
// kernel runs, whether the output needs clearing) stays with them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <vector>

#include "ctx_internal.hpp"
#include "decode_kernels.hpp"

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

// A call's host arrays as one block for one copy: part i at off[i], a multiple of 256 bytes. A part with no source is
// space the caller fills itself.
struct DescPart {
    const void *src;
    size_t bytes;
};
template <class T>
DescPart desc_part(const std::vector<T> &v) { return {v.data(), v.size() * sizeof(T)}; }
struct DescBlock {
    static constexpr int kMaxParts = 10;
    DescPart part[kMaxParts];
    size_t off[kMaxParts];
    size_t bytes = 0;
    int n = 0;
    DescBlock(std::initializer_list<DescPart> parts);
    void fill(uint8_t *pin) const;
    template <class T>
    T *at(void *base, int i) const { return reinterpret_cast<T *>(static_cast<uint8_t *>(base) + off[i]); }
};

// Pinned staging of the calls that queue their work without synchronising the host (corpus windows, streaming
// decoders): a slot is written again only once the copy out of it has completed, in steady state long since.
// fence_in orders the ctx stream after what the caller queued on its stream, fence_out the caller's later work after
// the ctx stream.
class StageRing {
public:
    static constexpr int kSlots = 8;
    StageRing() = default;
    StageRing(const StageRing &) = delete;
    StageRing &operator=(const StageRing &) = delete;
    ~StageRing();   // waits for the copies, frees the slots
    bool init();    // the events; false if one could not be made
    // the next slot, grown to at least `bytes`
    int acquire(flo_ctx *c, size_t bytes, uint8_t **pin);
    // the acquired slot's first `bytes` to `dst` on the ctx stream
    int upload(flo_ctx *c, void *dst, size_t bytes);
    int fence_in(flo_ctx *c, hipStream_t caller);
    int fence_out(flo_ctx *c, hipStream_t caller);

private:
    struct Slot {
        void *pin = nullptr;
        size_t cap = 0;
        hipEvent_t ev = nullptr;
        bool used = false;
    };
    Slot slots_[kSlots];
    unsigned next_ = 0;
    Slot *cur_ = nullptr;
    hipEvent_t ev_in_ = nullptr, ev_out_ = nullptr;
};

// The wrapper stage of `w` on the ctx stream: ll_decode_parallel, then ll_decode for the wrappers left to the serial
// kernel, under the given profile names. d_ch .. d_others are the device copies of w's arrays; scratch holds w.scratch
// ints, tabs and ent w.tiles() tile tables and entries. The caller launches its finish kernel behind it.
int launch_ll_wrappers(flo_ctx *c, const LlWrapperList &w, const uint8_t *bytes, const LlChannelDev *d_ch, const unsigned int *d_tile0,
                       int *d_serial, const unsigned int *d_others, int *scratch, unsigned int *tabs, uint2 *ent,
                       const char *name_parallel, const char *name_serial);
