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
#include "ll_route.hpp"

// (ll_route, ll_channel and LlWrapperList: ll_route.hpp, which needs no HIP)

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
