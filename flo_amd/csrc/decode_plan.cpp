// decode_plan.cpp — see decode_plan.hpp.
#include "decode_plan.hpp"

#include <cassert>
#include <cstring>

DescBlock::DescBlock(std::initializer_list<DescPart> parts) {
    assert(parts.size() <= (size_t)kMaxParts);
    for (const DescPart &p : parts) {
        part[n] = p;
        off[n++] = bytes;
        bytes += (p.bytes + 255) & ~(size_t)255;
    }
}

void DescBlock::fill(uint8_t *pin) const {
    for (int i = 0; i < n; i++)
        if (part[i].src && part[i].bytes) memcpy(pin + off[i], part[i].src, part[i].bytes);
}

StageRing::~StageRing() {
    for (Slot &s : slots_) {
        if (s.ev) hipEventSynchronize(s.ev), hipEventDestroy(s.ev);
        if (s.pin) hipHostFree(s.pin);
    }
    if (ev_in_) hipEventDestroy(ev_in_);
    if (ev_out_) hipEventDestroy(ev_out_);
}

bool StageRing::init() {
    bool ok = true;
    for (Slot &s : slots_)
        if (hipEventCreateWithFlags(&s.ev, hipEventDisableTiming) != hipSuccess) s.ev = nullptr, ok = false;
    if (hipEventCreateWithFlags(&ev_in_, hipEventDisableTiming) != hipSuccess) ev_in_ = nullptr, ok = false;
    if (hipEventCreateWithFlags(&ev_out_, hipEventDisableTiming) != hipSuccess) ev_out_ = nullptr, ok = false;
    return ok;
}

int StageRing::acquire(flo_ctx *c, size_t bytes, uint8_t **pin) {
    Slot &sl = slots_[next_++ % kSlots];
    cur_ = &sl;
    if (!sl.ev) return fail(c, FLO_ERR_DEVICE, "hipEventCreate failed");
    if (sl.used) HIPCHK(c, hipEventSynchronize(sl.ev));
    if (sl.cap < bytes) {
        if (sl.pin) hipHostFree(sl.pin);
        sl.pin = nullptr;
        sl.cap = 0;
        const size_t want = bytes + bytes / 4;
        HIPCHK(c, hipHostMalloc(&sl.pin, want, hipHostMallocDefault));
        sl.cap = want;
    }
    *pin = (uint8_t *)sl.pin;
    return FLO_OK;
}

int StageRing::upload(flo_ctx *c, void *dst, size_t bytes) {
    HIPCHK(c, hipMemcpyAsync(dst, cur_->pin, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipEventRecord(cur_->ev, c->stream));
    cur_->used = true;
    return FLO_OK;
}

int StageRing::fence_in(flo_ctx *c, hipStream_t caller) {
    if (caller != c->stream) {
        HIPCHK(c, hipEventRecord(ev_in_, caller));
        HIPCHK(c, hipStreamWaitEvent(c->stream, ev_in_, 0));
        HIPCHK(c, stream_delay(c->stream));
    }
    return FLO_OK;
}

int StageRing::fence_out(flo_ctx *c, hipStream_t caller) {
    if (caller != c->stream) {
        HIPCHK(c, hipEventRecord(ev_out_, c->stream));
        HIPCHK(c, hipStreamWaitEvent(caller, ev_out_, 0));
    }
    return FLO_OK;
}

int launch_ll_wrappers(flo_ctx *c, const LlWrapperList &w, const uint8_t *bytes, const LlChannelDev *d_ch, const unsigned int *d_tile0,
                       int *d_serial, const unsigned int *d_others, int *scratch, unsigned int *tabs, uint2 *ent,
                       const char *name_parallel, const char *name_serial) {
    const unsigned n = (unsigned)w.chs.size();
    LlParArgs P{bytes, d_ch, n, scratch, d_tile0, tabs, ent, d_serial, d_others, (unsigned)w.others.size()};
    int rc = timed_launch(c, name_parallel, [&] { return launch_ll_decode_parallel(P, w.max_tiles, c->stream); });
    if (rc != FLO_OK) return rc;
    LlDecArgs S{bytes, d_ch, n, scratch, d_serial};
    return timed_launch(c, name_serial, [&] { return launch_ll_decode(S, c->stream); });
}
