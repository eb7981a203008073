// devmem.hpp — the two scope guards of every entry point that takes temporary blocks from the device pool (devpool.hpp):
// the block itself, and the "stream idle before the blocks go back" guard declared behind it. Not part of the C ABI.
#pragma once
#include "ctx_internal.hpp"
#include "devpool.hpp"

// One pool block, released on scope exit. DevBuf<T>: n elements of T through alloc(); DevMem: bytes through pool_alloc(&m.p, ..).
template <class T = void>
struct DevBuf {
    T *p = nullptr;
    ~DevBuf() {
        if (p) pool_free(p);   // the owner has synchronised the stream by the time this runs (QuiesceOnExit)
    }
    bool alloc(size_t n) { return pool_alloc(&p, (n ? n : 1) * sizeof(T)) == hipSuccess; }
    template <class U>
    U *as() const { return reinterpret_cast<U *>(p); }
};
using DevMem = DevBuf<>;
// Declared right behind a function's DevMem objects, so that it is destroyed BEFORE them: whatever way the function is
// left (an error return in the middle included), the context's stream is idle when the blocks go back to the pool, where
// another context or thread may be handed them at once. On the normal path the stream has been synchronised already and
// this costs a few microseconds.
struct QuiesceOnExit {
    flo_ctx *c;
    explicit QuiesceOnExit(flo_ctx *ctx) : c(ctx) {}
    ~QuiesceOnExit() {
        if (c && c->stream) hipStreamSynchronize(c->stream);
    }
};
