// stream_delay.hpp — a bounded delay the library can queue in front of its own work (flo_debug_stream_delay), so that
// tests can make the device run late: results must not depend on when queued work runs. Defined in stream_delay.hip.
//
// With the switch on, one delay goes in front of every launch (timed_launch and the launch groups that bypass it) and
// onto every stream of the library's own right behind each hipStreamWaitEvent issued on it, so work that a missing
// wait, fork, join or early release would let the host or another stream overtake really is still queued.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>

namespace flo {

// flo_debug_stream_delay's setting: -1 off, 0 .. kMaxStreamDelayUs the microseconds of every delay the library queues
extern std::atomic<int> g_stream_delay;
constexpr int kMaxStreamDelayUs = 5000;

// One delay of about `us` microseconds on `s` (nothing while `s` is being captured). hipSuccess or the launch's error.
hipError_t stream_delay_enqueue(hipStream_t s, int us);

// The library's sites: one relaxed load when the switch is off.
inline hipError_t stream_delay(hipStream_t s) {
    const int us = g_stream_delay.load(std::memory_order_relaxed);
    return us < 0 ? hipSuccess : stream_delay_enqueue(s, us);
}

}  // namespace flo
