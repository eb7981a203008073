// stream_delay.hip — the delay kernel behind flo_debug_stream_delay (see stream_delay.hpp), in a translation unit of its
// own so that every other code object stays what it was.
//
// One wavefront sleeps in a loop whose iteration count the host fixes. The kernel reads and writes no memory, waits on
// nothing and polls nothing, so it ends by construction: it cannot deadlock streams that share a hardware queue (a
// process has a handful of queues and the library owns more streams than that). The duration is approximate - s_sleep
// counts shader clocks in units of 64 and the clock moves - and only "at least about this long" matters.
#include "stream_delay.hpp"

#include "../../include/flo_hip.h"

namespace flo {

constexpr int kSleepUnits = 16;                      // s_sleep 16: about 16 * 64 shader clocks
constexpr unsigned int kSleepClocks = kSleepUnits * 64;

__global__ __launch_bounds__(64) void stream_delay_kernel(unsigned int iterations) {
    for (unsigned int i = 0; i < iterations; i++) __builtin_amdgcn_s_sleep(kSleepUnits);
}

std::atomic<int> g_stream_delay{-1};
static std::atomic<unsigned long long> g_stream_delays{0};

// shader clock of the current device in MHz (read once; 2400 where the driver does not say)
static unsigned int shader_mhz() {
    static std::atomic<unsigned int> mhz{0};
    unsigned int m = mhz.load(std::memory_order_relaxed);
    if (m) return m;
    int dev = 0, khz = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&khz, hipDeviceAttributeClockRate, dev) != hipSuccess || khz < 100000 || khz > 10000000)
        khz = 2400000;
    m = (unsigned int)(khz / 1000);
    mhz.store(m, std::memory_order_relaxed);
    return m;
}

hipError_t stream_delay_enqueue(hipStream_t s, int us) {
    if (us < 0) return hipSuccess;
    if (us > kMaxStreamDelayUs) us = kMaxStreamDelayUs;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) != hipSuccess) (void)hipGetLastError();   // (the legacy stream cannot be asked)
    else if (cap != hipStreamCaptureStatusNone) return hipSuccess;
    const unsigned int iterations = (unsigned int)(((unsigned long long)us * shader_mhz() + kSleepClocks - 1) / kSleepClocks);
    hipLaunchKernelGGL(stream_delay_kernel, dim3(1), dim3(64), 0, s, iterations);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) g_stream_delays.fetch_add(1, std::memory_order_relaxed);
    return e;
}

}  // namespace flo

extern "C" int flo_debug_stream_delay(int microseconds) {
    if (microseconds < -1 || microseconds > flo::kMaxStreamDelayUs) return flo::g_stream_delay.load(std::memory_order_relaxed);
    return flo::g_stream_delay.exchange(microseconds, std::memory_order_relaxed);
}

extern "C" uint64_t flo_debug_stream_delays(void) { return flo::g_stream_delays.load(std::memory_order_relaxed); }

extern "C" int flo_debug_delay_enqueue(void *stream, int microseconds) {
    if (microseconds < 0 || microseconds > flo::kMaxStreamDelayUs) return FLO_ERR_ARG;
    return flo::stream_delay_enqueue((hipStream_t)stream, microseconds) == hipSuccess ? FLO_OK : FLO_ERR_DEVICE;
}
