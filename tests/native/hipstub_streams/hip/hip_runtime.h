// Test-only stand-in for <hip/hip_runtime.h>: a runtime whose device runs LATE, for tests/native/stager_paths_test.cpp,
// which compiles flo_amd/csrc/stager.cpp against it with a plain C++ compiler. The model is
// tests/native/hipstub_streams/late_runtime.cpp; its head says what is modelled. Nothing else may include this header.
#pragma once
#include <stddef.h>
#include <stdint.h>

typedef enum hipError_t {
    hipSuccess = 0,
    hipErrorInvalidValue = 1,
    hipErrorOutOfMemory = 2,
} hipError_t;

typedef enum hipMemcpyKind {
    hipMemcpyHostToHost = 0,
    hipMemcpyHostToDevice = 1,
    hipMemcpyDeviceToHost = 2,
} hipMemcpyKind;

typedef struct hipstubStream *hipStream_t;
typedef struct hipstubEvent *hipEvent_t;

#define hipEventDisableTiming 0x2
#define hipStreamNonBlocking 0x1

hipError_t hipGetDevice(int *device);
hipError_t hipSetDevice(int device);
hipError_t hipMalloc(void **ptr, size_t bytes);
hipError_t hipFree(void *ptr);
hipError_t hipHostMalloc(void **ptr, size_t bytes, unsigned flags = 0);
hipError_t hipHostFree(void *ptr);
hipError_t hipStreamCreateWithFlags(hipStream_t *stream, unsigned flags);
hipError_t hipStreamDestroy(hipStream_t stream);
hipError_t hipStreamSynchronize(hipStream_t stream);
hipError_t hipEventCreateWithFlags(hipEvent_t *event, unsigned flags);
hipError_t hipEventDestroy(hipEvent_t event);
hipError_t hipEventRecord(hipEvent_t event, hipStream_t stream);
hipError_t hipEventSynchronize(hipEvent_t event);
hipError_t hipStreamWaitEvent(hipStream_t stream, hipEvent_t event, unsigned flags);
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t stream);

// ---- test-only calls ---------------------------------------------------------------------------------------------------
namespace hipstub {

constexpr size_t kGuard = 64;               // guard bytes on either side of every hipMalloc block
constexpr unsigned char kGuardByte = 0xA5;
constexpr unsigned char kPoison = 0xDD;     // what hipFree / hipHostFree leave in a block

// scheduling: lazy (false) - nothing runs until something synchronises on it; eager (true) - an op runs as soon as it is
// at the head of its stream with its dependencies met. Set while nothing is queued.
void set_eager(bool eager);

// a gate holds `stream` behind it until it is opened (the CPU counterpart of a delay kernel); returns the gate's id
int gate(hipStream_t stream);
void open_gate(int id);
// number of host threads that are blocked inside a synchronise behind a closed gate right now
int gate_waiters();

hipError_t memset_async(void *dst, int value, size_t bytes, hipStream_t stream);
hipError_t nop_async(hipStream_t stream);

// the n-th call from now fails (1 = the next one); 0 = none
void fail_host_malloc(int nth);
void fail_event_create(int nth);

// run everything that is queued anywhere (every gate must be open)
void drain_all();

struct Counts {
    unsigned long long host_mallocs, host_frees, dev_mallocs, dev_frees, events_made, events_destroyed, streams_made, streams_destroyed;
    unsigned long long copies_run, copied_bytes, pinned_copies, pageable_copies;
    size_t host_live, dev_live, events_live, streams_live;   // made and not yet released
    unsigned long long violations;                            // what the model itself found wrong (each is printed to stderr)
};
Counts counts();
void reset_copy_counts();
// true if the guard bytes around the hipMalloc block `p` are intact
bool guards_intact(const void *p);

}  // namespace hipstub
