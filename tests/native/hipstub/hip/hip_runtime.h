// Test-only stand-in for <hip/hip_runtime.h>: the five runtime calls and the two error codes that
// flo_amd/csrc/devpool.cpp needs, so that the pool builds with a plain C++ compiler and runs on the CPU
// (tests/native/devpool_threads_test.cpp defines the calls on top of malloc). Nothing else may include it.
#pragma once
#include <stddef.h>

typedef enum hipError_t {
    hipSuccess = 0,
    hipErrorOutOfMemory = 2,
} hipError_t;

hipError_t hipGetDevice(int *device);
hipError_t hipMalloc(void **ptr, size_t bytes);
hipError_t hipFree(void *ptr);
hipError_t hipMemset(void *dst, int value, size_t bytes);
hipError_t hipDeviceSynchronize(void);
