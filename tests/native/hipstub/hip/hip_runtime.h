// A stand-in for <hip/hip_runtime.h> with the four allocator calls kdf_devbuf.h uses, over malloc: every live allocation
// is counted, a free of a pointer that is not live (a second free) is counted as a fault, and stub_fail_next makes the
// next allocation fail.  For tests/native/devbuf_check.cpp, built with a host compiler; no GPU, no HIP.
#pragma once
#include <cstddef>
#include <cstdlib>
#include <set>

typedef int hipError_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2 };

struct HipStub {
    std::set<void *> live_dev, live_pin;
    int allocs = 0, bad_frees = 0, last_error_cleared = 0;
    bool fail_next = false;
    hipError_t alloc(std::set<void *> &live, void **p, size_t n) {
        if (fail_next) { fail_next = false; *p = (void *)0x1; return hipErrorOutOfMemory; }   // (a failed call may leave garbage behind)
        *p = malloc(n ? n : 1);
        live.insert(*p); ++allocs;
        return hipSuccess;
    }
    hipError_t free(std::set<void *> &live, void *p) {
        if (!live.erase(p)) { ++bad_frees; return 1; }
        ::free(p);
        return hipSuccess;
    }
    size_t live() const { return live_dev.size() + live_pin.size(); }
};
inline HipStub &hip_stub() { static HipStub s; return s; }

inline hipError_t hipMalloc(void **p, size_t n) { return hip_stub().alloc(hip_stub().live_dev, p, n); }
inline hipError_t hipFree(void *p) { return hip_stub().free(hip_stub().live_dev, p); }
inline hipError_t hipHostMalloc(void **p, size_t n) { return hip_stub().alloc(hip_stub().live_pin, p, n); }
inline hipError_t hipHostFree(void *p) { return hip_stub().free(hip_stub().live_pin, p); }
inline hipError_t hipGetLastError() { ++hip_stub().last_error_cleared; return hipSuccess; }
