// kdf_devbuf.h -- the one way libkdf.so's host code owns memory it allocates: DevBuf (hipMalloc) and PinBuf
// (hipHostMalloc) free what they hold when they go, move and do not copy.  dev_reserve is the grow-only rule on top of
// DevBuf.  Needs hipMalloc / hipFree / hipHostMalloc / hipHostFree / hipGetLastError of <hip/hip_runtime.h> and nothing
// else, so a host compiler checks it against a stub of that header (tests/native/devbuf_check.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

template <bool PINNED>
struct OwnedBuf {
    void *p = nullptr;
    size_t bytes = 0;
    OwnedBuf() = default;
    OwnedBuf(const OwnedBuf &) = delete;
    OwnedBuf &operator=(const OwnedBuf &) = delete;
    OwnedBuf(OwnedBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    OwnedBuf &operator=(OwnedBuf &&o) noexcept {
        if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~OwnedBuf() { release(); }
    void release() { if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p)); p = nullptr; bytes = 0; }
    // exactly n bytes, contents undefined; what was held goes first.  On failure the buffer is empty and HIP's sticky
    // error is cleared
    hipError_t alloc(size_t n) {
        release();
        const hipError_t e = PINNED ? hipHostMalloc(&p, n) : hipMalloc(&p, n);
        if (e != hipSuccess) { (void)hipGetLastError(); p = nullptr; return e; }
        bytes = n;
        return hipSuccess;
    }
    template <typename T> T *as() const { return (T *)p; }
    explicit operator bool() const { return p != nullptr; }
};
using DevBuf = OwnedBuf<false>;       // device memory
using PinBuf = OwnedBuf<true>;        // pinned host memory

// ---- grow-only device scratch ---------------------------------------------------------------------------------------------
// what a site allocates for a request of b bytes
static inline size_t slack_8th(size_t b) { return b + b / 8 + 4096; }
static inline size_t slack_16th(size_t b) { return b + b / 16 + 4096; }
static inline size_t slack_page(size_t b) { return b + 4096; }
static inline size_t slack_exact(size_t b) { return b; }

// Room for `bytes` in b.  A buffer that is too small is replaced by one of `want` bytes (>= bytes: the site's slack rule);
// the old contents are not kept.  quiesce() -> hipError_t waits for whatever may still read the old buffer and is called
// only when there is one to free; if it fails the buffer stays.  Returns quiesce's or hipMalloc's error (b is then empty).
template <typename Q>
static hipError_t dev_reserve(DevBuf &b, size_t bytes, size_t want, Q &&quiesce) {
    if (b.bytes >= bytes) return hipSuccess;
    if (b.p) {
        const hipError_t e = quiesce();
        if (e != hipSuccess) return e;
    }
    return b.alloc(want);
}
