// devbuf_check.cpp -- the owning buffers and the grow-only rule of csrc/kdf_devbuf.h, against the counting allocator of
// tests/native/hipstub: a stand-alone host program (tests/test_devbuf_host.py builds and runs it, with
// -fsanitize=address,undefined; nothing of it is loaded into Python).  Prints one line per check and a summary line.
#include <cstdio>
#include <utility>

#include "kdf_devbuf.h"

static int failures = 0, checks = 0;
#define CHECK(cond) \
    do { ++checks; if (!(cond)) { ++failures; printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } } while (0)

template <typename B>
static void owning(const char *name) {
    HipStub &st = hip_stub();
    const size_t before = st.live();
    {                                                       // the destructor frees
        B a;
        CHECK(!a && a.p == nullptr && a.bytes == 0);
        CHECK(a.alloc(100) == hipSuccess && a && a.bytes == 100 && st.live() == before + 1);
        a.template as<unsigned char>()[99] = 7;             // (the sanitizer sees the write: the size is what was asked for)
    }
    CHECK(st.live() == before);
    {                                                       // a move leaves the source empty; nothing is freed twice
        B a;
        CHECK(a.alloc(64) == hipSuccess);
        void *const p = a.p;
        B b(std::move(a));
        CHECK(a.p == nullptr && a.bytes == 0 && b.p == p && b.bytes == 64 && st.live() == before + 1);
        B c;
        CHECK(c.alloc(32) == hipSuccess && st.live() == before + 2);
        c = std::move(b);                                   // what c held goes, b is empty
        CHECK(b.p == nullptr && b.bytes == 0 && c.p == p && c.bytes == 64 && st.live() == before + 1);
        B &same = c;
        c = std::move(same);                                // self-move: nothing happens
        CHECK(c.p == p && c.bytes == 64 && st.live() == before + 1);
        c.release(); c.release();                           // release twice: one free
        CHECK(!c && st.live() == before);
    }
    {                                                       // alloc replaces; a failing alloc leaves the buffer empty
        B a;
        CHECK(a.alloc(16) == hipSuccess && a.alloc(48) == hipSuccess && a.bytes == 48 && st.live() == before + 1);
        const int cleared = st.last_error_cleared;
        st.fail_next = true;
        CHECK(a.alloc(80) == hipErrorOutOfMemory && a.p == nullptr && a.bytes == 0 && st.live() == before);
        CHECK(st.last_error_cleared == cleared + 1);        // HIP's sticky error does not outlive the failure
    }
    CHECK(st.live() == before && st.bad_frees == 0);
    printf("%s: ok so far (%d checks)\n", name, checks);
}

static void reserve() {
    HipStub &st = hip_stub();
    int quiesced = 0;
    auto wait_ok = [&] { ++quiesced; return (hipError_t)hipSuccess; };
    auto wait_bad = [&] { ++quiesced; return (hipError_t)77; };
    {
        DevBuf b;
        // empty: allocated with the site's slack, nothing to wait for
        CHECK(dev_reserve(b, 1000, slack_8th(1000), wait_ok) == hipSuccess && b.bytes == 1000 + 125 + 4096 && quiesced == 0);
        // room already there: neither quiesce nor the allocator
        void *const p = b.p;
        const int allocs = st.allocs;
        CHECK(dev_reserve(b, 5000, slack_8th(5000), wait_bad) == hipSuccess && b.p == p && quiesced == 0 && st.allocs == allocs);
        CHECK(dev_reserve(b, 0, 0, wait_bad) == hipSuccess && b.p == p && quiesced == 0 && st.allocs == allocs);
        // too small, quiesce fails: pointer and size stay
        const size_t bytes = b.bytes;
        CHECK(dev_reserve(b, 1 << 20, slack_page(1 << 20), wait_bad) == 77 && b.p == p && b.bytes == bytes && quiesced == 1 && st.allocs == allocs);
        // too small, quiesce passes: replaced (old contents are not kept), one wait
        CHECK(dev_reserve(b, 1 << 20, slack_page(1 << 20), wait_ok) == hipSuccess && b.bytes == (1 << 20) + 4096 && quiesced == 2 && st.live() == 1);
        // a failing allocation: the error comes back, the buffer is empty
        st.fail_next = true;
        CHECK(dev_reserve(b, 1 << 21, slack_exact(1 << 21), wait_ok) == hipErrorOutOfMemory && b.p == nullptr && b.bytes == 0 && quiesced == 3 && st.live() == 0);
        // ... and usable again
        CHECK(dev_reserve(b, 10, slack_16th(10), wait_bad) == hipSuccess && b.bytes == 10 + 4096 && quiesced == 3);
    }
    CHECK(st.live() == 0 && st.bad_frees == 0);
    CHECK(slack_8th(800) == 800 + 100 + 4096 && slack_16th(1600) == 1600 + 100 + 4096 && slack_page(5) == 5 + 4096 && slack_exact(5) == 5);
}

int main() {
    owning<DevBuf>("DevBuf");
    owning<PinBuf>("PinBuf");
    {                                                       // each kind goes back to its own allocator
        DevBuf d; PinBuf h;
        CHECK(d.alloc(8) == hipSuccess && h.alloc(8) == hipSuccess);
        CHECK(hip_stub().live_dev.size() == 1 && hip_stub().live_pin.size() == 1);
    }
    reserve();
    const size_t live = hip_stub().live();
    CHECK(live == 0);
    printf("devbuf: %d checks, %d failed, %zu live allocations at exit, %d bad frees\n", checks, failures, live, hip_stub().bad_frees);
    return failures || live || hip_stub().bad_frees ? 1 : 0;
}
