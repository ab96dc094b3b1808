// kdf_hostutil.h -- host plumbing the engine and the read spool share (no kernels): the owning buffers and the grow-only
// rule (kdf_devbuf.h), a HIP-event timer with the stage stamps of the binned path, and the read-offsets check.  Each takes
// what differs between its users as a parameter: the slack and the wait before a free (dev_reserve), the tag of a timed
// span (EvTimer), where a message goes (check_read_offsets).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <vector>

#include "kdf_devbuf.h"

// ---- HIP-event timing -------------------------------------------------------------------------------------------------------
// Pending (start, stop) event pairs with a 64-bit tag each, folded into running totals by collect(): `passes` counts the
// pairs with a non-zero tag, `tag_sum` adds the tags up.  A plain timer tags every span 1 (passes = spans).
struct EvTimer {
    struct Pair { hipEvent_t e0, e1; uint64_t tag; };
    std::vector<Pair> pending;
    double ms = 0.0;
    uint64_t passes = 0, tag_sum = 0;
    // waits for every pending stop event, adds the spans up and destroys their events; nothing pending: nothing done
    void collect() {
        for (const Pair &p : pending) {
            float t = 0.f;
            (void)hipEventSynchronize(p.e1);
            if (hipEventElapsedTime(&t, p.e0, p.e1) == hipSuccess) { ms += t; tag_sum += p.tag; passes += p.tag != 0; }
            (void)hipEventDestroy(p.e0); (void)hipEventDestroy(p.e1);
        }
        pending.clear();
    }
    void reset() { collect(); ms = 0.0; passes = tag_sum = 0; }
    int64_t us() { collect(); return (int64_t)(ms * 1000.0 + 0.5); }
};
// One timed span on stream s: starts where it is declared, joins the timer's pending pairs at stop().  With `on` false, or
// when an event cannot be created or recorded, it times nothing; a span that goes out of scope unstopped (an error return
// between the launches) leaves nothing behind.
struct EvSpan {
    EvTimer &timer; hipStream_t s; uint64_t tag;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    EvSpan(EvTimer &t, bool on, hipStream_t s_, uint64_t tag_ = 1) : timer(t), s(s_), tag(tag_) {
        if (on && (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess || hipEventRecord(e0, s) != hipSuccess)) drop();
    }
    EvSpan(const EvSpan &) = delete;
    EvSpan &operator=(const EvSpan &) = delete;
    ~EvSpan() { drop(); }
    void stop() {
        if (!e1) return;
        if (hipEventRecord(e1, s) != hipSuccess) return drop();
        timer.pending.push_back({e0, e1, tag});
        e0 = e1 = nullptr;
    }
    void drop() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        e0 = e1 = nullptr;
    }
};
// The stamps between the stages of one launch group on stream s: stamp() records an event (with `on` false: nothing),
// commit() hands the events over as one record; stamps that go out of scope uncommitted (an error return between the
// launches) are destroyed.  (Hidden: the library's symbol table gains nothing by it.)
struct __attribute__((visibility("hidden"))) StageStamps {
    bool on; hipStream_t s;
    std::vector<hipEvent_t> ev;
    StageStamps(bool on_, hipStream_t s_) : on(on_), s(s_) {}
    StageStamps(const StageStamps &) = delete;
    StageStamps &operator=(const StageStamps &) = delete;
    ~StageStamps() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
    void stamp() {
        hipEvent_t e = nullptr;
        if (!on || hipEventCreate(&e) != hipSuccess) return;
        (void)hipEventRecord(e, s);
        ev.push_back(e);
    }
    void commit(std::vector<std::vector<hipEvent_t>> &records) {
        if (on) records.push_back(ev);
        ev.clear();
    }
};
// stat "<name>_us" / "<name>_passes" of a table of timers (names[i] NULL: timer i has no stats of that form) -> the timer
// and which of the two, or NULL
static inline EvTimer *timer_of_stat(EvTimer *timers, const char *const *names, int count, const std::string &stat, bool *us) {
    for (int i = 0; i < count; ++i) {
        if (!names[i] || stat.rfind(names[i], 0) != 0) continue;
        const std::string rest = stat.substr(std::char_traits<char>::length(names[i]));
        if (rest == "_us" || rest == "_passes") { *us = rest == "_us"; return &timers[i]; }
    }
    return nullptr;
}

// ---- read offsets -------------------------------------------------------------------------------------------------------------
// n_reads >= 0, and for n_reads > 0: offsets given, offsets[0] >= 0, no decrease.  fail(code, fmt, ...) -> int takes the
// message of a KDF_ERR_INVALID (1) and returns the code; 0 when all holds.
template <typename F>
static int check_read_offsets(F &&fail, const char *fn, const int64_t *offs, int64_t n_reads) {
    if (n_reads < 0) return fail(1, "%s: n_reads = %lld is negative", fn, (long long)n_reads);
    if (n_reads == 0) return 0;
    if (!offs) return fail(1, "%s: read_offsets is NULL", fn);
    if (offs[0] < 0) return fail(1, "%s: read_offsets[0] = %lld is negative", fn, (long long)offs[0]);
    for (int64_t r = 0; r < n_reads; ++r)
        if (offs[r + 1] < offs[r])
            return fail(1, "%s: read_offsets decrease at read %lld (%lld after %lld)", fn, (long long)r, (long long)offs[r + 1],
                        (long long)offs[r]);
    return 0;
}
