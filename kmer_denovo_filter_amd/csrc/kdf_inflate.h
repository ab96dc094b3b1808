// kdf_inflate.h -- raw DEFLATE (RFC 1951) decoder of one BGZF block, written once for the device and the host.
//
// The decoder is a template over a LANE GROUP: L.id() of L.count() lanes that run the same code in lockstep.  On the
// device the group is one wavefront (kdf_bamdev.h: 64 lanes, one BGZF block per wave); on the host it is one lane
// (tests/native/inflate_check.cpp compiles THIS file with a host compiler and sanitizers).  All control flow is uniform
// over the group: every lane reads the same input bits and the same table entries (one broadcast load each), so the
// "symbol loop of one lane" costs no cross-lane traffic, and the lanes differ only where they share out work:
//   * the fast decode tables are filled symbol-strided,
//   * stored bytes and match bytes are copied lane-strided (byte i of a match comes from out[pos - dist + i % dist],
//     which is always below pos: bytes written by EARLIER instructions of the same group, never by this copy).
// A later load sees an earlier store of another lane of the same wave with no fence instruction: the vector memory
// instructions of a wavefront are issued in order into one per-CU L1 that every lane of the wave shares, which is why a
// fence at wavefront scope compiles to no instruction (LLVM AMDGPU backend user guide, "Memory Model" for gfx90a / gfx942,
// the targets gfx950 follows: "no special action is required for coherence between the lanes of a single wavefront").  It
// is the guarantee a single lane's own store-then-load of one address rests on, at cache-line granularity.  L.sync() is
// that wavefront-scope fence plus a wave barrier: it keeps the COMPILER from moving accesses across the points where
// lanes exchange data.  On the GPU the equality with zlib over matches at every distance around the lane count, and over
// chains of matches that each copy what the one before stored, checks it
// (test_gpu_bamdev.py::test_lanes_see_the_bytes_other_lanes_stored_at_every_distance).
//
// Memory safety is by construction, whatever the bytes say:
//   * every input read is below `in_len` (the bit reader never looks past it; a code that needs more bits than are
//     left is KDF_INF_TRUNCATED),
//   * every output write is below `out_len` (the block's ISIZE),
//   * every match distance is <= the bytes already written,
//   * over-subscribed code sets, and incomplete ones other than the single-code set zlib admits, are rejected,
//   * every iteration of every loop consumes at least one input bit or writes at least one output byte or counts a
//     bounded index up, so a malformed block can neither run away nor hang.
// A block must end exactly at out_len (KDF_INF_SIZE otherwise).  out_len == 0 decodes nothing and is KDF_INF_OK, as
// the host reader's bgzf_inflate.  No CRC is checked (the host reader checks none).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define KDF_INF_HD __host__ __device__ __forceinline__
#else
#define KDF_INF_HD inline
#endif

// block status (stat of kdf_bgzf_inflate_dev's d_block_status)
#define KDF_INF_OK          0
#define KDF_INF_TRUNCATED   1   // the payload ends inside a code, a header or a stored run
#define KDF_INF_BTYPE       2   // block type 3
#define KDF_INF_STORED      3   // LEN != ~NLEN
#define KDF_INF_CODES       4   // bad code set: too many codes, over-subscribed or incomplete, no end-of-block code, bad repeat
#define KDF_INF_SYMBOL      5   // a bit pattern that is no code of the set, or length / distance symbol out of range
#define KDF_INF_DISTANCE    6   // a distance beyond the bytes written so far
#define KDF_INF_SIZE        7   // more output than ISIZE, or the stream ends before ISIZE bytes
#define KDF_INF_BOUNDS      8   // the block table entry does not fit the buffers (checked before any byte is read)
#define KDF_INF_FORCED      9   // not the decoder's: the host marks blocks so under the engine option "bamdev_host_inflate"

#define KDF_INF_LBITS 10        // fast table of the literal/length code: 2^10 entries
#define KDF_INF_DBITS 8         // fast table of the distance code (and of the code-length code): 2^8 entries

// decode tables of one lane group: 3.7 KB (LDS on the device)
struct KdfInfTables {
    uint16_t lfast[1 << KDF_INF_LBITS];   // symbol << 4 | code length; 0: longer than the table (or no code)
    uint16_t dfast[1 << KDF_INF_DBITS];
    uint16_t lsym[288], dsym[32];         // symbols sorted by (code length, symbol): the canonical order
    uint16_t lcnt[16], dcnt[16];          // codes per length
    uint16_t work[48];                    // kdf_inf_build: first index, first code and fill cursor per length
    uint8_t lens[320];                    // code lengths being read: literal/length then distance, one run
};

struct KdfLaneHost {                      // the host's lane group: one lane
    unsigned id() const { return 0; }
    unsigned count() const { return 1; }
    void sync() const {}
};

struct KdfInfBits {                       // LSB-first bit reader over in[0, len)
    const uint8_t *in; uint32_t len, pos; uint64_t buf; uint32_t cnt;
};

KDF_INF_HD void kdf_inf_refill(KdfInfBits &b) {
    if (b.cnt >= 48) return;
    if (b.pos + 8 <= b.len) {             // (bits above cnt are stream bits already: OR-ing them in again changes nothing)
        uint64_t w; memcpy(&w, b.in + b.pos, 8);
        b.buf |= w << b.cnt;
        b.pos += (63 - b.cnt) >> 3;
        b.cnt |= 56;
        return;
    }
    while (b.cnt <= 56 && b.pos < b.len) { b.buf |= (uint64_t)b.in[b.pos++] << b.cnt; b.cnt += 8; }
}
// n <= 32 bits, or false when the input has fewer left
KDF_INF_HD bool kdf_inf_take(KdfInfBits &b, uint32_t n, uint32_t &v) {
    if (b.cnt < n) { kdf_inf_refill(b); if (b.cnt < n) return false; }
    v = (uint32_t)(b.buf & ((1ull << n) - 1));
    b.buf >>= n; b.cnt -= n;
    return true;
}

KDF_INF_HD uint32_t kdf_inf_rev(uint32_t code, uint32_t len) {   // the low `len` bits of code, reversed
    uint32_t r = 0;
    for (uint32_t i = 0; i < len; ++i) { r = (r << 1) | (code & 1); code >>= 1; }
    return r;
}

// Canonical code of lens[0, n) (n <= 288) -> cnt, sym and the fast table of 2^fbits entries.  kind 0: the code-length
// code (must be complete), 1: literal/length, 2: distance (incomplete only as zlib admits it: one code of one bit; no
// code at all builds a table that rejects every pattern).  false: over-subscribed or inadmissibly incomplete.
template <class Lane>
KDF_INF_HD bool kdf_inf_build(const Lane &L, const uint8_t *lens, uint32_t n, uint16_t *cnt, uint16_t *sym, uint16_t *fast,
                              uint32_t fbits, int kind, uint16_t *work) {
    uint16_t *offs = work, *first = work + 16, *at = work + 32;             // (in the tables, not in registers: indexed by length)
    for (uint32_t l = 0; l < 16; ++l) cnt[l] = 0;
    L.sync();
    for (uint32_t s = 0; s < n; ++s) cnt[lens[s]] = (uint16_t)(cnt[lens[s]] + 1);     // (uniform: every lane writes the same value)
    L.sync();
    int left = 1; uint32_t maxlen = 0;
    for (uint32_t l = 1; l < 16; ++l) {
        left = (left << 1) - (int)cnt[l];
        if (left < 0) return false;                                          // over-subscribed
        if (cnt[l]) maxlen = l;
    }
    if (left > 0 && maxlen != 0 && (kind == 0 || maxlen != 1)) return false;     // incomplete
    if (maxlen == 0 && kind == 0) return false;
    offs[0] = 0; offs[1] = 0; first[0] = 0; first[1] = 0;
    { uint32_t code = 0, o = 0; for (uint32_t l = 1; l < 15; ++l) { o += cnt[l]; offs[l + 1] = (uint16_t)o; code = (code + cnt[l]) << 1; first[l + 1] = (uint16_t)code; } }
    L.sync();
    {   // the sorted symbol list (serial: 288 steps at most)
        for (uint32_t l = 0; l < 16; ++l) at[l] = offs[l];
        L.sync();
        for (uint32_t s = 0; s < n; ++s) if (lens[s]) { const uint32_t a = at[lens[s]]; sym[a] = (uint16_t)s; at[lens[s]] = (uint16_t)(a + 1); }
        L.sync();
    }
    const uint32_t fsize = 1u << fbits;
    for (uint32_t i = L.id(); i < fsize; i += L.count()) fast[i] = 0;
    L.sync();
    const uint32_t total = (uint32_t)offs[15] + cnt[15];
    for (uint32_t i = L.id(); i < total; i += L.count()) {                       // symbol-strided fill
        const uint32_t s = sym[i], l = lens[s];
        if (l > fbits) continue;
        const uint32_t code = (uint32_t)first[l] + (i - offs[l]);
        const uint16_t e = (uint16_t)((s << 4) | l);
        for (uint32_t j = kdf_inf_rev(code, l); j < fsize; j += 1u << l) fast[j] = e;
    }
    L.sync();
    return true;
}

// next symbol of a code; false: truncated input (st = TRUNCATED) or no such code (st = SYMBOL)
KDF_INF_HD bool kdf_inf_symbol(KdfInfBits &b, const uint16_t *fast, uint32_t fbits, const uint16_t *cnt, const uint16_t *sym,
                               uint32_t &out, int &st) {
    kdf_inf_refill(b);
    const uint32_t e = fast[b.buf & ((1u << fbits) - 1)];
    uint32_t len = e & 15, s = e >> 4;
    if (!len) {                                                              // canonical walk, one bit per step (<= 15 steps)
        uint32_t code = 0, firstc = 0, index = 0; uint64_t bits = b.buf;
        for (len = 1; len < 16; ++len) {
            code |= (uint32_t)(bits & 1); bits >>= 1;
            const uint32_t c = cnt[len];
            if (code < firstc + c) { s = sym[index + (code - firstc)]; break; }
            index += c; firstc = (firstc + c) << 1; code <<= 1;
        }
        if (len == 16) { st = b.cnt < 15 ? KDF_INF_TRUNCATED : KDF_INF_SYMBOL; return false; }
    }
    if (len > b.cnt) { st = KDF_INF_TRUNCATED; return false; }
    b.buf >>= len; b.cnt -= len;
    out = s;
    return true;
}

// Inflate in[0, in_len) into out[0, out_len).  Returns a KDF_INF_* status, the same on every lane.
template <class Lane>
KDF_INF_HD int kdf_inflate_block(const Lane &L, const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t out_len, KdfInfTables &T) {
    const uint16_t lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    const uint8_t lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    const uint16_t dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
    const uint8_t dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
    const uint8_t clorder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    if (out_len == 0) return KDF_INF_OK;
    KdfInfBits b{in, in_len, 0, 0, 0};
    uint32_t pos = 0, v = 0, last = 0;
    int st = KDF_INF_OK;
    do {
        if (!kdf_inf_take(b, 1, last) || !kdf_inf_take(b, 2, v)) return KDF_INF_TRUNCATED;
        if (v == 3) return KDF_INF_BTYPE;
        if (v == 0) {                                                        // stored
            b.buf >>= b.cnt & 7; b.cnt -= b.cnt & 7;
            b.pos -= b.cnt >> 3; b.buf = 0; b.cnt = 0;                       // back to the first unread whole byte
            if (b.pos + 4 > in_len) return KDF_INF_TRUNCATED;
            const uint32_t len = in[b.pos] | ((uint32_t)in[b.pos + 1] << 8), nlen = in[b.pos + 2] | ((uint32_t)in[b.pos + 3] << 8);
            if ((len ^ nlen) != 0xFFFFu) return KDF_INF_STORED;
            b.pos += 4;
            if (len > in_len - b.pos) return KDF_INF_TRUNCATED;
            if (len > out_len - pos) return KDF_INF_SIZE;
            for (uint32_t i = L.id(); i < len; i += L.count()) out[pos + i] = in[b.pos + i];
            L.sync();
            pos += len; b.pos += len;
            continue;
        }
        if (v == 1) {                                                        // fixed codes
            for (uint32_t s = L.id(); s < 288; s += L.count()) T.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
            for (uint32_t s = L.id(); s < 32; s += L.count()) T.lens[288 + s] = 5;      // (30 and 31 are codes no stream may use)
            L.sync();
            if (!kdf_inf_build(L, T.lens, 288, T.lcnt, T.lsym, T.lfast, KDF_INF_LBITS, 1, T.work)) return KDF_INF_CODES;
            if (!kdf_inf_build(L, T.lens + 288, 32, T.dcnt, T.dsym, T.dfast, KDF_INF_DBITS, 2, T.work)) return KDF_INF_CODES;
        } else {                                                             // dynamic codes
            uint32_t nlen, ndist, ncode;
            if (!kdf_inf_take(b, 5, nlen) || !kdf_inf_take(b, 5, ndist) || !kdf_inf_take(b, 4, ncode)) return KDF_INF_TRUNCATED;
            nlen += 257; ndist += 1; ncode += 4;
            if (nlen > 286 || ndist > 30) return KDF_INF_CODES;
            L.sync();
            for (uint32_t i = L.id(); i < 19; i += L.count()) T.lens[i] = 0;
            L.sync();
            for (uint32_t i = 0; i < ncode; ++i) { if (!kdf_inf_take(b, 3, v)) return KDF_INF_TRUNCATED; T.lens[clorder[i]] = (uint8_t)v; }   // (uniform stores)
            L.sync();
            // (the code-length code borrows the distance tables: they are rebuilt below)
            if (!kdf_inf_build(L, T.lens, 19, T.dcnt, T.dsym, T.dfast, KDF_INF_DBITS, 0, T.work)) return KDF_INF_CODES;
            uint32_t i = 0, prev = 0;
            uint8_t *run = T.lens;                                           // (the built code-length code no longer reads T.lens; uniform stores)
            while (i < nlen + ndist) {                                       // a repeat may run from the lengths into the distances
                uint32_t s;
                if (!kdf_inf_symbol(b, T.dfast, KDF_INF_DBITS, T.dcnt, T.dsym, s, st)) return st;
                if (s < 16) { run[i++] = (uint8_t)s; prev = s; continue; }
                uint32_t rep, val = 0;
                if (s == 16) { if (i == 0) return KDF_INF_CODES; if (!kdf_inf_take(b, 2, rep)) return KDF_INF_TRUNCATED; rep += 3; val = prev; }
                else if (s == 17) { if (!kdf_inf_take(b, 3, rep)) return KDF_INF_TRUNCATED; rep += 3; }
                else { if (!kdf_inf_take(b, 7, rep)) return KDF_INF_TRUNCATED; rep += 11; }
                if (i + rep > nlen + ndist) return KDF_INF_CODES;
                while (rep--) run[i++] = (uint8_t)val;
                prev = val;
            }
            L.sync();
            if (run[256] == 0) return KDF_INF_CODES;                         // no end-of-block code
            if (!kdf_inf_build(L, T.lens, nlen, T.lcnt, T.lsym, T.lfast, KDF_INF_LBITS, 1, T.work)) return KDF_INF_CODES;
            if (!kdf_inf_build(L, T.lens + nlen, ndist, T.dcnt, T.dsym, T.dfast, KDF_INF_DBITS, 2, T.work)) return KDF_INF_CODES;
        }
        for (;;) {                                                           // the symbol loop: >= 1 input bit per turn
            uint32_t s;
            if (!kdf_inf_symbol(b, T.lfast, KDF_INF_LBITS, T.lcnt, T.lsym, s, st)) return st;
            if (s < 256) {
                if (pos >= out_len) return KDF_INF_SIZE;
                if (L.id() == 0) out[pos] = (uint8_t)s;
                ++pos;
                continue;
            }
            if (s == 256) break;
            s -= 257;
            if (s >= 29) return KDF_INF_SYMBOL;
            uint32_t len = lbase[s], dist, ds;
            if (lext[s]) { if (!kdf_inf_take(b, lext[s], v)) return KDF_INF_TRUNCATED; len += v; }
            if (!kdf_inf_symbol(b, T.dfast, KDF_INF_DBITS, T.dcnt, T.dsym, ds, st)) return st;
            if (ds >= 30) return KDF_INF_SYMBOL;
            dist = dbase[ds];
            if (dext[ds]) { if (!kdf_inf_take(b, dext[ds], v)) return KDF_INF_TRUNCATED; dist += v; }
            if (dist > pos) return KDF_INF_DISTANCE;
            if (len > out_len - pos) return KDF_INF_SIZE;
            L.sync();                                                        // (the bytes behind pos are written)
            const uint8_t *src = out + (pos - dist);
            if (dist >= len) { for (uint32_t i = L.id(); i < len; i += L.count()) out[pos + i] = src[i]; }
            else { for (uint32_t i = L.id(); i < len; i += L.count()) out[pos + i] = src[i % dist]; }
            L.sync();
            pos += len;
        }
    } while (!last);
    return pos == out_len ? KDF_INF_OK : KDF_INF_SIZE;
}
