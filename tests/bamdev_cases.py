"""Shared inputs of the device BAM feeder's tests: DEFLATE payloads made by zlib, hand-made legal ones that zlib's encoder
never writes (tests/deflate_writer.py), a short fixed list of corrupt ones, seeded mutants judged by zlib, a BGZF writer with chosen block cuts, the stand-alone decoder program, and a Python restatement of the record walk
(written from the contract in include/kdf.h, "device BAM feeder")."""
import functools
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np

import deflate_writer as dw
from conftest import ROOT
from deflate_writer import Block

NT16 = "=ACMGRSVTWYHKDBN"


# ---- DEFLATE payloads -----------------------------------------------------------------------------------------------------
def deflate(data: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=8) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    return c.compress(data) + c.flush()


def _bam_like(rng, n):
    """Bytes with the texture of BAM records: names, 4-bit sequence, runs of qualities."""
    out = bytearray()
    i = 0
    while len(out) < n:
        out += struct.pack("<iiI", 380, 1, 10_000 + 37 * i)
        out += b"read_%07d\0" % i
        out += rng.integers(0, 256, 75, dtype=np.uint8).tobytes()
        out += bytes(rng.choice(np.array([2, 11, 25, 37], np.uint8), 150, p=[.05, .1, .25, .6]))
        i += 1
    return bytes(out[:n])


def valid_payloads():
    """[(label, payload, inflated)]: what zlib makes of the issue's list -- levels 0 / 1 / 6 / 9, the four strategies,
    incompressible bytes, one byte 65280 times, an empty block; blocks of 65280 bytes hold several DEFLATE blocks."""
    rng = np.random.default_rng(20240611)
    text = _bam_like(rng, 65280)
    noise = rng.integers(0, 256, 65280, dtype=np.uint8).tobytes()
    far = noise[:300] + bytes(32768 - 300) + noise[:300] + b"xyz" * 1000      # a match at distance 32768, overlapping copies
    out = []
    for level in (0, 1, 6, 9):
        out.append((f"text-l{level}", deflate(text, level), text))
    for name, strat in (("fixed", zlib.Z_FIXED), ("huffman", zlib.Z_HUFFMAN_ONLY), ("rle", zlib.Z_RLE), ("filtered", zlib.Z_FILTERED)):
        out.append((f"text-{name}", deflate(text, 6, strat), text))
    out.append(("noise-l6", deflate(noise, 6), noise))
    out.append(("noise-l0", deflate(noise, 0), noise))
    out.append(("run-l6", deflate(b"A" * 65280, 6), b"A" * 65280))            # matches of length 258, distance 1
    out.append(("run-l1-mem1", deflate(b"A" * 65280, 1, mem_level=1), b"A" * 65280))
    out.append(("far-l9", deflate(far, 9), far))
    out.append(("short-fixed", deflate(b"hello hello hello", 6, zlib.Z_FIXED), b"hello hello hello"))
    out.append(("one-byte", deflate(b"Q", 9), b"Q"))
    out.append(("empty", deflate(b"", 6), b""))
    out.append(("text-l6-mem1", deflate(text, 6, mem_level=1), text))           # a new DEFLATE block every few hundred symbols
    return out


def corrupt_payloads():
    """The short fixed list of corrupt blocks the GPU tests may use: [(label, payload, isize)].  tests/test_inflate_core.py
    shows on the CPU, under sanitizers, that the decoder rejects each of them cleanly."""
    v = {l: (p, d) for l, p, d in valid_payloads()}
    out = []
    p, d = v["noise-l0"]
    out.append(("stored-nlen-swapped", p[:1] + p[3:5] + p[1:3] + p[5:], len(d)))
    p, d = v["text-l6"]
    out.append(("truncated-half", p[:len(p) // 2], len(d)))
    out.append(("truncated-3-bytes", p[:3], len(d)))
    out.append(("isize-short", p, len(d) - 1))
    out.append(("isize-long", p, len(d) + 1))
    out.append(("btype-3", bytes([p[0] | 0x06]) + p[1:], len(d)))
    # a fixed-code block: literal 'a', then a match of length 3 at distance 3 -- two bytes before the start of the output
    bits = [1, 1, 0] + _msb(0x30 + ord("a"), 8) + _msb(1, 7) + _msb(2, 5) + _msb(0, 7)
    out.append(("distance-too-far", _pack_bits(bits), 4))
    out.append(("empty-payload", b"", 17))
    return out + illegal_neighbours()


def illegal_neighbours():
    """[(label, payload, isize)]: streams one step outside the hand-made legal ones.  zlib refuses each as invalid (asserted
    here); eight zero bytes behind each keep "the payload ends" from being the reason."""
    A, B = ord("a"), ord("b")
    ll = _lens(261, {A: 3, B: 2, 256: 3, 257: 3, 258: 3, 259: 3, 260: 3})
    head = dw.rle(ll[:256])
    toks = [A, B, B, A, (3, 1)]
    two = _lens(257, {A: 1, 256: 1})
    blocks = [
        ("repeat-overruns-nlen-plus-ndist", Block("dynamic", toks, True, cl=head + [3, (16, 6), 3, (16, 6)], nlen=261, ndist=8)),
        ("repeat-is-the-first-length", Block("dynamic", [3], True, cl=[(16, 3)] + dw.rle(_lens(254, {0: 1, 253: 1})), nlen=257, ndist=1)),
        ("two-distance-codes-incomplete", Block("dynamic", [A, (3, 1)], True, litlen=_lens(258, {A: 2, 256: 2, 257: 1}), dist=[1, 2])),
        ("literal-length-code-over-subscribed", Block("dynamic", [A, B], True, litlen=_lens(257, {A: 1, B: 1, 256: 1}), dist=[0])),
        ("no-code-for-256", Block("dynamic", [A, B], True, litlen=_lens(257, {A: 1, B: 1}), dist=[0], eob=False)),
        ("fixed-symbol-286", Block("fixed", [A, ("L", 286)], True)),
        ("fixed-symbol-287", Block("fixed", [A, ("L", 287)], True)),
        ("fixed-distance-symbol-30", Block("fixed", [A, B, A, ("D", 3, 30)], True)),
        ("fixed-distance-symbol-31", Block("fixed", [A, B, A, ("D", 3, 31)], True)),
        ("nlen-287", Block("dynamic", [A], True, litlen=two + [0] * 30, dist=[0])),
        ("ndist-31", Block("dynamic", [A], True, litlen=two, dist=[1, 1] + [0] * 29)),
    ]
    return [(label, dw.illegal(dw.deflate_blocks([blk]) + bytes(8)), 6) for label, blk in blocks]


# ---- DEFLATE payloads zlib's encoder never writes ---------------------------------------------------------------------------
def _case(label, blocks, tail=b""):
    payload = dw.deflate_blocks(blocks) + tail
    return (label, payload, dw.legal(payload))


def _lens(size, table):
    out = [0] * size
    for s, l in table.items():
        out[s] = l
    return out


def _repeat_cases():
    """Code-length repeats at and across the border between the two arrays.  The literal/length code is 'a' 3, 'b' 2, 256 3,
    257..260 3; the distance code is eight codes of 3 bits: seven equal lengths on either side of the border."""
    A, B = ord("a"), ord("b")
    ll = _lens(261, {A: 3, B: 2, 256: 3, 257: 3, 258: 3, 259: 3, 260: 3})
    dl = [3] * 8
    toks = [A, B, B, A, A, B, A, B, (3, 1), (4, 2), (5, 3), (6, 4), (3, 5), (4, 6), (5, 7), (6, 8), B]
    head = dw.rle(ll[:256])
    out = [_case("repeat-crosses-16", [Block("dynamic", toks, True, cl=head + [3, (16, 6), (16, 6)], nlen=261, ndist=8)]),
           _case("repeat-coded-apart", [Block("dynamic", toks, True, litlen=ll, dist=dl, joint=False)]),
           _case("repeat-coded-jointly", [Block("dynamic", toks, True, litlen=ll, dist=dl, joint=True)]),
           # the repeat ends exactly on nlen; the distance lengths then open with a repeat of the length before the border
           _case("repeat-ends-on-nlen", [Block("dynamic", toks, True, cl=head + [3, (16, 4), (16, 6), 3, 3], nlen=261, ndist=8)]),
           _case("repeat-ends-on-nlen-plus-ndist", [Block("dynamic", toks, True, cl=head + [3, 3, 3, 3, 3, 3, 3, (16, 6)], nlen=261, ndist=8)])]
    assert all(d == out[0][2] for _, _, d in out)
    # zero runs across the border: 17 covers 258..263 and distance symbols 0..3; 18 covers 258..269 and 0..9
    ll = _lens(264, {A: 2, B: 2, 256: 2, 257: 2})
    toks = [A, B, B, A, B, A, A, A, (3, 5), (3, 6), (3, 7), (3, 8), B]
    out.append(_case("repeat-crosses-17", [Block("dynamic", toks, True, cl=dw.rle(ll[:258]) + [(17, 10), 1, 1], nlen=264, ndist=6)]))
    toks = [A, B] * 32 + [(3, 33), (3, 48), (3, 49), (3, 64), A]
    out.append(_case("repeat-crosses-18", [Block("dynamic", toks, True, cl=dw.rle(ll[:258]) + [(18, 22), 1, 1], nlen=270, ndist=12)]))
    return out


def _one_code_cases():
    A, B = ord("a"), ord("b")
    ll = _lens(258, {A: 2, 256: 2, 257: 1})
    out = [_case("one-distance-code-symbol-0", [Block("dynamic", [A, (3, 1), (3, 1)], True, litlen=ll, dist=[1])])]
    ll = _lens(258, {A: 2, B: 3, 256: 3, 257: 1})
    toks = [A, B] * 16 + [(3, 25), (3, 32), (3, 28)]
    blk = Block("dynamic", toks, True, litlen=ll, dist=[0] * 9 + [1], joint=False)
    assert blk.cl[-2:] == [(17, 9), 1]                                   # the zero lengths before it are one run
    out.append(_case("one-distance-code-symbol-9", [blk]))
    out.append(_case("no-distance-code", [Block("dynamic", [A, B, B, A], True, litlen=_lens(257, {A: 2, B: 2, 256: 1}), dist=[0])]))
    out.append(_case("eob-only", [Block("dynamic", [], False, litlen=_lens(257, {256: 1}), dist=[0]), Block("fixed", [A, B, (5, 2)], True)]))
    return out


def _long_code_cases():
    """Code lengths 1, 2, ..., 14, 15, 15 on sixteen symbols of either alphabet; every code is used."""
    rng = np.random.default_rng(1951)
    lits = [ord(c) for c in "acgtnACGTN=\0"]
    # (a permutation, so that literals, the end code and the length symbols each get short and long codes)
    lsyms = [lits[0], 257, lits[1], lits[2], 264, lits[3], lits[4], lits[5], 256, lits[6], lits[7], 270, lits[8], lits[9], lits[10], lits[11]]
    ll = _lens(271, dict(zip(lsyms, list(range(1, 16)) + [15])))
    dl = [6, 1, 9, 2, 12, 3, 15, 4, 10, 5, 15, 7, 13, 8, 14, 11]
    toks = [int(x) for x in rng.choice(lits, 160)] + lits + [int(x) for x in rng.choice(lits, 96)]
    for ds in range(16):
        for i, d in enumerate((dw.DBASE[ds], dw.DBASE[ds] + (1 << dw.DEXT[ds]) - 1)):
            toks += [((3, 10, 23, 26)[(2 * ds + i) % 4], d), int(rng.choice(lits))]
    first = Block("dynamic", toks, False, litlen=ll, dist=dl)
    # every USED code is behind the fast tables: literal/length codes of 11 bits and more, distance codes of 9 and more
    x, y = ord("x"), ord("y")
    ll2 = _lens(260, {**{s: s + 1 for s in range(10)}, x: 11, y: 12, 256: 13, 257: 14, 258: 15, 259: 15})
    dl2 = list(range(1, 16)) + [15]
    toks2 = [x, y, y, x, x, x, y, x]
    for ds in range(8, 16):
        toks2 += [(3 + ds % 3, dw.DBASE[ds]), y, (3 + (ds + 1) % 3, dw.DBASE[ds] + (1 << dw.DEXT[ds]) - 1), x]
    return [_case("lengths-1-to-15", [first, Block("dynamic", toks2, True, litlen=ll2, dist=dl2)]),
            _case("lengths-all-behind-the-fast-tables", [Block("stored", data=bytes(rng.integers(0, 256, 300, dtype=np.uint8))),
                                                         Block("dynamic", toks2, True, litlen=ll2, dist=dl2)])]


def _extra_bit_tokens(rng, fill_to):
    """Literals and matches up to `fill_to` bytes of output, then every length symbol and every distance symbol with its
    extra bits all zero and all one (length 258 once more at the end)."""
    toks, n = [int(x) for x in rng.integers(0, 256, 300)], 300
    while n + 258 + 7 <= fill_to:
        toks += [(258, 300)] + [int(x) for x in rng.integers(0, 256, 7)]
        n += 265
    toks += [int(x) for x in rng.integers(0, 256, fill_to - n)]
    for s in range(28):
        for length in (dw.LBASE[s], dw.LBASE[s] + (1 << dw.LEXT[s]) - 1):
            toks += [(length, 299), int(rng.integers(0, 256))]
    for s in range(30):
        for d in (dw.DBASE[s], dw.DBASE[s] + (1 << dw.DEXT[s]) - 1):
            if d <= fill_to:
                toks += [(3 + s % 6, d), int(rng.integers(0, 256))]
    return toks + [(258, 77)]


def _extra_bits_cases():
    rng = np.random.default_rng(284)
    out = [_case("len-258-as-284", [Block("fixed", [7, 8, 9, (258, 3), (258, 1), (257, 2), (258, 258)], True, use_284=True)]),
           _case("len-258-as-285", [Block("fixed", [7, 8, 9, (258, 3), (258, 1), (257, 2), (258, 258)], True)])]
    assert out[0][2] == out[1][2] and out[0][1] != out[1][1]
    out.append(_case("extra-bits-both-ends-fixed", [Block("fixed", _extra_bit_tokens(rng, 4096), True, use_284=True)]))
    # the one output above 32 KB: distance 32768 = symbol 29 with all thirteen extra bits set.  Both alphabets at their full
    # size (nlen 286 with 285 used, ndist 30 with 29 used): 226 codes of 8 bits and 60 of 9; 2 codes of 4 bits and 28 of 5
    toks = _extra_bit_tokens(rng, 32768)
    assert (3 + 29 % 6, 32768) in toks and (258, 77) in toks
    out.append(_case("extra-bits-both-ends-nlen-286-ndist-30", [
        Block("dynamic", toks, False, litlen=[8] * 226 + [9] * 60, dist=[4] * 2 + [5] * 28),
        Block("fixed", [(258, 32768), (227, 24577), 1], True, use_284=True)]))
    assert 32768 < len(out[-1][2]) < 40000
    return out


EVERY_DISTANCE = list(range(1, 131)) + [191, 192, 193, 255, 256, 257]


def _distance_cases():
    """For every distance d around the lane count: one literal, then matches at distance d shorter than, as long as and
    longer than d.  In fixed blocks, several payloads of under 20 KB of output each."""
    rng = np.random.default_rng(64)
    out, toks, n, lo = [], None, 0, None
    for d in EVERY_DISTANCE + [None]:
        if d is None or (toks is not None and n + 6 * d + 270 > 20000):
            out.append(_case(f"every-distance-{lo}-to-{prev}", [Block("fixed", toks, True)]))
            toks = None
        if d is None:
            break
        if toks is None:
            toks, lo = [int(x) for x in rng.integers(0, 256, d - 1)], d
            n = d - 1
        toks.append(int(rng.integers(0, 256)))
        n += 1
        for length in (3, d - 1, d, d + 1, 2 * d + 1, 258):
            if 3 <= length <= 258:
                toks.append((length, d))
                n += length
        prev = d
    return out


def _chain_cases():
    """Runs of matches with no literal between them; each reads bytes that the match before it wrote (its distance is at
    most that match's length), so a lane reads what another lane stored one copy earlier."""
    rng = np.random.default_rng(6464)
    out = []
    for label, dists in (("match-chains-below-64", list(range(1, 64))), ("match-chains-at-64", [64]), ("match-chains-above-64", list(range(65, 200))),
                         ("match-chains-mixed", [1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193])):
        toks, n = [int(x) for x in rng.integers(0, 256, 258)], 258
        while n < 14000:
            plen = 258                                                   # (the literals before the chain count as its first link)
            for _ in range(int(rng.integers(2, 12))):
                ok = [d for d in dists if d <= plen]
                d = int(rng.choice(ok)) if ok else min(dists)
                length = int(rng.choice([3, 4, d - 1, d, d + 1, 2 * d - 1, 2 * d, 2 * d + 1, 63, 64, 65, 258, int(rng.integers(3, 259))]))
                length = min(max(length, 3), 258)
                toks.append((length, d))
                n += length
                plen = length
            toks.append(int(rng.integers(0, 256)))
            n += 1
        out.append(_case(label, [Block("fixed", toks, True)]))
    return out


def flush_payload():
    """What zlib writes around Z_SYNC_FLUSH and Z_FULL_FLUSH: empty stored blocks at odd bit positions between Huffman blocks"""
    rng = np.random.default_rng(3)
    text = _bam_like(rng, 6000)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    p = c.compress(text[:1000]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(text[1000:1003]) + c.flush(zlib.Z_SYNC_FLUSH)
    p += c.compress(text[1003:4000]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(text[4000:]) + c.flush()
    return p, text


def _simple_dynamic(tokens, last=False):
    """A dynamic block with balanced complete codes over the symbols the tokens use"""
    ls, ds = {256, 257}, set()
    for t in tokens:
        if isinstance(t, int):
            ls.add(t)
        else:
            ls.add(dw._length_symbol(t[0], False)[0])
            ds.add(dw._distance_symbol(t[1])[0])
    ds |= {0, 1} if ds else set()
    return Block("dynamic", tokens, last, litlen=dw.lengths_for(ls, max(ls) + 1), dist=dw.lengths_for(ds, max(ds) + 1) if ds else [0])


def _stored_cases():
    rng = np.random.default_rng(8)
    out = []
    for k in range(8):
        # a fixed block is 3 + 7 bits and 8 bits a literal below 144, 9 bits one above: (k - 2) mod 8 of the latter
        first = [int(x) for x in rng.integers(0, 144, 40)] + [int(x) for x in rng.integers(144, 256, (k - 2) % 8)]
        data = bytes(rng.integers(0, 256, 11 + k, dtype=np.uint8))
        blocks = [Block("fixed", first), Block("stored", data=data), Block("fixed", [5, (30, len(data) + 20), (4, 3), 6], True)]
        starts = []
        dw.deflate_blocks(blocks, starts)
        assert starts[1] % 8 == k
        out.append(_case(f"huffman-stored-huffman-bit-{k}", blocks))
    p, text = flush_payload()
    assert dw.legal(p) == text
    out.append(("zlib-sync-and-full-flush", p, text))
    out.append(_case("empty-stored-blocks", [Block("fixed", [1, 2, 3]), Block("stored"), Block("stored"), Block("fixed", [(5, 3), 4]),
                                             Block("fixed", []), _simple_dynamic([]), Block("stored", data=b"xy"), Block("stored", last=True)]))
    blocks = []
    for i in range(501):
        r = int(rng.integers(0, 256))
        toks = [r, (i + 1) & 255] + ([(3 + i % 20, 1 + i % min(2 * len(blocks) + 1, 900))] if blocks else [])
        blocks.append(Block("stored", data=bytes([r, i & 255, 0][:i % 4])) if i % 3 == 0 else Block("fixed", toks) if i % 3 == 1 else _simple_dynamic(toks))
    blocks[-1].last = True
    out.append(_case("many-blocks", blocks))
    return out


def _tail_cases():
    """Payloads of 3 to 9 bytes (the bit reader's byte-wise refill).  From 4 bytes on the last code ends on the last bit: a
    fixed block of n literals and a match of length 19 at distance 1 is 24 + 8 n bits.  No stream with any output is
    shorter than 18 bits, and none of exactly 24 bits exists, so the 3-byte stream ends on 6 bits of padding."""
    out = [_case("tail-3-bytes", [Block("fixed", [65], True)])]
    for n in range(1, 7):
        blocks = [Block("fixed", list(range(66, 66 + n)) + [(19, 1)], True)]
        assert dw.bit_length(blocks) == 24 + 8 * n
        out.append(_case(f"tail-bits-{3 + n}-bytes", blocks))
        assert len(out[-1][1]) == 3 + n
    blocks = [Block("fixed", [200, 201, 202, 203, 204, 205], True)]           # six literals of 9 bits: 64 bits
    assert dw.bit_length(blocks) == 64
    out.append(_case("tail-bits-8-bytes-9-bit-codes", blocks))
    out.append(_case("trailing-bytes-after-the-final-block", [Block("fixed", [1, 2, (9, 2)], True)], tail=b"\xde\xad\xbe\xef" * 3))
    return out


@functools.lru_cache(maxsize=None)
def _handmade():
    out = (_repeat_cases() + _one_code_cases() + _long_code_cases() + _extra_bits_cases() + _distance_cases() + _chain_cases()
           + _stored_cases() + _tail_cases())
    assert len({l for l, _, _ in out}) == len(out)
    assert all(0 < len(d) <= 65536 for _, _, d in out)
    assert all(len(d) < 20000 for l, _, d in out if not l.startswith("extra-bits-both-ends-nlen-286"))
    return tuple(out)


def handmade_payloads():
    """[(label, payload, inflated)]: legal DEFLATE that zlib's encoder never writes (tests/deflate_writer.py), one feature
    per label.  Every `inflated` is what zlib's inflate makes of the payload, never what the writer meant."""
    return list(_handmade())


# ---- mutants, judged by zlib --------------------------------------------------------------------------------------------------
MUTANTS, MUTANT_SEED = 30_000, 1951


def mutation_bases():
    """[(payload, inflated)]: the hand-made streams of under 20 KB of output and the zlib-made ones of at most 4 KB"""
    return ([(p, d) for _, p, d in handmade_payloads() if len(d) < 20000]
            + [(p, d) for _, p, d in valid_payloads() if len(d) <= 4096] + [flush_payload()])


def zlib_verdict(payload):
    """zlib's output if it reaches the end of the stream with 1 to 65536 bytes, else None"""
    z = zlib.decompressobj(-15)
    try:
        out = z.decompress(payload, 65537)
    except zlib.error:
        return None
    return out if z.eof and 1 <= len(out) <= 65536 else None


def mutants(n=MUTANTS, seed=MUTANT_SEED):
    """Yields n cases (payload, isize, expected bytes or None) in a fixed order: a base stream with 1 to 3 bits flipped in
    its first 200 bytes.  zlib judges each: where it reaches the end of the stream with 1 to 65536 bytes the mutant is
    a VALID block whose bytes and ISIZE are zlib's; otherwise it is an invalid one (ISIZE: the base's)."""
    bases = mutation_bases()
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(bases), n)
    flips = rng.integers(1, 4, n)
    where = rng.integers(0, 1 << 30, (n, 3))
    for i in range(n):
        p, d = bases[int(pick[i])]
        m = bytearray(p)
        for j in range(int(flips[i])):
            bit = int(where[i, j]) % (8 * min(len(p), 200))
            m[bit >> 3] ^= 1 << (bit & 7)
        m = bytes(m)
        want = zlib_verdict(m)
        yield (m, len(want), want) if want is not None else (m, max(len(d), 1), None)


def _msb(code, n):
    return [(code >> (n - 1 - i)) & 1 for i in range(n)]


def _pack_bits(bits):
    bits = bits + [0] * (-len(bits) % 8)
    return bytes(sum(bits[i + j] << j for j in range(8)) for i in range(0, len(bits), 8))


# ---- the stand-alone decoder program ----------------------------------------------------------------------------------------
def build_inflate_check(tmpdir) -> str:
    """Compile tests/native/inflate_check.cpp for the host with sanitizers -- g++, or hipcc's host compiler where there is
    no g++ -- and return the program's path.  No compiler at all is an error, not a skip: the program is the cap that keeps
    the zlib fallback from hiding a broken decoder."""
    exe = os.path.join(str(tmpdir), "inflate_check")
    src = os.path.join(ROOT, "tests", "native", "inflate_check.cpp")
    inc = os.path.join(ROOT, "kmer_denovo_filter_amd", "csrc")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{inc}", src, "-o", exe]
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    if shutil.which("g++"):
        cmd = ["g++"] + flags
    elif hipcc:
        cmd = [hipcc, "-x", "c++"] + flags                             # host only: no device pass
    else:
        raise RuntimeError("neither g++ nor hipcc: the decoder's CPU program cannot be built")
    subprocess.run(cmd, check=True)
    return exe


def run_inflate_check(exe, cases, tmpdir, n_fuzz=0):
    """cases: [(payload, isize, expected bytes or None)] -> ([(status, equal)], (rejected, accepted), CompletedProcess)."""
    path = os.path.join(str(tmpdir), "cases.bin")
    with open(path, "wb") as f:
        for payload, isize, want in cases:
            f.write(struct.pack("<III", len(payload), isize, 1 if want is not None else 0))
            f.write(payload)
            if want is not None:
                f.write(want)
    pr = subprocess.run([exe, path, str(n_fuzz)], capture_output=True, text=True)
    res, fuzz = [], None
    for line in pr.stdout.splitlines():
        w = line.split()
        if w and w[0] == "case":
            res.append((int(w[3]), int(w[5])))
        elif w and w[0] == "fuzz":
            fuzz = (int(w[3]), int(w[5]))
    return res, fuzz, pr


# ---- BGZF / BAM writers -----------------------------------------------------------------------------------------------------
def bgzf_block(payload: bytes, isize: int, crc: int = 0, extra_before: bytes = b"") -> bytes:
    """One BGZF block around a raw DEFLATE payload; extra_before: further gzip subfields ahead of BC."""
    xlen = len(extra_before) + 6
    bsize = 12 + xlen + len(payload) + 8 - 1
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", xlen) + extra_before + b"BC\x02\0" + struct.pack("<H", bsize)
            + payload + struct.pack("<II", crc, isize))


BGZF_EOF = bgzf_block(deflate(b""), 0)


def write_bgzf(path, data: bytes, cuts=None, block=65280, level=6, empty_after=()):
    """data as BGZF blocks cut at the byte offsets `cuts` (default: every `block` bytes); empty_after: indices of blocks
    after which an empty block (ISIZE 0) is written.  Ends with the EOF marker.  Returns the block start offsets in data."""
    if cuts is None:
        cuts = list(range(block, len(data), block))
    edges = [0] + sorted(c for c in set(cuts) if 0 < c < len(data)) + [len(data)]
    with open(path, "wb") as f:
        for i in range(len(edges) - 1):
            piece = data[edges[i]:edges[i + 1]]
            f.write(bgzf_block(deflate(piece, level), len(piece), zlib.crc32(piece)))
            if i in empty_after:
                f.write(BGZF_EOF)
        f.write(BGZF_EOF)
    return edges[:-1]


def bam_header(refs=(("chr1", 1_000_000),)) -> bytes:
    text = "@HD\tVN:1.6\tSO:unsorted\n" + "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in refs)
    out = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(refs))
    for n, l in refs:
        out += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", l)
    return out


def bam_record(name: str, flag: int, seq: str, qual=True, pos=100, tags: bytes = b"") -> bytes:
    """One alignment record (unaligned CIGAR-less form; qual False: the 0xFF filler of a record without qualities)."""
    l = len(seq)
    codes = [NT16.index(c) for c in seq.upper()]
    if l & 1:
        codes.append(0)
    sq = bytes((codes[i] << 4) | codes[i + 1] for i in range(0, len(codes), 2))
    ql = (bytes([30]) * l) if qual else (b"\xff" * l)
    body = struct.pack("<iiBBHHHiiii", 0, pos, len(name) + 1, 60, 4680, 0, flag, l, -1, -1, 0) + name.encode() + b"\0" + sq + ql + tags
    return struct.pack("<i", len(body)) + body


def synthetic_bam(tmp_path, n_runs=300, block=700):
    """Runs of two to four records (a supplementary and sometimes a secondary ahead of READ1 and READ2, reads of 0 to 89
    bases with N) in BGZF blocks of `block` bytes, two empty blocks in mid-file."""
    rng = np.random.default_rng(7)
    data = bytearray(bam_header())
    for i in range(n_runs):
        name = f"pair{i:05d}"
        seqs = ["".join(rng.choice(list("ACGTN"), int(rng.integers(0, 90)), p=[.24, .24, .24, .24, .04])) for _ in range(4)]
        data += bam_record(name, 0x900 | 0x40, seqs[0], qual=False)          # a supplementary: flagged off inside the run
        data += bam_record(name, 0x100 | 0x40, seqs[1], qual=False) if i % 3 == 0 else b""
        data += bam_record(name, 0x40, seqs[2])
        data += bam_record(name, 0x80, seqs[3])
    path = str(tmp_path / "syn.bam")
    write_bgzf(path, bytes(data), block=block, empty_after=(5, 40))
    return path


# ---- the walk, restated -------------------------------------------------------------------------------------------------------
def walk(buf: bytes, start: int, stop, flag_off: int, collapse: bool, at_eof: bool):
    """Records of one sub-range of an inflated span -> (sequences, finished).  start: offset of the first record; stop:
    offset of the end zone (None: the file's end); at_eof: the span ends where the file ends.  Sequences are strings
    over ACGT and N (anything else reads as N, as the stream's invalid mask)."""
    out = []
    best = [None, None, None]
    score = [-1, -1, -1]
    run = None

    def flush():
        for i in range(3):
            if score[i] >= 0:
                out.append(best[i])
                score[i] = -1

    q = start
    while True:
        if len(buf) - q < 4:
            if not at_eof:
                return out, False
            break
        bs = struct.unpack_from("<i", buf, q)[0]
        assert bs >= 32
        if len(buf) - q < 4 + bs:
            assert not at_eof, "truncated record"
            return out, False
        p = q + 4
        l_rn = buf[p + 8]
        n_cig, flag, l_seq = struct.unpack_from("<HHi", buf, p + 12)
        zone = stop is not None and q >= stop
        if zone and not collapse:
            return out, True
        q += 4 + bs
        if flag & flag_off:
            continue
        so = p + 32 + l_rn + 4 * n_cig
        nib = np.frombuffer(buf, np.uint8, (l_seq + 1) // 2, so)
        codes = np.stack([nib >> 4, nib & 15], 1).reshape(-1)[:l_seq]
        seq = "".join("ACGT"[{1: 0, 2: 1, 4: 2, 8: 3}[c]] if c in (1, 2, 4, 8) else "N" for c in codes.tolist())
        if not collapse:
            out.append(seq)
            continue
        name = buf[p + 32:p + 32 + max(l_rn - 1, 0)]
        if run is None or name != run:
            if run is not None:
                flush()
            if zone:
                return out, True
            run = name
        r1, r2 = bool(flag & 0x40), bool(flag & 0x80)
        part = 1 if (r1 and not r2) else 2 if (r2 and not r1) else 0
        sc = 2 if (l_seq > 0 and buf[so + (l_seq + 1) // 2] != 0xFF) else 1
        if sc > score[part]:
            best[part], score[part] = seq, sc
    if run is not None:
        flush()
    return out, True


def stream_reads(st):
    """ReadStream -> list of strings over ACGT / N (the separator after each read dropped)."""
    n = st.n_bases
    pk = np.asarray(st.packed, np.uint64)
    iv = np.asarray(st.invalid, np.uint64)
    pos = np.arange(n, dtype=np.uint64)
    codes = ((pk[pos >> np.uint64(5)] >> ((pos & np.uint64(31)) * np.uint64(2))) & np.uint64(3)).astype(np.uint8)
    bad = ((iv[pos >> np.uint64(6)] >> (pos & np.uint64(63))) & np.uint64(1)).astype(bool)
    asc = np.frombuffer(b"ACGT", np.uint8)[codes]
    asc[bad] = ord("N")
    s = asc.tobytes().decode()
    off = [int(x) for x in st.offsets]
    return [s[off[i]:off[i + 1] - 1] for i in range(len(off) - 1)]
