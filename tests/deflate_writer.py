"""A token-level DEFLATE writer for the tests, written from RFC 1951 (section 3.2).  It writes what the caller says,
legal or not: blocks of chosen types, chosen tokens, and for a dynamic block chosen code lengths and a chosen run-length
coding of them -- the streams zlib's own encoder never makes.

The writer is NOT a reference.  The truth about every payload it makes is zlib's inflate: legal(payload) returns what
zlib decodes (and asserts that zlib reached the end of the stream), illegal(payload) asserts that zlib refuses it.

Tokens of a block:
    int 0..255                 a literal
    (length, distance)         a match, 3 <= length <= 258, 1 <= distance <= 32768
    ("L", symbol)              a raw literal/length symbol, no extra bits (for the symbols no stream may use)
    ("D", length, dsymbol)     a match whose distance is written as a raw distance symbol, no extra bits
The code lengths of a dynamic block, as written into its header, are a list of
    int 0..15                  one length
    (16 | 17 | 18, count)      a repeat: 16 the previous length 3..6 times, 17 zero 3..10 times, 18 zero 11..138 times
"""
import zlib

# RFC 1951 3.2.5: extra bits of the length symbols 257..285 and of the distance symbols 0..29; the bases follow from them
LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
LBASE = [3 + sum(1 << e for e in LEXT[:i]) for i in range(28)] + [258]
DEXT = [0] * 4 + [e for e in range(1, 14) for _ in (0, 1)]
DBASE = [1 + sum(1 << e for e in DEXT[:i]) for i in range(30)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]      # 3.2.7
FIXED_LITLEN = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8                          # 3.2.6
FIXED_DIST = [5] * 32


class BitWriter:
    """Bits go into bytes from the least significant bit up; a Huffman code goes in most significant bit first."""

    def __init__(self):
        self.out, self.acc, self.k, self.n = bytearray(), 0, 0, 0       # whole bytes, the bits behind them, and the bit offset

    def bits(self, value, n):
        assert 0 <= value < (1 << n)
        self.acc |= value << self.k
        self.k += n
        self.n += n
        while self.k >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.k -= 8

    def code(self, code, n):
        self.bits(int(format(code, "0%db" % n)[::-1], 2), n)

    def align(self):
        self.bits(0, -self.n % 8)

    def raw(self, data: bytes):
        assert self.k == 0
        self.out += data
        self.n += 8 * len(data)

    def getvalue(self) -> bytes:
        return bytes(self.out) + (bytes([self.acc]) if self.k else b"")


def canonical(lengths):
    """{symbol: (code, length)} by the algorithm of 3.2.2; a length of 0 means no code.  Nothing is validated."""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 17
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, l in enumerate(lengths):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def balanced(n):
    """n >= 2 code lengths of a complete code, as equal as a complete code allows (the longer ones last)."""
    assert n >= 2
    k = (n - 1).bit_length()
    short = (1 << k) - n
    return [k - 1] * short + [k] * (n - short)


def lengths_for(symbols, size):
    """A complete balanced code for the given symbols (at least two) in an alphabet of `size`: every other length 0."""
    symbols = sorted(set(symbols))
    out = [0] * size
    for s, l in zip(symbols, balanced(len(symbols))):
        out[s] = l
    return out


def rle(lengths):
    """A greedy run-length coding of one sequence of code lengths (3.2.7)."""
    out, i = [], 0
    while i < len(lengths):
        v, j = lengths[i], i
        while j < len(lengths) and lengths[j] == v:
            j += 1
        run = j - i
        if v == 0 and run >= 3:
            take = min(run, 138)
            out.append((18 if take >= 11 else 17, take))
        elif v != 0 and run >= 4:
            out.append(v)
            take = 1 + min(run - 1, 6)
            out.append((16, take - 1))
        else:
            out.append(v)
            take = 1
        i += take
    return out


def expand(cl):
    """The code lengths that a coded sequence states."""
    out = []
    for x in cl:
        if isinstance(x, int):
            out.append(x)
        elif x[0] == 16:
            out += [out[-1] if out else 0] * x[1]
        else:
            out += [0] * x[1]
    return out


class Block:
    """One DEFLATE block.  kind: "stored" | "fixed" | "dynamic".

    stored:  data (bytes), at most 65535.
    dynamic: litlen and dist are the two code-length arrays as the header states them (nlen = len(litlen), ndist =
             len(dist)); joint: their run-length coding treats them as one sequence (repeats may cross) or as two; cl:
             the coded sequence itself, where the caller wants a particular one -- then litlen and dist are what it
             expands to, cut at nlen and nlen + ndist (by default 257.. and 1.. as far as the sequence reaches).
    use_284: length 258 is written as symbol 284 with extra bits 31, not as symbol 285.
    eob:     False leaves the end-of-block code out (for streams that are illegal before it)."""

    def __init__(self, kind, tokens=(), last=False, data=b"", litlen=None, dist=None, joint=True, cl=None, nlen=None, ndist=None,
                 use_284=False, eob=True):
        assert kind in ("stored", "fixed", "dynamic")
        self.kind, self.tokens, self.last, self.data = kind, list(tokens), last, bytes(data)
        self.joint, self.use_284, self.eob = joint, use_284, eob
        if kind == "dynamic":
            if cl is None:
                cl = rle(list(litlen) + list(dist)) if joint else rle(list(litlen)) + rle(list(dist))
                nlen, ndist = len(litlen), len(dist)
            else:
                assert nlen is not None and ndist is not None
                full = expand(cl)
                litlen, dist = full[:nlen], full[nlen:nlen + ndist]
            self.cl, self.nlen, self.ndist = list(cl), nlen, ndist
        if kind == "fixed":
            litlen, dist = FIXED_LITLEN, FIXED_DIST
        self.litlen, self.dist = litlen, dist


def _length_symbol(length, use_284):
    if length == 258:
        return (284, 31, 5) if use_284 else (285, 0, 0)
    s = max(i for i in range(28) if LBASE[i] <= length)
    assert length - LBASE[s] < (1 << LEXT[s])
    return 257 + s, length - LBASE[s], LEXT[s]


def _distance_symbol(distance):
    s = max(i for i in range(30) if DBASE[i] <= distance)
    assert distance - DBASE[s] < (1 << DEXT[s])
    return s, distance - DBASE[s], DEXT[s]


def _write_tokens(w, blk):
    lcode, dcode = canonical(blk.litlen), canonical(blk.dist)
    for t in blk.tokens:
        if isinstance(t, int):
            w.code(*lcode[t])
        elif t[0] == "L":
            w.code(*lcode[t[1]])
        else:
            raw = t[0] == "D"
            length, d = (t[1], t[2]) if raw else t
            s, extra, n = _length_symbol(length, blk.use_284)
            w.code(*lcode[s])
            w.bits(extra, n)
            ds, dextra, dn = (d, 0, 0) if raw else _distance_symbol(d)
            w.code(*dcode[ds])
            w.bits(dextra, dn)
    if blk.eob:
        w.code(*lcode[256])


def _write_dynamic_header(w, blk):
    used = sorted({x if isinstance(x, int) else x[0] for x in blk.cl})
    if len(used) < 2:                                              # the code-length code must be complete: two codes at least
        used = sorted(set(used) | {0 if used != [0] else 1})
    cll = lengths_for(used, 19)
    ncode = max(4, 1 + max(i for i, s in enumerate(CL_ORDER) if cll[s]))
    w.bits(blk.nlen - 257, 5)
    w.bits(blk.ndist - 1, 5)
    w.bits(ncode - 4, 4)
    for s in CL_ORDER[:ncode]:
        w.bits(cll[s], 3)
    code = canonical(cll)
    for x in blk.cl:
        if isinstance(x, int):
            w.code(*code[x])
        else:
            s, count = x
            w.code(*code[s])
            if s == 16:
                w.bits(count - 3, 2)
            elif s == 17:
                w.bits(count - 3, 3)
            else:
                w.bits(count - 11, 7)


def deflate_blocks(blocks, starts=None) -> bytes:
    """The raw payload of the blocks, in order.  starts: a list that receives each block header's bit offset."""
    w = BitWriter()
    for blk in blocks:
        if starts is not None:
            starts.append(w.n)
        w.bits(1 if blk.last else 0, 1)
        w.bits({"stored": 0, "fixed": 1, "dynamic": 2}[blk.kind], 2)
        if blk.kind == "stored":
            w.align()
            w.bits(len(blk.data), 16)
            w.bits(len(blk.data) ^ 0xFFFF, 16)
            w.raw(blk.data)
            continue
        if blk.kind == "dynamic":
            _write_dynamic_header(w, blk)
        _write_tokens(w, blk)
    return w.getvalue()


def bit_length(blocks) -> int:
    """Bits of the payload up to and including its last code (the padding of the last byte not counted)."""
    starts = []
    deflate_blocks(list(blocks) + [Block("fixed")], starts)
    return starts[-1]


def legal(payload: bytes) -> bytes:
    """What zlib inflates the payload to.  zlib must reach the end of the stream."""
    d = zlib.decompressobj(-15)
    out = d.decompress(payload)
    assert d.eof, "zlib does not reach the end of the stream"
    return out


def illegal(payload: bytes) -> bytes:
    """Asserts that zlib refuses the payload as invalid (not merely as cut short); returns the payload."""
    try:
        legal(payload)
    except zlib.error:
        return payload
    raise AssertionError("zlib accepts the payload, or only finds it too short")
