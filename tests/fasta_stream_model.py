"""A numpy MODEL of the device FASTA feeder (include/kdf.h "device FASTA feeder"), written from the header's text alone: no
engine, no library.  ``pack_chunk`` is kdf_fasta_pack* for one chunk; ``CASES`` is the case list the CPU and the GPU
tests share.

A stream is held as a uint8 array of CODES, one per position: 0 .. 3 = A C G T, 4 = invalid (N, IUPAC, a blank, an
interior CR, a separator).  ``to_words`` turns codes into the packed and mask words of the header's "Read streams".
"""
import os

import numpy as np

IN_RECORD, MID_LINE, IN_HEADER = 1, 2, 4
LF, CR, GT = 10, 13, 62

_CODE = np.full(256, 4, np.uint8)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _i


class State:
    """kdf_fasta_state"""

    def __init__(self, flags=0, records=0, positions=0):
        self.flags, self.records, self.positions = flags, records, positions

    def copy(self):
        return State(self.flags, self.records, self.positions)

    def __eq__(self, o):
        return (self.flags, self.records, self.positions) == (o.flags, o.records, o.positions)

    def __repr__(self):
        return f"State(flags={self.flags}, records={self.records}, positions={self.positions})"


class NoProgress(ValueError):
    """a non-empty chunk that is not the last and holds only CR: KDF_ERR_INVALID"""


def pack_chunk(text: bytes, final: bool, state: State, prev=None, carry: int = 0):
    """One call -> (codes of the call's stream, offsets int64[n_reads + 1], consumed, state afterwards).  ``prev``: the
    codes of the previous stream (None: none).  ``state`` is not modified."""
    t = np.frombuffer(bytes(text), np.uint8)
    n = len(t)
    if n == 0 and not final:
        return np.zeros(0, np.uint8), np.zeros(1, np.int64), 0, state.copy()
    in_rec0 = bool(state.flags & IN_RECORD)
    mid0 = bool(state.flags & MID_LINE)
    hdr0 = mid0 and bool(state.flags & IN_HEADER)
    c = min(carry, len(prev)) if (carry > 0 and prev is not None and len(prev) > 0 and in_rec0) else 0
    head = np.asarray(prev[len(prev) - c:], np.uint8) if c else np.zeros(0, np.uint8)
    # consumed: all of the last chunk, else all but the trailing run of CR
    m = n
    if not final:
        other = np.flatnonzero(t != CR)
        m = int(other[-1]) + 1 if len(other) else 0
        if m == 0:
            raise NoProgress("a chunk of CR only")
    t = t[:m]
    idx = np.arange(m)
    nl, cr = t == LF, t == CR
    ls = np.zeros(m, bool)                                   # line starts
    if m:
        ls[0] = not mid0
        ls[1:] = nl[:-1]
    hs = ls & (t == GT)                                      # header starts
    # the line of a byte: 0 = the line the chunk begins in the middle of
    line = np.cumsum(ls)
    first_is_hdr = np.concatenate(([hdr0], hs[ls]))
    in_hdr = first_is_hdr[line]
    # a CR is dropped iff only CR lie between it and the next LF or the end (of the consumed bytes: of the file)
    nxt = np.where(~cr, idx, m)
    nxt = np.minimum.accumulate(nxt[::-1])[::-1] if m else nxt
    ends = np.concatenate((nl, [True]))
    dropped = cr & ends[nxt]
    hs_before = np.cumsum(hs) - hs
    open_before = in_rec0 | (hs_before > 0)
    sep = hs & open_before
    base = ~in_hdr & ~nl & ~dropped & open_before & ~hs
    emit = sep | base
    codes = np.where(sep, 4, _CODE[t])[emit].astype(np.uint8)
    n_hs = int(hs.sum())
    open_after = in_rec0 or n_hs > 0
    closing = final and open_after
    stream = np.concatenate((head, codes, np.full(1 if closing else 0, 4, np.uint8)))
    # offsets: piece 0 of an open record from 0; a record starts behind the separator its '>' emits
    pos_before = c + np.cumsum(emit) - emit
    starts = (pos_before + sep)[hs]
    offsets = np.concatenate(([0] if in_rec0 else [], starts, [len(stream)])).astype(np.int64)
    out = State(0, state.records + n_hs, state.positions + len(stream) - c)
    if not final:
        mid = bool(t[m - 1] != LF)
        out.flags = (IN_RECORD if open_after else 0) | (MID_LINE if mid else 0) | (IN_HEADER if mid and bool(in_hdr[m - 1]) else 0)
    return stream, offsets, m, out


def pack_file(text: bytes):
    """the whole file in one final chunk -> (codes, offsets)"""
    s, off, m, _ = pack_chunk(text, True, State())
    assert m == len(text)
    return s, off


def pack_cuts(text: bytes, cuts, carry: int = 0):
    """The file in the chunks [0, cuts[0]), [cuts[0], cuts[1]) ... with what a call leaves handed over again in front of
    the next chunk, the last one final.  -> list of (codes, offsets, consumed, state afterwards, the text of the call);
    codes None: the call is refused (a chunk of CR only)."""
    calls, state, prev, left = [], State(), None, b""
    bounds = [0, *cuts, len(text)]
    for i in range(len(bounds) - 1):
        final = i == len(bounds) - 2
        chunk = left + text[bounds[i]:bounds[i + 1]]
        try:
            s, off, m, state = pack_chunk(chunk, final, state, prev, carry)
        except NoProgress:                                   # refused, state unchanged: the caller hands it all over again
            calls.append((None, None, 0, state.copy(), chunk))
            left = chunk
            continue
        calls.append((s, off, m, state.copy(), chunk))
        left = chunk[m:]
        if len(chunk) or final:
            prev = s
    return calls


def join_slices(calls, carry_of=lambda call_index, codes: 0):
    """the calls' streams without their carried heads, concatenated"""
    return np.concatenate([np.zeros(0, np.uint8)] + [c[0][carry_of(i, c[0]):] for i, c in enumerate(calls) if c[0] is not None])


def stream_words(n_bases: int):
    T = (n_bases + 63) // 64
    return 2 * T + 4, T + 2


def to_words(codes):
    """(packed uint64[pw], invalid uint64[mw]) of kdf_stream_words(len(codes)): zero bits and set mask bits past the end"""
    n = len(codes)
    pw, mw = stream_words(n)
    two = np.zeros(pw * 32, np.uint8)
    two[:n] = np.where(codes < 4, codes, 0)
    bits = np.zeros((pw * 32, 2), np.uint8)
    bits[:, 0], bits[:, 1] = two & 1, two >> 1
    packed = np.packbits(bits.reshape(-1), bitorder="little").view("<u8").astype(np.uint64)
    inv = np.ones(mw * 64, np.uint8)
    inv[:n] = codes > 3
    invalid = np.packbits(inv, bitorder="little").view("<u8").astype(np.uint64)
    return packed, invalid


def from_words(packed, invalid, n_bases: int):
    """codes of the first n_bases positions of a stream"""
    two = np.unpackbits(np.ascontiguousarray(packed).view(np.uint8), bitorder="little").reshape(-1, 2)
    inv = np.unpackbits(np.ascontiguousarray(invalid).view(np.uint8), bitorder="little")
    codes = (two[:n_bases, 0] | (two[:n_bases, 1] << 1)).astype(np.uint8)
    assert not (codes[inv[:n_bases] == 1] != 0).any(), "an invalid position with packed bits"
    return np.where(inv[:n_bases] == 1, 4, codes).astype(np.uint8)


def records_of(codes, offsets):
    """the records as strings of ACGTN, separators dropped (a piece without one keeps all its positions)"""
    out = []
    for r in range(len(offsets) - 1):
        piece = codes[offsets[r]:offsets[r + 1]]
        if len(piece) and piece[-1] == 4:
            piece = piece[:-1]
        out.append("".join("ACGTN"[c] for c in piece))
    return out


# ---- the case list ----------------------------------------------------------------------------------------------------

TABLE = [                                                    # (text, the records the header's rule gives)
    (b">a\r\nAC\r\nGT\r\n", ["ACGT"]),
    (b">a\nAC\r\r\nGT", ["ACGT"]),
    (b">a\nA\rC\nG T\n", ["ANCGNT"]),
    (b"ACGT\n>a\nAC\n", ["AC"]),
    (b"ACGT\nAC\n", []),
    (b">a\n>b\nAC\n>c\n", ["", "AC", ""]),
    (b">\nAC\n\n\n>d", ["AC", ""]),
    (b">a\nac\n  \nnN\n", ["ACNNNN"]),
    (b">a\nAC\n>", ["AC", ""]),
    (b" >a\nAC\n>b\nA>C\n", ["ANC"]),
    (b"", []),
    (b"\n\n", []),
]


def random_fasta(seed: int, width, crlf: bool, n_records: int = 6, mean_len: int = 150, lead: bytes = b"", final_newline: bool = True) -> bytes:
    """A seeded multi-FASTA: lines of ``width`` bases (None: unwrapped), LF or CRLF, lower case, N runs and IUPAC codes,
    empty records, ``lead`` before the first header."""
    rng = np.random.default_rng(seed)
    eol = b"\r\n" if crlf else b"\n"
    out = [lead]
    for r in range(n_records):
        out.append(b">r%d some text" % r + eol)
        n = 0 if rng.random() < 0.2 else int(rng.integers(1, 2 * mean_len))
        seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), n)
        if n and rng.random() < 0.5:                         # lower case stretch
            a = int(rng.integers(0, n))
            seq[a:a + int(rng.integers(1, 40))] |= 0x20
        if n and rng.random() < 0.6:                         # N run
            a = int(rng.integers(0, n))
            seq[a:a + int(rng.integers(1, 30))] = ord("N")
        for _ in range(int(rng.integers(0, 3))):             # IUPAC codes
            if n:
                seq[int(rng.integers(0, n))] = rng.choice(np.frombuffer(b"RYKMSWBDHVn", np.uint8))
        seq = seq.tobytes()
        w = width or max(n, 1)
        for a in range(0, n, w):
            out.append(seq[a:a + w] + eol)
    text = b"".join(out)
    if not final_newline and text.endswith(eol):
        text = text[:-len(eol)]
    return text


def cases():
    """[(name, text)]: the header's table, the golden mini reference, seeded random texts"""
    out = [("table%d" % i, t) for i, (t, _) in enumerate(TABLE)]
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "giab", "mini_ref.fa")
    with open(golden, "rb") as f:
        out.append(("mini_ref", f.read()))
    seed = 0
    for width in (1, 60, 61, None):
        for crlf in (False, True):
            seed += 1
            out.append((f"random_w{width}_{'crlf' if crlf else 'lf'}", random_fasta(seed, width, crlf, lead=b"ACGT\nstray\n" if seed % 2 else b"",
                                                                                    final_newline=seed % 3 != 0)))
    out.append(("random_small", random_fasta(99, 7, True, n_records=3, mean_len=20, final_newline=False)))
    out.append(("random_long", random_fasta(100, 60, False, n_records=24, mean_len=6000)))
    return out
