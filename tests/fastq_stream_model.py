"""A plain numpy/Python MODEL of the device FASTQ feeder (include/kdf.h "device FASTQ feeder"), written from the header's
text alone: no engine, no library.  ``pack_chunk`` is kdf_fastq_pack for one call; ``cases()`` is the case list the CPU
and the GPU tests share.

A stream is held as a uint8 array of CODES, one per position: 0 .. 3 = A C G T, 4 = invalid (N, IUPAC, a blank, an
interior CR, a base of low quality, a separator).  ``to_words`` (of the FASTA model: the same "Read streams" layout) turns
codes into the packed and mask words.
"""
from collections import namedtuple

import numpy as np

from fasta_stream_model import from_words, stream_words, to_words  # noqa: F401  (the stream layout is the same)

BAD_HEADER, BAD_PLUS, LENGTH, TRUNCATED = 1, 2, 3, 4
TILE = 4096                                                  # KDF_FASTQ_TILE_BYTES (test_abi_fastq_feeder.py holds it to the header)
LF, CR = 10, 13

_CODE = np.full(256, 4, np.uint8)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _i


class FormatError(ValueError):
    """KDF_ERR_IO: ``offset`` of the first byte of the first bad record within the call's text, ``rule`` it breaks"""

    def __init__(self, offset, rule):
        super().__init__(f"record at {offset} breaks rule {rule}")
        self.offset, self.rule = offset, rule


class State:
    """kdf_fastq_state"""

    def __init__(self, records=0, positions=0, bytes=0):  # noqa: A002
        self.records, self.positions, self.bytes = records, positions, bytes

    def copy(self):
        return State(self.records, self.positions, self.bytes)

    def key(self):
        return (self.records, self.positions, self.bytes)

    def __eq__(self, o):
        return self.key() == o.key()

    def __repr__(self):
        return "State(records=%d, positions=%d, bytes=%d)" % self.key()


def _strip(t, s, e):
    """the line [s, e) without the CR directly in front of its end"""
    while e > s and t[e - 1] == CR:
        e -= 1
    return e


def pack_chunk(text: bytes, final: bool, min_qual: int = 0):
    """One call -> (codes of the call's stream, offsets int64[n_reads + 1], consumed); FormatError for a text that breaks
    a rule.  A call that is not the last and holds no complete record gives (no codes, [0], 0): it writes nothing."""
    t = bytes(text)
    n = len(t)
    while n and t[n - 1] in (LF, CR):                        # the trailing bytes that are only LF / CR ...
        n -= 1
    if not final:                                            # ... of which a call that is not the last sees the first line end
        while n < len(t) and t[n] == CR:
            n += 1
        n = min(n + 1, len(t))
    ends = np.flatnonzero(np.frombuffer(t[:n], np.uint8) == LF).tolist()
    if final and n:
        ends.append(n)                                       # the text's end closes the last line
    lines, start = [], 0
    for e in ends:
        lines.append((start, e))
        start = e + 1
    n_rec = -(-len(lines) // 4) if final else len(lines) // 4
    lines = lines[:4 * n_rec]
    consumed = len(t) if final else (lines[-1][1] + 1 if n_rec else 0)
    codes, offsets, bad = [], [0], None
    for r in range(n_rec):
        rec = lines[4 * r:4 * r + 4]
        have = len(rec)
        s0, e0 = rec[0]
        rule = 0 if (s0 < e0 and t[s0] == ord("@")) else BAD_HEADER
        seq = qual = b""
        if have >= 2:
            seq = t[rec[1][0]:_strip(t, *rec[1])]
        if have >= 3 and not rule and not (rec[2][0] < rec[2][1] and t[rec[2][0]] == ord("+")):
            rule = BAD_PLUS
        if have == 4:
            qual = t[rec[3][0]:_strip(t, *rec[3])]
            if not rule and len(qual) != len(seq):
                rule = LENGTH
        elif not rule and not (have == 3 and len(seq) == 0):  # three lines and no bases: an empty quality line
            rule = TRUNCATED
        if rule:
            if bad is None:
                bad = (s0, rule)
            continue
        c = _CODE[np.frombuffer(seq, np.uint8)]
        if min_qual > 0 and len(seq):
            c = np.where(np.frombuffer(qual, np.uint8) < min_qual, 4, c).astype(np.uint8)
        codes += [c, np.full(1, 4, np.uint8)]
        offsets.append(offsets[-1] + len(seq) + 1)
    if bad is not None:
        raise FormatError(*bad)
    return np.concatenate([np.zeros(0, np.uint8)] + codes), np.asarray(offsets, np.int64), consumed


def pack_file(text: bytes, min_qual: int = 0):
    """the whole file in one final call -> (codes, offsets)"""
    codes, off, m = pack_chunk(text, True, min_qual)
    assert m == len(text)
    return codes, off


def pack_cuts(text: bytes, cuts, min_qual: int = 0):
    """The file in the chunks [0, cuts[0]), [cuts[0], cuts[1]) ... with what a call leaves handed over again in front of the
    next chunk, the last one final -> list of (codes, offsets, consumed, state afterwards, the text of the call)."""
    calls, state, left = [], State(), b""
    bounds = [0, *cuts, len(text)]
    for i in range(len(bounds) - 1):
        chunk = left + text[bounds[i]:bounds[i + 1]]
        codes, off, m = pack_chunk(chunk, i == len(bounds) - 2, min_qual)
        state = State(state.records + len(off) - 1, state.positions + len(codes), state.bytes + m)
        calls.append((codes, off, m, state.copy(), chunk))
        left = chunk[m:]
    return calls


def masked(seq: bytes, qual: bytes, min_qual: int) -> bytes:
    """the read with the bases of a quality below min_qual turned to N"""
    return bytes(ord("N") if (min_qual > 0 and q < min_qual) else b for b, q in zip(seq, qual))


# ---- the case list ----------------------------------------------------------------------------------------------------

Case = namedtuple("Case", "name text reads bad")             # reads: [(sequence, quality)] of a well-formed text; bad: (offset, rule)


def seq(n, seed, ns=True):
    """n seeded bases with a lower-case stretch and, with ``ns``, a run of N"""
    rng = np.random.default_rng(seed)
    s = rng.choice(np.frombuffer(b"ACGT", np.uint8), n)
    if n > 8:
        a = int(rng.integers(0, n - 4))
        s[a:a + int(rng.integers(1, 12))] |= 0x20
        if ns:
            a = int(rng.integers(0, n - 4))
            s[a:a + int(rng.integers(1, 6))] = ord("N")
    return s.tobytes()


def qual(n, seed):
    """n seeded quality bytes '!' .. 'I'"""
    return np.random.default_rng(seed + 7919).integers(33, 74, n).astype(np.uint8).tobytes()


def reads_of(lengths, seed=0):
    return [(seq(n, seed + 31 * i), qual(n, seed + 31 * i)) for i, n in enumerate(lengths)]


def fq(reads, eol=b"\n", header=lambda i: b"@r%d" % i, plus=lambda i: b"+", final_newline=True, tail=b""):
    text = b"".join(header(i) + eol + s + eol + plus(i) + eol + q + eol for i, (s, q) in enumerate(reads))
    if not final_newline and text:
        text = text[:-len(eol)]
    return text + tail


def cases():
    """[Case]: every shape the header's rule names, at the smallest size that can break a kernel"""
    out = []

    def good(name, text, reads):
        out.append(Case(name, text, [(bytes(s), bytes(q)) for s, q in reads], None))

    def bad(name, text, offset, rule):
        out.append(Case(name, text, None, (offset, rule)))

    word = reads_of((0, 1, 31, 32, 33, 63, 64, 65), 1)
    good("word_lengths", fq(word), word)
    for n in (0, 1, 31, 32, 33, 63, 64, 65):
        one = reads_of((n,), 100 + n)
        good("one_record_%d" % n, fq(one), one)
    good("no_records", b"", [])
    good("only_line_ends", b"\n\r\n\n", [])
    three = reads_of((5, 0, 9), 2)
    good("no_final_newline", fq(three, final_newline=False), three)
    good("crlf", fq(three, eol=b"\r\n"), three)
    good("cr_cr_lf", fq(three, eol=b"\r\r\n"), three)
    good("crlf_no_final_newline", fq(three, eol=b"\r\n", final_newline=False), three)
    good("interior_cr", b"@a\nAC\rGT\n+\nII\rII\n@b\n\rA\n+\n!I\n", [(b"AC\rGT", b"II\rII"), (b"\rA", b"!I")])
    iupac = b"acgtnRYKMSWBDHV Aa"
    good("lower_and_iupac", fq([(iupac, b"I" * len(iupac))]), [(iupac, b"I" * len(iupac))])
    good("at_and_plus_quality", b"@a\nACGT\n+\n@III\n@b\nACGT\n+\n+III\n@c\nAC\n+\n@+\n@d\nA\n+\n@\n", [(b"ACGT", b"@III"), (b"ACGT", b"+III"), (b"AC", b"@+"), (b"A", b"@")])
    good("plus_name", fq(three, plus=lambda i: b"+r%d some text" % i), three)
    good("at_in_header_and_sequence_of_signs", b"@a @b +c\nAC\n+@\nII\n", [(b"AC", b"II")])
    long_hdr = reads_of((40, 20), 3)
    good("header_longer_than_a_tile", fq(long_hdr, header=lambda i: b"@" + b"h@+" * (TILE // 2) + b"%d" % i), long_hdr)
    # a line end on the last byte and on the first byte of a tile: the header's '\n' at TILE - 1, then (50 bases later) the
    # sequence's; the second text has both one byte later
    edge = reads_of((TILE - 2, 33), 4)
    for shift, name in ((0, "line_end_on_last_byte_of_a_tile"), (1, "line_end_on_first_byte_of_a_tile")):
        text = fq(edge, header=lambda i, s=shift: b"@" + b"x" * (TILE - 2 + s if i == 0 else 3))
        assert text[TILE - 1 + shift] == LF
        good(name, text, edge)
    edge2 = reads_of((TILE, 12), 5)                             # the header ends on the last byte of tile 0, the sequence on the first of tile 2
    text = fq(edge2, header=lambda i: b"@" + b"y" * (TILE - 2 if i == 0 else 1))
    assert text[TILE - 1] == LF and text[2 * TILE] == LF
    good("line_ends_on_both_tile_edges", text, edge2)
    split = reads_of((3000, 70), 6)
    text = fq(split, plus=lambda i: b"+" + b"p" * (1100 if i == 0 else 0))
    assert text.index(b"\n+p") < TILE < text.index(b"p\n") + 2           # the sequence line lies in tile 0, its quality line behind it
    good("sequence_and_quality_in_different_tiles", text, split)
    tenk = reads_of((10000,), 7)
    good("one_read_of_10k", fq(tenk), tenk)
    good("one_trailing_blank_line", fq(three, tail=b"\n"), three)
    good("five_trailing_blank_lines", fq(three, tail=b"\n\r\n\n\n\r\n"), three)
    last_empty = reads_of((7, 0), 8)
    good("last_record_empty", fq(last_empty), last_empty)
    good("last_record_empty_no_final_newline", fq(last_empty)[:-1], last_empty)        # "...@r1\n\n+\n": the final '\n' of the empty quality line is gone
    good("last_record_empty_three_lines", fq(last_empty)[:-2], last_empty)             # "...@r1\n\n+"
    good("only_an_empty_record", b"@\n\n+", [(b"", b"")])
    rnd = reads_of(np.random.default_rng(9).integers(100, 201, 460).tolist(), 9)
    good("random_150k", fq(rnd), rnd)
    rnd_crlf = reads_of(np.random.default_rng(10).integers(0, 90, 300).tolist(), 10)
    good("random_short_crlf", fq(rnd_crlf, eol=b"\r\n", final_newline=False), rnd_crlf)
    # one bad case per rule, each behind a good record
    first = fq(reads_of((6,), 11))
    bad("bad_header", first + b"r1\nAC\n+\nII\n", len(first), BAD_HEADER)
    bad("blank_line_between_records", first + b"\n@r1\nAC\n+\nII\n", len(first), BAD_HEADER)
    bad("bad_plus", first + b"@r1\nAC\n-\nII\n", len(first), BAD_PLUS)
    bad("wrapped_sequence", first + b"@r1\nAC\nGT\n+\nIIII\n", len(first), BAD_PLUS)
    bad("length", first + b"@r1\nACG\n+\nII\n" + first, len(first), LENGTH)
    bad("one_stray_line", first + b"@r1\nAC\n+\nII\r\r\n@X\n", len(first) + 14, TRUNCATED)      # (CR CR LF is a line end: r1 is whole; the stray line is a cut-off record)
    bad("truncated_two_lines", first + b"@r1\nAC\n", len(first), TRUNCATED)
    bad("truncated_three_lines", first + b"@r1\nAC\n+\n", len(first), TRUNCATED)
    bad("truncated_and_bad_header", first + b"r1\nAC\n", len(first), BAD_HEADER)
    bad("two_bad_records", first + b"@r1\nAC\n+\nI\n" + first + b"x\nAC\n+\nII\n", len(first), LENGTH)
    many = fq(reads_of([150] * 40, 12))
    bad("two_bad_records_far_apart", many + b"@q\nAC\n*\nII\n" + many + b"@q\nAC\n+\nIII\n" + many, len(many), BAD_PLUS)
    assert max(len(c.text) for c in out) < 160000
    return out
