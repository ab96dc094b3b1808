"""Shared inputs of the device BAM feeder's tests: DEFLATE payloads made by zlib, a short fixed list of corrupt ones,
a BGZF writer with chosen block cuts, the stand-alone decoder program, and a Python restatement of the record walk
(written from the contract in include/kdf.h, "device BAM feeder")."""
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np

from conftest import ROOT

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
    return out


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
