"""The case list of the device FASTA feeder, pinned on the CPU: on every case the numpy model of the header's rule
(tests/fasta_stream_model.py) == the host reader (``fasta_reader``, one batch) unpacked == ``oracle.read_fasta``, and the
model's chunked form equals its whole form -- slices, state, ``consumed``, offsets and carry.  No GPU; it passes without
the feature, and that is its job: the GPU tests compare the kernels with this model.

``oracle.read_fasta`` opens its file in text mode, where a lone CR ends a line, so it is compared on the cases in which
every CR stands in front of a line end (the rule and the host reader make an interior CR an invalid position: the table
case ``A\\rC``); the other two are compared on all.  Cut points: every one for the cases up to 256 bytes; for the longer
ones the first 64 bytes, two bytes either side of 40 line ends, and 60 seeded random ones, plus seeded sets of 3 to 9 chunks.
"""
import re

import numpy as np
import pytest

import fasta_stream_model as M

CASES = M.cases()
IDS = [name for name, _ in CASES]


def _write(tmp_path, text):
    p = str(tmp_path / "case.fa")
    with open(p, "wb") as f:
        f.write(text)
    return p


def _cuts_of(text):
    n = len(text)
    if n <= 256:
        return list(range(n + 1))
    rng = np.random.default_rng(n)
    ends = [m.start() for m in re.finditer(rb"[\r\n>]", text)]
    picked = [ends[i] for i in np.linspace(0, len(ends) - 1, 40).astype(int)] if ends else []
    cuts = set(range(65)) | {e + d for e in picked for d in (-2, -1, 0, 1, 2)} | set(rng.integers(0, n + 1, 60).tolist())
    return sorted(c for c in cuts if 0 <= c <= n)


def test_table_records():
    for text, want in M.TABLE:
        codes, off = M.pack_file(text)
        assert M.records_of(codes, off) == want, text
        assert (codes[off[1:] - 1] == 4).all()                           # every record ends in its separator
        assert len(off) - 1 == len(want)


@pytest.mark.parametrize("name,text", CASES, ids=IDS)
def test_model_is_the_host_reader(tmp_path, name, text):
    from kmer_denovo_filter_amd.reads import fasta_reader
    codes, off = M.pack_file(text)
    batches = list(fasta_reader(_write(tmp_path, text), 31, max_bases=1 << 22, max_reads=1 << 16))
    if len(off) == 1:
        assert batches == []
        return
    assert len(batches) == 1
    b = batches[0]
    assert b.n_bases == len(codes)
    assert (np.asarray(b.offsets) == off).all()
    assert (M.from_words(b.packed, b.invalid, b.n_bases) == codes).all()
    packed, invalid = M.to_words(codes)
    assert (b.packed == packed).all() and (b.invalid == invalid).all()   # the words behind n_bases too


ORACLE_CASES = [(n, t) for n, t in CASES if not re.search(rb"\r(?![\r\n])", re.sub(rb"\r+\Z", b"", t))]   # no CR inside a line


@pytest.mark.parametrize("name,text", ORACLE_CASES, ids=[n for n, _ in ORACLE_CASES])
def test_model_is_the_oracle(tmp_path, oracle, name, text):
    codes, off = M.pack_file(text)
    want = ["".join(c.upper() if c in "ACGTacgt" else "N" for c in seq) for _, seq in oracle.read_fasta(_write(tmp_path, text))]
    assert M.records_of(codes, off) == want


def _check_calls(text, cuts, carry):
    whole, whole_off = M.pack_file(text)
    calls = M.pack_cuts(text, cuts, carry)
    heads = []
    prev = None
    for i, (s, off, m, st, chunk) in enumerate(calls):
        if s is None:
            assert len(chunk) and set(chunk) == {13}
            heads.append(0)
            continue
        final = i == len(calls) - 1
        before = calls[i - 1][3] if i else M.State()
        if not len(chunk) and not final:                                 # emits nothing, changes nothing
            assert len(s) == 0 and list(off) == [0] and m == 0 and st == before
            heads.append(0)
            continue
        assert m == (len(chunk) if final else len(chunk.rstrip(b"\r")))
        c = 0
        # the head is the tail of the previous stream, iff a record was open
        if carry and prev is not None and len(prev) and before.flags & M.IN_RECORD:
            c = min(carry, len(prev))
            assert (s[:c] == prev[len(prev) - c:]).all()
        heads.append(c)
        assert off[0] == 0 and off[-1] == len(s) and (np.diff(off) >= 0).all()
        assert len(off) - 1 == (1 if before.flags & M.IN_RECORD else 0) + st.records - before.records
        assert st.positions - before.positions == len(s) - c
        if len(chunk) or final:
            prev = s
    got = M.join_slices(calls, lambda i, s: heads[i])
    assert len(got) == len(whole) and (got == whole).all()
    last = calls[-1][3]
    assert last.flags == 0 and last.records == len(whole_off) - 1 and last.positions == len(whole)
    return calls


@pytest.mark.parametrize("name,text", CASES, ids=IDS)
def test_two_chunks_equal_the_whole(name, text):
    for cut in _cuts_of(text):
        for carry in (0, 4):
            _check_calls(text, [cut], carry)


@pytest.mark.parametrize("name,text", CASES, ids=IDS)
def test_many_chunks_equal_the_whole(name, text):
    rng = np.random.default_rng(len(text) + 7)
    for rep in range(8):
        cuts = sorted(rng.integers(0, len(text) + 1, int(rng.integers(2, 9))).tolist())
        _check_calls(text, cuts, (0, 30)[rep & 1])


def test_states_at_the_named_cuts():
    """between CR and LF, inside CR CR LF, either side of a '>', inside a header"""
    text = b">ab\r\nAC\r\r\nG\n>c\nT\n"
    def state_after(cut):
        return M.pack_cuts(text, [cut])[0]
    s, off, m, st, _ = state_after(4)                                    # ">ab\r" | "\nAC..": the CR is left to the next call
    assert m == 3 and st.flags == M.IN_RECORD | M.MID_LINE | M.IN_HEADER and len(s) == 0
    s, off, m, st, _ = state_after(8)                                    # ">ab\r\nAC\r" | "\r\nG"
    assert m == 7 and st.flags == M.IN_RECORD | M.MID_LINE and len(s) == 2
    s, off, m, st, _ = state_after(12)                                   # in front of the second '>'
    assert m == 12 and st.flags == M.IN_RECORD and len(s) == 3 and st.records == 1
    s, off, m, st, _ = state_after(13)                                   # behind it: its separator is out, the record counted
    assert m == 13 and st.flags == M.IN_RECORD | M.MID_LINE | M.IN_HEADER and len(s) == 4 and st.records == 2
    assert list(off) == [0, 4, 4]
    with pytest.raises(M.NoProgress):
        M.pack_chunk(b"\r\r", False, M.State())
    s, off, m, st = M.pack_chunk(b"", True, M.State(M.IN_RECORD, 1, 5))   # an empty last call closes the record
    assert list(s) == [4] and list(off) == [0, 1] and st.flags == 0
    s, off, m, st = M.pack_chunk(b"", False, M.State(M.IN_RECORD, 1, 5))
    assert len(s) == 0 and st == M.State(M.IN_RECORD, 1, 5)
