"""The case list of the device FASTQ feeder, pinned on the CPU: on every well-formed case the model of the header's rule
(tests/fastq_stream_model.py) == ``ReadStream.from_strings`` of the case's sequences -- the existing host packer, which
shares nothing with the feeder -- word for word and offset for offset; with ``min_qual`` set, == ``from_strings`` of the
sequences with the low-quality bases replaced by N; every bad case raises its (offset, rule); and the model's chunked form
concatenates to its whole form at every cut.  No GPU; it passes without the kernels, and that is its job: the GPU tests
compare the kernels with this model.  Cut points: every one for the cases up to 256 bytes; for the longer ones the first
64 bytes, two bytes either side of 40 line ends and of the tile edges, and 60 seeded random ones, plus seeded sets of 3
to 9 chunks."""
import numpy as np
import pytest

import fastq_stream_model as M

CASES = M.cases()
GOOD = [c for c in CASES if c.bad is None]
BAD = [c for c in CASES if c.bad is not None]


def quals_of(case):
    """min_qual values for a case: off, '!' (nothing is below it), a value that splits the case's qualities, 255"""
    q = np.frombuffer(b"".join(q for _, q in case.reads), np.uint8)
    mid = int(np.sort(q)[len(q) // 2]) if len(q) else 50
    return (0, 33, mid, 255)


def test_the_list_holds_the_shapes_the_issue_names():
    names = {c.name for c in CASES}
    assert len(names) == len(CASES)
    lengths = {len(s) for c in GOOD for s, _ in c.reads}
    assert {0, 1, 31, 32, 33, 63, 64, 65, 10000} <= lengths
    assert {len(c.reads) for c in GOOD} >= {0, 1}
    assert {c.bad[1] for c in BAD} == {M.BAD_HEADER, M.BAD_PLUS, M.LENGTH, M.TRUNCATED}
    assert 140000 < max(len(c.text) for c in CASES) < 160000
    by = {c.name: c for c in CASES}
    assert not by["no_final_newline"].text.endswith(b"\n") and b"\r\r\n" in by["cr_cr_lf"].text
    assert by["five_trailing_blank_lines"].text.endswith(b"\n\n\r\n\n\n\r\n") and by["one_trailing_blank_line"].text.endswith(b"\n\n")
    assert by["header_longer_than_a_tile"].text.index(b"\n") > M.TILE
    assert by["line_end_on_last_byte_of_a_tile"].text[M.TILE - 1] == M.LF and by["line_end_on_first_byte_of_a_tile"].text[M.TILE] == M.LF
    t = by["sequence_and_quality_in_different_tiles"].text
    lines = t.split(b"\n")
    assert len(lines[0]) + 1 + len(lines[1]) < M.TILE < len(lines[0]) + len(lines[1]) + len(lines[2]) + 3
    assert len(by["one_read_of_10k"].text) > 3 * M.TILE + 2 * 10000 - 4 * M.TILE and len(by["one_read_of_10k"].reads[0][0]) > 2 * M.TILE
    assert by["at_and_plus_quality"].text.count(b"\n@") > 4 and b"\n+III" in by["at_and_plus_quality"].text


@pytest.mark.parametrize("case", GOOD, ids=[c.name for c in GOOD])
def test_model_is_the_host_packer(case):
    from kmer_denovo_filter_amd.reads import ReadStream
    for mq in quals_of(case):
        codes, off = M.pack_file(case.text, mq)
        want = ReadStream.from_strings([M.masked(s, q, mq) for s, q in case.reads])
        assert want.n_bases == len(codes) == sum(len(s) + 1 for s, _ in case.reads)
        packed, invalid = M.to_words(codes)
        assert (want.packed == packed).all() and (want.invalid == invalid).all()      # the words behind n_bases too
        assert (np.asarray(want.offsets) == off).all()
        if mq == 255 and len(codes):
            assert (codes == 4).all()
        if mq in (0, 33):                                                                # '!' is the lowest quality a case holds
            assert (codes == M.pack_file(case.text, 0)[0]).all()


def test_a_mid_quality_masks_some_bases_and_not_all():
    case = next(c for c in GOOD if c.name == "random_150k")
    mid = quals_of(case)[2]
    plain, low = M.pack_file(case.text)[0], M.pack_file(case.text, mid)[0]
    assert 0.3 < ((low == 4) & (plain != 4)).sum() / (plain != 4).sum() < 0.7


@pytest.mark.parametrize("case", BAD, ids=[c.name for c in BAD])
def test_bad_cases_raise_their_rule(case):
    for mq in (0, 50):
        with pytest.raises(M.FormatError) as ei:
            M.pack_file(case.text, mq)
        assert (ei.value.offset, ei.value.rule) == case.bad


def _cuts_of(text):
    n = len(text)
    if n <= 256:
        return list(range(n + 1))
    rng = np.random.default_rng(n)
    ends = np.flatnonzero(np.frombuffer(text, np.uint8) == M.LF).tolist()
    picked = [ends[i] for i in np.linspace(0, len(ends) - 1, 40).astype(int)] + list(range(M.TILE, n, M.TILE))
    cuts = set(range(65)) | {e + d for e in picked for d in (-2, -1, 0, 1, 2)} | set(rng.integers(0, n + 1, 60).tolist())
    return sorted(c for c in cuts if 0 <= c <= n)


def _check_calls(text, cuts, mq):
    whole, whole_off = M.pack_file(text, mq)
    calls = M.pack_cuts(text, cuts, mq)
    assert sum(c[2] for c in calls) == len(text)
    pos = 0
    for i, (codes, off, m, st, chunk) in enumerate(calls):
        final = i == len(calls) - 1
        assert off[0] == 0 and off[-1] == len(codes) and (np.diff(off) >= 1).all()
        if final:
            assert m == len(chunk)
        else:                                                            # whole records only: the consumed text ends in the fourth '\n' of its last record
            assert m <= len(chunk) and chunk[:m].count(b"\n") == 4 * (len(off) - 1)
            assert m == 0 or chunk[m - 1] == M.LF
            rest = chunk[m:]
            body = rest.rstrip(b"\r\n")                                    # (of the line ends behind it the call sees the first)
            assert body.count(b"\n") + (b"\n" in rest[len(body):]) < 4
        assert (codes == whole[pos:pos + len(codes)]).all()
        pos += len(codes)
    got_off = np.concatenate([[0]] + [c[1][1:] + (calls[i - 1][3].positions if i else 0) for i, c in enumerate(calls)])
    assert pos == len(whole) and (got_off == whole_off).all()
    assert calls[-1][3] == M.State(len(whole_off) - 1, len(whole), len(text))


@pytest.mark.parametrize("case", GOOD, ids=[c.name for c in GOOD])
def test_two_chunks_equal_the_whole(case):
    for cut in _cuts_of(case.text):
        _check_calls(case.text, [cut], 0)
    for cut in _cuts_of(case.text)[::7]:
        _check_calls(case.text, [cut], quals_of(case)[2])


@pytest.mark.parametrize("case", GOOD, ids=[c.name for c in GOOD])
def test_many_chunks_equal_the_whole(case):
    rng = np.random.default_rng(len(case.text) + 7)
    for rep in range(8):
        cuts = sorted(rng.integers(0, len(case.text) + 1, int(rng.integers(2, 9))).tolist())
        _check_calls(case.text, cuts, (0, quals_of(case)[2])[rep & 1])


def test_a_chunk_without_a_complete_record_is_left_whole():
    text = next(c for c in GOOD if c.name == "no_final_newline").text
    end = text.index(b"\n@r1") + 1
    for cut in range(end):
        codes, off, m = M.pack_chunk(text[:cut], False)
        assert len(codes) == 0 and list(off) == [0] and m == 0
    codes, off, m = M.pack_chunk(text[:end], False)
    assert m == end and len(off) == 2
    # an incomplete record is not examined by a call that is not the last; the last call reports it
    codes, off, m = M.pack_chunk(text[:end] + b"oops\nAC", False)
    assert m == end and len(off) == 2
    with pytest.raises(M.FormatError) as ei:
        M.pack_chunk(b"oops\nAC", True)
    assert (ei.value.offset, ei.value.rule) == (0, M.BAD_HEADER)
