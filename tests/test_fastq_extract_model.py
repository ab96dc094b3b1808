"""The model of kdf_fq_extract (tests/fastq_extract_model.py) delimits records by its own reading of THE RULE; here it is
held to the feeder's model on the feeder's case list: the same number of records, the same ``consumed``, the same
(offset, rule) of a format error -- for the whole text as a final call, as a call that is not the last, and cut in two.
The kept form of a record is checked against the reads the case was built from.  No GPU."""
import numpy as np
import pytest

import fastq_extract_model as X
import fastq_stream_model as M

CASES = M.cases()


def _both(text, final):
    try:
        codes, offs, consumed = M.pack_chunk(text, final)
        want = (len(offs) - 1, consumed)
    except M.FormatError as ex:
        want = ("bad", ex.offset, ex.rule)
    try:
        recs, consumed = X.records_of(text, final)
        got = (len(recs), consumed)
    except X.FormatError as ex:
        got = ("bad", ex.offset, ex.rule)
    return want, got


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
@pytest.mark.parametrize("final", (True, False))
def test_records_consumed_and_errors_agree(case, final):
    want, got = _both(case.text, final)
    assert want == got


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cut_in_two_agrees(case):
    rng = np.random.default_rng(len(case.text))
    for cut in sorted(set(rng.integers(0, len(case.text) + 1, 8).tolist())):
        head = case.text[:cut]
        want, got = _both(head, False)
        assert want == got, cut
        if want[0] == "bad":
            continue
        want, got = _both(case.text[want[1]:], True)
        assert want == got, cut


@pytest.mark.parametrize("case", [c for c in CASES if c.bad is None], ids=[c.name for c in CASES if c.bad is None])
def test_kept_form_of_every_record(case):
    recs, consumed = X.records_of(case.text, True)
    assert consumed == len(case.text) and len(recs) == len(case.reads)
    for body, (s, q) in zip(recs, case.reads):
        lines = body.split(b"\n")
        assert body.endswith(b"\n") and len(lines) == 5 and lines[4] == b""            # four lines, each closed by a LF
        assert lines[0][:1] == b"@" and lines[2][:1] == b"+"
        assert lines[1].rstrip(b"\r") == s and lines[3].rstrip(b"\r") == q
    whole = b"".join(recs)
    assert len(whole) <= consumed + 2
    # all of the text but its trailing blank lines, and at most two supplied line ends
    stem = case.text.rstrip(b"\r\n")
    assert whole[:len(stem)] == stem and whole[len(stem):].strip(b"\r\n") == b""
    # keeping everything is the concatenation, keeping nothing is empty, and the offsets are the running lengths
    out, offs, m = X.extract_chunk(case.text, True, [1] * len(recs))
    assert (out, m) == (whole, len(case.text)) and offs == list(np.cumsum([0] + [len(b) for b in recs]))
    assert X.extract_chunk(case.text, True, [0] * len(recs)) == (b"", [0], len(case.text))


def test_refusals():
    text = M.fq(M.reads_of((5, 0, 9), 2))
    with pytest.raises(X.Invalid):
        X.extract_chunk(text, True, [1, 1])
    with pytest.raises(X.Invalid):
        X.extract_chunk(text, True, [1, 1, 1, 1])
    out, _, _ = X.extract_chunk(text, True, [1, 0, 1])
    X.extract_chunk(text, True, [1, 0, 1], cap_out=len(out))
    with pytest.raises(X.Invalid):
        X.extract_chunk(text, True, [1, 0, 1], cap_out=len(out) - 1)
    with pytest.raises(X.Invalid):
        X.extract_chunk(b"", True, [1])
    bad = [c for c in CASES if c.name == "length"][0]
    with pytest.raises(X.FormatError):                      # the format comes before the count
        X.extract_chunk(bad.text, True, [])


def test_cuts_concatenate_to_the_whole():
    reads = M.reads_of(np.random.default_rng(3).integers(0, 120, 60).tolist(), 3)
    text = M.fq(reads, eol=b"\r\n", final_newline=False)
    keep = (np.random.default_rng(4).random(len(reads)) < 0.4).tolist()
    whole, _, _ = X.extract_chunk(text, True, keep)
    cuts = sorted(set(np.random.default_rng(5).integers(1, len(text), 12).tolist()))
    calls = X.extract_cuts(text, cuts, keep)
    assert b"".join(c[3] for c in calls) == whole and sum(c[2] for c in calls) == len(reads)
