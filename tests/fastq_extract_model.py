"""A plain-Python MODEL of kdf_fq_extract (include/kdf.h "FASTQ record extract"), written from the header's text alone:
no engine, no library, and its own reading of THE RULE for where records begin and end (tests/test_fastq_extract_model.py
holds it to ``fastq_stream_model.pack_chunk`` on the shared case list).

``records_of`` delimits one call's text; ``extract_chunk`` is kdf_fq_extract for one call; ``extract_cuts`` carries a
file through several calls as the file layer does.
"""
BAD_HEADER, BAD_PLUS, LENGTH, TRUNCATED = 1, 2, 3, 4
LF, CR = 10, 13


class FormatError(ValueError):
    """KDF_ERR_IO: ``offset`` of the first byte of the first bad record within the call's text, ``rule`` it breaks"""

    def __init__(self, offset, rule):
        super().__init__(f"record at {offset} breaks rule {rule}")
        self.offset, self.rule = offset, rule


class Invalid(ValueError):
    """KDF_ERR_INVALID: a wrong n_reads, an output that is too small"""


def _content(t, s, e):
    """the length of the line [s, e) without the CR directly in front of its end"""
    while e > s and t[e - 1] == CR:
        e -= 1
    return e - s


def records_of(text: bytes, final: bool):
    """One call -> ([the kept form of every record, as bytes], consumed); FormatError for the lowest bad record's lowest
    rule.  A record's kept form: its bytes through the LF of line 3; on the final call the last one is completed."""
    t = bytes(text)
    n = len(t)
    end = n
    while end and t[end - 1] in (LF, CR):                    # the final call's text ends in front of its trailing LF / CR
        end -= 1
    if final:
        seen = end
    else:                                                    # a call that is not the last sees the first line end of them
        seen = end
        while seen < n and t[seen] == CR:
            seen += 1
        seen = min(seen + 1, n)
    # lines: (start, the offset of the LF that ends it or, on the final call's last line, `end`)
    lines, start = [], 0
    for i in range(seen):
        if t[i] == LF:
            lines.append((start, i))
            start = i + 1
    if final and end:
        lines.append((start, end))                           # the text's end closes the last line
    n_rec = (len(lines) + 3) // 4 if final else len(lines) // 4
    out, bad = [], None
    for r in range(n_rec):
        rec = lines[4 * r:4 * r + 4]
        s0 = rec[0][0]
        rule = 0
        if not (rec[0][1] > s0 and t[s0] == ord("@")):
            rule = BAD_HEADER
        seq_len = _content(t, *rec[1]) if len(rec) >= 2 else 0
        if not rule and len(rec) >= 3 and not (rec[2][1] > rec[2][0] and t[rec[2][0]] == ord("+")):
            rule = BAD_PLUS
        if not rule and len(rec) == 4 and _content(t, *rec[3]) != seq_len:
            rule = LENGTH
        if not rule and len(rec) < 4 and not (len(rec) == 3 and seq_len == 0):
            rule = TRUNCATED
        if rule:
            if bad is None:
                bad = (s0, rule)
            continue
        if final and r == n_rec - 1:
            # behind `end` lie only CR and LF: through the first LF verbatim, or, without one, the CRs go and a LF is written
            p = end
            while p < n and t[p] == CR:
                p += 1
            body = t[s0:p + 1] if p < n else t[s0:end] + b"\n"
            if len(rec) == 3:
                body += b"\n"                                # the quality line that the rule supplies
        else:
            body = t[s0:rec[3][1] + 1]
        out.append(body)
    if bad is not None:
        raise FormatError(*bad)
    consumed = n if final else (lines[4 * n_rec - 1][1] + 1 if n_rec else 0)
    return out, consumed


def extract_chunk(text: bytes, final: bool, keep, cap_out=None):
    """kdf_fq_extract for one call -> (out bytes, offsets [n_kept + 1], consumed).  ``keep``: one flag per record;
    Invalid when it has another length than the call has records or when the output needs more than ``cap_out`` bytes
    (both behind the format check)."""
    if len(text) == 0:
        if len(keep):
            raise Invalid("0 records, %d flags" % len(keep))
        return b"", [0], 0
    recs, consumed = records_of(text, final)
    if len(recs) != len(keep):
        raise Invalid("%d records, %d flags" % (len(recs), len(keep)))
    parts = [b for b, k in zip(recs, keep) if k]
    offsets = [0]
    for b in parts:
        offsets.append(offsets[-1] + len(b))
    if cap_out is not None and offsets[-1] > cap_out:
        raise Invalid("%d bytes, room for %d" % (offsets[-1], cap_out))
    if not final and not recs:
        return b"", [0], 0
    return b"".join(parts), offsets, consumed


def extract_cuts(text: bytes, cuts, keep):
    """The file in the chunks [0, cuts[0]), [cuts[0], cuts[1]) ..., what a call leaves handed over again in front of the
    next chunk, the last call final, ``keep`` indexed by the record's number in the file -> the list of
    (chunk, first record, records, out bytes, consumed)."""
    calls, left, done = [], b"", 0
    bounds = [0, *cuts, len(text)]
    for i in range(len(bounds) - 1):
        chunk = left + text[bounds[i]:bounds[i + 1]]
        final = i == len(bounds) - 2
        recs, _ = records_of(chunk, final) if chunk else ([], 0)
        out, _, m = extract_chunk(chunk, final, keep[done:done + len(recs)])
        calls.append((chunk, done, len(recs), out, m))
        done += len(recs)
        left = chunk[m:]
    return calls
