"""The device feeder's DEFLATE decoder (csrc/kdf_inflate.h), compiled for the CPU with one lane: a stand-alone program
built with -fsanitize=address,undefined and run as a subprocess (never loaded into Python).

* every block zlib makes must decode byte for byte -- the decoder may reject NONE of them (the zlib fallback of the
  driver exists for what the decoder does not handle; for zlib-made input that set is empty);
* a few thousand seeded corruptions must each end in a status, with no sanitizer report;
* the short fixed list of corrupt blocks the GPU tests use is rejected cleanly here first;
* legal streams that zlib's encoder never writes (tests/deflate_writer.py; bamdev_cases.handmade_payloads) decode byte
  for byte as well, and none is rejected;
* 30 000 seeded mutants of small streams, each judged by zlib first: the decoder must give zlib's bytes for every one
  zlib accepts and a non-zero status for every other one."""
import os
import zlib

import pytest

import bamdev_cases as bc


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return bc.build_inflate_check(tmp_path_factory.mktemp("inflate_check"))


def test_valid_blocks_equal_zlib_and_none_is_rejected(exe, tmp_path):
    vs = bc.valid_payloads()
    res, _, pr = bc.run_inflate_check(exe, [(p, len(d), d) for _, p, d in vs], tmp_path)
    assert pr.returncode == 0, pr.stdout[-2000:] + pr.stderr[-4000:]
    assert len(res) == len(vs)
    for (label, _, _), (status, equal) in zip(vs, res):
        assert status == 0 and equal == 1, (label, status, equal)


def test_seeded_corruptions_end_in_a_status(exe, tmp_path):
    vs = bc.valid_payloads()
    n = 4000
    _, fuzz, pr = bc.run_inflate_check(exe, [(p, len(d), d) for _, p, d in vs], tmp_path, n_fuzz=n)
    assert pr.returncode == 0 and not pr.stderr.strip(), pr.stderr[-4000:]          # (a sanitizer report aborts the program)
    assert fuzz is not None and sum(fuzz) == n
    assert fuzz[0] > n // 2                                                         # most corruptions are detectable


def test_fixed_corrupt_list_is_rejected_cleanly(exe, tmp_path):
    cs = bc.corrupt_payloads()
    res, _, pr = bc.run_inflate_check(exe, [(p, isize, None) for _, p, isize in cs], tmp_path)
    assert pr.returncode == 0 and not pr.stderr.strip(), pr.stderr[-4000:]
    for (label, _, _), (status, _) in zip(cs, res):
        assert status != 0, label


def test_handmade_blocks_equal_zlib_and_none_is_rejected(exe, tmp_path):
    hs = bc.handmade_payloads()
    res, _, pr = bc.run_inflate_check(exe, [(p, len(d), d) for _, p, d in hs], tmp_path)
    assert not pr.stderr.strip(), pr.stderr[-4000:]
    assert len(res) == len(hs)
    for (label, _, _), (status, equal) in zip(hs, res):
        assert status == 0 and equal == 1, (label, status, equal)
    assert pr.returncode == 0


def test_zlib_refuses_every_illegal_neighbour():
    """deflate_writer.illegal() has asserted it while the list was built; here it is said of legal() itself"""
    import deflate_writer as dw
    ns = bc.illegal_neighbours()
    assert len(ns) == 11
    for label, p, _ in ns:
        with pytest.raises(zlib.error):
            dw.legal(p)


def test_mutants_get_zlibs_verdict_and_zlibs_bytes(exe, tmp_path):
    ms = list(bc.mutants())
    valid = [w for _, _, w in ms if w is not None]
    assert len(ms) == 30_000 and len(valid) >= 5000 and len(set(valid)) >= 3000          # (the test is not vacuous)
    res, _, pr = bc.run_inflate_check(exe, ms, tmp_path)
    os.remove(tmp_path / "cases.bin")                                                    # (tens of MB: not kept with the test's other files)
    assert not pr.stderr.strip(), pr.stderr[-4000:]                                      # (a sanitizer report aborts the program)
    assert len(res) == len(ms)
    wrong = [(i, status, equal) for i, ((_, _, w), (status, equal)) in enumerate(zip(ms, res))
             if ((status, equal) != (0, 1) if w is not None else status == 0)]
    assert not wrong, (len(wrong), wrong[:10])
    assert pr.returncode == 0
    assert {status for (_, _, w), (status, _) in zip(ms, res) if w is None} >= set(range(1, 8))
