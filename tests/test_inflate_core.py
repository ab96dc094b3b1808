"""The device feeder's DEFLATE decoder (csrc/kdf_inflate.h), compiled for the CPU with one lane: a stand-alone program
built with -fsanitize=address,undefined and run as a subprocess (never loaded into Python).

* every block zlib makes must decode byte for byte -- the decoder may reject NONE of them (the zlib fallback of the
  driver exists for what the decoder does not handle; for zlib-made input that set is empty);
* a few thousand seeded corruptions must each end in a status, with no sanitizer report;
* the short fixed list of corrupt blocks the GPU tests use is rejected cleanly here first."""
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
