"""The run guesses of the binned path (``kb_guess_scale`` / ``kb_guess_scaled`` / ``kb_guess_run``, csrc/kdf_device.h) against
the exact integer divisions they replaced: ``tests/native/run_guess_check.cpp``, a stand-alone program built for the host
with -fsanitize=address,undefined and run as a subprocess (never loaded into Python).

* kernel C's factor: every ``total`` in [1, 2^20] and the powers of two +- 1 up to 2^32 - 1, ``nruns`` in {1, 2, 3, 255, 256,
  257, 511, 512, 1024}, at both ends, the middle and around the entries where the quotient steps;
* the piece sort's guess: every entry of every pair of up to 2100 entries, and the first 65 536 entries, the last and the
  middle ones of pairs of 2^12 .. 2^32 - 1 entries, with 1 .. 2048 runs;
* each with the reciprocal as the host divides it and one ulp to either side (the device's v_rcp_f32 is good to 1 ulp).

A guess must lie in [0, runs - 1] and differ from the exact one by at most one run; a zero divisor gives 0."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("run_guess_check")), "run_guess_check")
    src = os.path.join(ROOT, "tests", "native", "run_guess_check.cpp")
    inc = os.path.join(ROOT, "kmer_denovo_filter_amd", "csrc")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{inc}", src, "-o", out]
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    if shutil.which("g++"):
        cmd = ["g++"] + flags
    elif hipcc:
        cmd = [hipcc, "-x", "c++"] + flags                             # host only: no device pass
    else:
        raise RuntimeError("neither g++ nor hipcc: the run-guess program cannot be built")
    subprocess.run(cmd, check=True)
    return out


def test_guesses_are_within_one_run_of_the_exact_division(exe):
    pr = subprocess.run([exe], capture_output=True, text=True)
    assert pr.returncode == 0 and not pr.stderr.strip(), pr.stdout[-2000:] + pr.stderr[-4000:]
    got = dict(re.findall(r"^(kb_guess_\w+): (\d+) cases", pr.stdout, re.M))
    # both parts ran, over the ranges the docstring names (2^20 totals x 9 run counts x 3 reciprocals alone are 2.8e7)
    assert int(got["kb_guess_scale"]) > 100_000_000 and int(got["kb_guess_run"]) > 100_000_000, pr.stdout
    assert pr.stdout.count(" 0 out of bounds") == 2, pr.stdout
