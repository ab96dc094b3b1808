"""The layout of a host form's staging frame (``StageLayout``, csrc/kdf_engine_priv.h): ``tests/native/stage_layout_check.cpp``,
a stand-alone program built for the host with -fsanitize=address,undefined and run as a subprocess (never loaded into
Python).  It includes the header's host-only part alone, so the layout arithmetic holds no HIP call.

Over 6000 random lists of 1 to 16 items, sizes drawn from {0, 1, 15, 16, 255, 256, 257, 4095, 4096, random up to 2^33}:
every non-empty item is 256-aligned, items do not overlap, the total is at least the sum of the sizes and at most that plus
256 bytes of padding per item, an empty item resolves to null, and offsets are ``size_t`` (no wrap for a 2^33-byte item)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("stage_layout_check")), "stage_layout_check")
    src = os.path.join(ROOT, "tests", "native", "stage_layout_check.cpp")
    inc = os.path.join(ROOT, "kmer_denovo_filter_amd", "csrc")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{inc}", src, "-o", out]
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    if shutil.which("g++"):
        cmd = ["g++"] + flags
    elif hipcc:
        cmd = [hipcc, "-x", "c++"] + flags                             # host only: no device pass
    else:
        raise RuntimeError("neither g++ nor hipcc: the stage-layout program cannot be built")
    subprocess.run(cmd, check=True)
    return out


def test_items_are_aligned_disjoint_and_tightly_packed(exe):
    pr = subprocess.run([exe], capture_output=True, text=True)
    assert pr.returncode == 0 and not pr.stderr.strip(), pr.stdout[-2000:] + pr.stderr[-4000:]
    m = re.search(r"^stage_layout: (\d+) lists, (\d+) items, (\d+) empty, (\d+) of 4 GB and more, (\d+) broken rules$", pr.stdout, re.M)
    assert m, pr.stdout
    lists, items, empty, huge, bad = map(int, m.groups())
    # a few thousand lists ran, with empty items and items past 2^32 bytes among them
    assert lists >= 3000 and items >= lists and empty > 1000 and huge > 100 and bad == 0, pr.stdout
