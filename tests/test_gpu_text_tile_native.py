"""What the text kernels share (csrc/kdf_text.h) against the host: ``tests/native/text_tile_check.hip``, a stand-alone
program compiled for gfx950 and run once as a child process.

The granule load: texts of 0, 1, 15, 16, 17, 4095, 4096 and 4097 random bytes at 0, 1 and 15 bytes behind a 16-byte
boundary, the granules at text offset -15, at 0 and the last one, and the one at 0 again with a lower bound of 3, byte for
byte with the fill value outside the bounds.
The backward search ``kt_last_outside``: texts of 0, 1, 255, 256, 257 and 513 bytes whose trailing run is the whole
text, empty, ends on a round boundary or crosses one.  ``kdf_base_code``: all 256 byte values, device against host."""
import os
import re
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_text_primitives_equal_the_host(tmp_path):
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    assert hipcc, "hipcc: the text program cannot be built"
    exe = str(tmp_path / "text_tile_check")
    src = os.path.join(ROOT, "tests", "native", "text_tile_check.hip")
    inc = os.path.join(ROOT, "kmer_denovo_filter_amd", "csrc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{inc}", src, "-o", exe], check=True)
    pr = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert pr.returncode == 0, pr.stdout[-4000:] + pr.stderr[-4000:]
    got = dict((name, int(n)) for name, n in re.findall(r"^(granules|last outside|base codes): (\d+) cases", pr.stdout, re.M))
    assert got == {"granules": 8 * 3 * (3 + 1), "last outside": 6 * 4, "base codes": 256} and "\n0 wrong" in pr.stdout, pr.stdout
