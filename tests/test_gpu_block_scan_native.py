"""The DPP wave scans, the block scans on them and kernel A's strip scan (csrc/kdf_scan.h) against host prefix sums:
``tests/native/block_scan_check.hip``, a stand-alone program compiled for gfx950 and run once as a child process.

Block scans (exclusive prefix; total where the scan returns one) of workgroups of 64, 128, 256, 512, 768 and 1024 threads:
all zeros, all ones, the lane index, random values with a sum below 2^32, values whose sum wraps 2^32, and a single
non-zero value at lanes 0, 15, 16, 31, 32, 47, 48 and 63 of the first, a middle and the last wave.  The strip scan: every
``nb`` in 1, 2, 4 .. 1024 with counts that sum to at most 16 384, and nothing written past ``offs[nb]``.

Block sums (``kb_block_sum`` on uint32 and on 64-bit values, ``kb_block_max``) of workgroups of 64, 256 and 1024 threads:
all zeros, all ones, one non-zero value at lane 0 and at lane 63 of the first and of the last wave, a 32-bit sum that
wraps, a 64-bit sum beyond 2^32.  The scan of 64-bit block sums by one workgroup (``kb_sums_exscan``): n = 0, 1, 255, 256,
257, 511, 513 and 65 537, random values below 2^40 and values ``1 << 32 | len``, the total through every thread and
nothing written at or past ``sums[n]``."""
import os
import re
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scans_equal_host_prefix_sums(tmp_path):
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    assert hipcc, "hipcc: the scan program cannot be built"
    exe = str(tmp_path / "block_scan_check")
    src = os.path.join(ROOT, "tests", "native", "block_scan_check.hip")
    inc = os.path.join(ROOT, "kmer_denovo_filter_amd", "csrc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{inc}", src, "-o", exe], check=True)
    pr = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert pr.returncode == 0, pr.stdout[-4000:] + pr.stderr[-4000:]
    got = dict((name, int(n)) for name, n in re.findall(r"^(block scans|strip scans|block sums|sums scans): (\d+) cases", pr.stdout, re.M))
    assert got == {"block scans": 6 * 29 * 2, "strip scans": 11 * 6, "block sums": 3 * 2 * 7, "sums scans": 2 * 8} and "\n0 wrong" in pr.stdout, pr.stdout
