"""The entry map of the binned path's gathers (``kb_entry_off``, csrc/kdf_device.h: kernel C's narrow path and the pipelined
piece sort): ``tests/native/entry_map_check.cpp``, a stand-alone program built for the host with
-fsanitize=address,undefined and run as a subprocess (never loaded into Python).

For segment widths S in {8, 16, 32, 64} and E in {8, 12, 16} entries per lane:

* (lane, step) -> offset is a bijection onto [0, 64 E);
* S = 64 is the plain map 64 q + l;
* the offset is the lane's first entry plus S q;
* for a wave block cut at any ``live`` in [0, 64 E], the steps with at least one live lane are the prefix
  q < min(E, ceil(live / S)), the first entry of step q is lane 0's at S q (the bound ``wbase + S q0`` of kernel C's
  wave-uniform exits), and a lane whose first entry is dead has none alive."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("entry_map_check")), "entry_map_check")
    src = os.path.join(ROOT, "tests", "native", "entry_map_check.cpp")
    inc = os.path.join(ROOT, "kmer_denovo_filter_amd", "csrc")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{inc}", src, "-o", out]
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    if shutil.which("g++"):
        cmd = ["g++"] + flags
    elif hipcc:
        cmd = [hipcc, "-x", "c++"] + flags                             # host only: no device pass
    else:
        raise RuntimeError("neither g++ nor hipcc: the entry-map program cannot be built")
    subprocess.run(cmd, check=True)
    return out


def test_entry_map_is_a_bijection_with_prefix_steps(exe):
    pr = subprocess.run([exe], capture_output=True, text=True)
    assert pr.returncode == 0 and not pr.stderr.strip(), pr.stdout[-2000:] + pr.stderr[-4000:]
    got = re.findall(r"^kb_entry_off S = (\d+) E = (\d+): (\d+) cases", pr.stdout, re.M)
    assert sorted((int(s), int(e)) for s, e, _ in got) == sorted((s, e) for s in (8, 16, 32, 64) for e in (8, 12, 16)), pr.stdout
    # every (lane, step) and every cut of every block was looked at: 64 E + (64 E + 1) E cases
    assert all(int(n) == 64 * int(e) + (64 * int(e) + 1) * int(e) for _, e, n in got), pr.stdout
    assert "kb_entry_off: 0 failures" in pr.stdout, pr.stdout
