"""The owning buffers of the engine's host side (``DevBuf`` / ``PinBuf`` / ``dev_reserve``, csrc/kdf_devbuf.h):
``tests/native/devbuf_check.cpp``, a stand-alone program built for the host with -fsanitize=address,undefined against the
counting allocator of ``tests/native/hipstub`` and run as a subprocess (never loaded into Python).

The destructor frees; a move leaves its source empty and nothing is freed twice; ``dev_reserve`` with room already there
calls neither ``quiesce`` nor the allocator; a failing ``quiesce`` keeps pointer and size; a failing allocation leaves the
buffer empty and returns the error; no allocation is live at exit."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("devbuf_check")), "devbuf_check")
    src = os.path.join(ROOT, "tests", "native", "devbuf_check.cpp")
    stub = os.path.join(ROOT, "tests", "native", "hipstub")           # its hip/hip_runtime.h comes first
    inc = os.path.join(ROOT, "kmer_denovo_filter_amd", "csrc")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{stub}", f"-I{inc}", src, "-o", out]
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    if shutil.which("g++"):
        cmd = ["g++"] + flags
    elif hipcc:
        cmd = [hipcc, "-x", "c++"] + flags                             # host only: no device pass
    else:
        raise RuntimeError("neither g++ nor hipcc: the buffer program cannot be built")
    subprocess.run(cmd, check=True)
    return out


def test_buffers_own_move_and_reserve(exe):
    pr = subprocess.run([exe], capture_output=True, text=True)
    assert pr.returncode == 0 and not pr.stderr.strip(), pr.stdout[-2000:] + pr.stderr[-4000:]
    m = re.search(r"^devbuf: (\d+) checks, (\d+) failed, (\d+) live allocations at exit, (\d+) bad frees$", pr.stdout, re.M)
    assert m, pr.stdout
    checks, failed, live, bad = map(int, m.groups())
    assert checks >= 38 and failed == 0 and live == 0 and bad == 0, pr.stdout
