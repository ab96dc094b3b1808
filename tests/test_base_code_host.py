"""``kdf_base_code`` (csrc/kdf_text.h), the one base code of the text kernels, on the host against the Python key codec
(``keys.encode``): ``tests/native/base_code_check.cpp``, a stand-alone program built for the host with
-fsanitize=address,undefined and run as a subprocess (never loaded into Python).  All 256 byte values: A/C/G/T in either
case are 0 .. 3 as the codec has them, every other byte is 4 where the codec says 255."""
import os
import shutil
import subprocess

import numpy as np

from kmer_denovo_filter_amd import keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_base_code_equals_the_key_codec(tmp_path):
    out = str(tmp_path / "base_code_check")
    src = os.path.join(ROOT, "tests", "native", "base_code_check.cpp")
    inc = os.path.join(ROOT, "kmer_denovo_filter_amd", "csrc")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{inc}", src, "-o", out]
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    if shutil.which("g++"):
        cmd = ["g++"] + flags
    elif hipcc:
        cmd = [hipcc, "-x", "c++"] + flags                             # host only: no device pass
    else:
        raise RuntimeError("neither g++ nor hipcc: the base-code program cannot be built")
    subprocess.run(cmd, check=True)
    pr = subprocess.run([out], capture_output=True, text=True)
    assert pr.returncode == 0 and not pr.stderr.strip(), pr.stdout[-2000:] + pr.stderr[-4000:]
    got = np.array(pr.stdout.split(), dtype=np.int64)
    want = keys.encode(np.arange(256, dtype=np.uint8)).astype(np.int64)
    want[want == 255] = 4
    assert got.shape == (256,) and np.array_equal(got, want), (got, want)
    assert sorted(np.flatnonzero(want < 4).tolist()) == sorted(b"ACGTacgt")
