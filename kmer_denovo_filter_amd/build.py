"""Build libkdf.so (HIP kernels + C ABI) in-tree for gfx950.

``python -m kmer_denovo_filter_amd.build`` or ``build_native()``.  hipcc
cross-compiles without a GPU; the resulting ``kmer_denovo_filter_amd/libkdf.so``
is git-ignored but travels to the GPU box with the tree.

The units are compiled concurrently, and each is rebuilt when a file it includes
changed: the compiler writes the list (``<unit>.d``, beside ``<unit>.o``).
"""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

_PKG = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_PKG, "csrc")
_INC = os.path.join(os.path.dirname(_PKG), "include")
LIB_PATH = os.path.join(_PKG, "libkdf.so")

# DPP wave scans for uniform-address atomics with per-lane values: this toolchain's default is an iterative
# loop over the active lanes (~8 instructions per lane), which made the bucket kernels scalar-issue bound
_ENGINE_FLAGS = ["--offload-arch=gfx950", "-O3", "-mllvm", "-amdgpu-atomic-optimizer-strategy=DPP"]
_SOURCES = [
    ("kdf_engine.hip", _ENGINE_FLAGS),               # the core: by far the longest compile, so it starts first
    ("kdf_engine_reads.hip", _ENGINE_FLAGS),
    ("kdf_spool.hip", _ENGINE_FLAGS),
    ("kdf_kmerfasta.hip", _ENGINE_FLAGS),
    ("kdf_fastafeed.hip", _ENGINE_FLAGS),
    ("kdf_fastqfeed.hip", _ENGINE_FLAGS),
    ("kdf_indexcodec.hip", _ENGINE_FLAGS),
    ("kdf_sort.hip", ["--offload-arch=gfx950", "-O3"]),
    ("kdf_host.cpp", ["-O2", "-x", "c++"]),          # host only: no device pass
]


def _jobs() -> int:
    try:
        n = int(os.environ.get("MAX_JOBS", "") or 8)
    except ValueError:
        n = 8
    return max(1, min(len(_SOURCES), n, 16))


def _dep_files(d: str):
    """The prerequisites a compiler-written .d file names (make syntax: `target: a b \\` ...)."""
    with open(d) as f:
        text = f.read().replace("\\\n", " ")
    return text.split(":", 1)[1].split() if ":" in text else []


def _fresh(o: str, d: str) -> bool:
    """o is newer than every file its unit was compiled from."""
    if not (os.path.exists(o) and os.path.exists(d)):
        return False
    t = os.path.getmtime(o)
    try:
        return all(os.path.getmtime(p) <= t for p in _dep_files(d))
    except OSError:                                  # a file the unit included is gone
        return False


def _compile(cmd, o: str, d: str) -> subprocess.CompletedProcess:
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:                            # nothing half-made may pass for this unit's object next time
        for p in (o, d):
            if os.path.exists(p):
                os.remove(p)
    return r


def build_native(force: bool = False, verbose: bool = False) -> str:
    hipcc = os.environ.get("HIPCC", "hipcc")
    extra = os.environ.get("KDF_EXTRA_FLAGS", "").split()      # experiments: -DSK_C_THREADS=512 ...
    objs, todo = [], []
    for src, flags in _SOURCES:
        s = os.path.join(_CSRC, src)
        o = os.path.join(_CSRC, os.path.splitext(src)[0] + ".o")
        d = os.path.splitext(o)[0] + ".d"
        objs.append(o)
        if not force and _fresh(o, d):
            continue
        todo.append(([hipcc, *flags, *extra, "-fPIC", "-std=c++17", f"-I{_INC}", f"-I{_CSRC}", "-MD", "-MF", d, "-c", s, "-o", o], o, d))
    if todo:
        if verbose:
            for cmd, _, _ in todo:
                print(" ".join(cmd), file=sys.stderr)
        with ThreadPoolExecutor(max_workers=_jobs()) as pool:
            results = list(pool.map(lambda t: _compile(*t), todo))
        failed = None
        for r in results:                            # every unit's compiler output, in the order of _SOURCES
            if r.stdout:
                sys.stderr.write(r.stdout)
            if r.returncode != 0 and failed is None:
                failed = r
        if failed is not None:
            raise subprocess.CalledProcessError(failed.returncode, failed.args, output=failed.stdout)
    if force or todo or not os.path.exists(LIB_PATH) or any(os.path.getmtime(o) > os.path.getmtime(LIB_PATH) for o in objs):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", f"-Wl,--version-script={os.path.join(_CSRC, 'libkdf.map')}",
               "-o", LIB_PATH, *objs, "-lz"]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.run(cmd, check=True)
    return LIB_PATH


if __name__ == "__main__":
    print(build_native(force="--force" in sys.argv, verbose=True))
