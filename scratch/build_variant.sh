#!/bin/bash
# usage (here, no GPU needed): scratch/build_variant.sh NAME -DFOO=1 ...   -> scratch/variants/libkdf_NAME.so
# (kernel variants for same-box A/B runs on the GPU box: scratch/sweep_variants.sh swaps them in one after the other)
# Every engine unit (build.py's _SOURCES with the engine's flags) is compiled with the variant's flags, side by side;
# kdf_sort.o and kdf_host.o are taken from the ordinary build when it has left them.
set -e
cd "$(dirname "$0")/.."
name=$1; shift
C=kmer_denovo_filter_amd/csrc
UNITS="kdf_engine kdf_engine_reads kdf_spool"
mkdir -p scratch/variants /tmp/kdfvar_$name
pids=""
for u in $UNITS; do
    hipcc --offload-arch=gfx950 -O3 -mllvm -amdgpu-atomic-optimizer-strategy=DPP "$@" -fPIC -std=c++17 -Iinclude -I$C -c $C/$u.hip -o /tmp/kdfvar_$name/$u.o &
    pids="$pids $!"
done
for p in $pids; do wait $p; done
[ -f $C/kdf_sort.o ] || hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -Iinclude -I$C -c $C/kdf_sort.hip -o $C/kdf_sort.o
[ -f $C/kdf_host.o ] || hipcc -O2 -x c++ -fPIC -std=c++17 -Iinclude -I$C -c $C/kdf_host.cpp -o $C/kdf_host.o
objs=""
for u in $UNITS; do objs="$objs /tmp/kdfvar_$name/$u.o"; done
hipcc --offload-arch=gfx950 -shared -fPIC -Wl,--version-script=$C/libkdf.map -o scratch/variants/libkdf_$name.so $objs $C/kdf_sort.o $C/kdf_host.o -lz
echo built scratch/variants/libkdf_$name.so
