// kdf_sort.h -- what kdf_sort.hip offers beyond the two dump sorts (those are declared where they are used, in
// kdf_engine.hip): the permutation of a multi-word LSD sort, for callers that gather through it themselves
// (kdf_regions.h).  Host only.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>

// One stable pass: item i's key word is keys[i * stride], of which bits [begin_bit, end_bit) take part.
struct KdfSortPass {
    const uint64_t *keys;
    uint64_t stride;
    int begin_bit, end_bit;
};

// d_perm[0 .. n): the order of the n items ascending by the passes' words, passes[0] the LEAST significant (so equal
// items keep their input order).  Nothing is gathered: the keys stay where they are.  n < 2^32; scratch (24 bytes per
// item and rocPRIM's own) is allocated and freed per call, and the call synchronises the stream.
int kdf_sort_perm_device(const KdfSortPass *passes, int n_passes, uint64_t n, uint32_t *d_perm, hipStream_t stream, std::string &err);
