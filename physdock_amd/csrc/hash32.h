// The two 32-bit hash functions of the ligand graph kernels (fingerprint.hip, canonical.hip), mod 2^32: the finaliser of MurmurHash3
// and one chaining step over it.  tests/fingerprint_ref.py holds the same two in Python integers.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ unsigned fp_fmix(unsigned h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
__device__ __forceinline__ unsigned fp_push(unsigned h, unsigned v) { return fp_fmix(h * 0x01000193u + v + 0x9E3779B9u); }
