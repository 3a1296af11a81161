// Sets of up to 128 atoms as two 64-bit words, shared by the ligand graph kernels (ligand_features.hip, aromaticity.hip): one ligand
// has at most 128 atoms, so an atom's neighbours, a search front or a path fit one Mask.
#pragma once
#include <hip/hip_runtime.h>

typedef unsigned long long u64;

struct Mask {
    u64 lo, hi;
};
__device__ __forceinline__ bool mk_any(Mask m) { return (m.lo | m.hi) != 0; }
__device__ __forceinline__ bool mk_has(Mask m, int a) { return ((a < 64 ? m.lo >> a : m.hi >> (a - 64)) & 1ull) != 0; }
__device__ __forceinline__ Mask mk_bit(int a) { return a < 64 ? Mask{1ull << a, 0ull} : Mask{0ull, 1ull << (a - 64)}; }
__device__ __forceinline__ Mask mk_or(Mask a, Mask b) { return Mask{a.lo | b.lo, a.hi | b.hi}; }
__device__ __forceinline__ Mask mk_and(Mask a, Mask b) { return Mask{a.lo & b.lo, a.hi & b.hi}; }
__device__ __forceinline__ Mask mk_andn(Mask a, Mask b) { return Mask{a.lo & ~b.lo, a.hi & ~b.hi}; }
__device__ __forceinline__ int mk_first(Mask m) { return m.lo ? __ffsll((long long)m.lo) - 1 : 63 + __ffsll((long long)m.hi); }
// the atoms above a (a in 0 .. 127)
__device__ __forceinline__ Mask mk_above(int a) {
    return a < 63 ? Mask{~0ull << (a + 1), ~0ull} : (a == 63 ? Mask{0ull, ~0ull} : (a < 127 ? Mask{0ull, ~0ull << (a - 63)} : Mask{0ull, 0ull}));
}
