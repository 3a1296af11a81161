// Philox4x32-10 (Salmon et al., SC'11): the one counter-based generator of the package.  Its bits are pinned by
// tests/test_sampler_kernels_gpu.py and by every seeded test of the conformer and Vina-search kernels.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

struct Philox {
    uint32_t k0, k1;
    // c -> the four 32-bit words of block c under the key (k0, k1)
    __device__ __forceinline__ void gen(uint32_t (&c)[4]) const {
        uint32_t a = k0, b = k1;
#pragma unroll
        for (int i = 0; i < 10; ++i) {
            const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
            const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ a, n1 = (uint32_t)p1;
            const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ b, n3 = (uint32_t)p0;
            c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
            a += 0x9E3779B9u; b += 0xBB67AE85u;
        }
    }
};
