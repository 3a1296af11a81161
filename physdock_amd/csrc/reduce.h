// Wave and block reductions shared by the kernels (included by common.h).  Every result is returned to every lane / thread, and
// every tree is fixed, so a reduction gives the same bits from run to run.
#pragma once
#include <hip/hip_runtime.h>

// xor butterfly over the 64 lanes of a wave: v is the own value, w the partner's
#define PD_WAVE_REDUCE(NAME, T, COMBINE)                          \
    __device__ __forceinline__ T NAME(T v) {                      \
        _Pragma("unroll") for (int o = 32; o > 0; o >>= 1) {      \
            const T w = __shfl_xor(v, o);                         \
            v = COMBINE;                                          \
        }                                                         \
        return v;                                                 \
    }
PD_WAVE_REDUCE(wave_sum, float, v + w)
PD_WAVE_REDUCE(wave_sum, double, v + w)
PD_WAVE_REDUCE(wave_sum, int, v + w)
PD_WAVE_REDUCE(wave_sum, unsigned, v + w)
PD_WAVE_REDUCE(wave_max, float, fmaxf(v, w))
PD_WAVE_REDUCE(wave_max, double, fmax(v, w))
PD_WAVE_REDUCE(wave_min, float, fminf(v, w))
PD_WAVE_REDUCE(wave_min, double, fmin(v, w))
PD_WAVE_REDUCE(wave_or, int, v | w)
#undef PD_WAVE_REDUCE

// sum of one float64 per thread of an NT-thread block (NT a power of two, sh holds NT doubles) by a halving tree in LDS
template <int NT>
__device__ __forceinline__ double block_sum_det(double v, double* sh) {
    __syncthreads();
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    return sh[0];
}

// The same for a block of EXACTLY 256 threads = four waves: a butterfly per wave, then the four wave partials (red holds 4 doubles).
// The butterflies are written out: through wave_sum / wave_max hipcc schedules the kernels of mmff.hip and conformers.hip differently.
__device__ __forceinline__ double block_sum_d(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ double block_max_d(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

// lanes that share one atom's terms in such a block: the largest power of two <= 256 / L, at most `widest` (lanes of one wave, adjacent)
__device__ __forceinline__ int threads_per_atom(int L, int widest) {
    int t = widest;
    while (t > 1 && t * L > 256) t >>= 1;
    return t;
}
